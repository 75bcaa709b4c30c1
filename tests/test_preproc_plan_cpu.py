"""CPU (`-m "not gpu"`): what the preprocessing host layer (csrc/preproc_plan.h) decides, as values.

vq_debug_resample_plan builds the coefficient tables and the plan of a Pillow resize without touching a device; its three
switches are arguments, so nothing here depends on the environment.  vq_debug_preproc_small_plans returns slice_frames, the
scene batch plan and PostLayout.

The pinned tables hold what the resampler launched BEFORE the plan existed (commit 87ce963), read off that commit's
vq_preproc.hip by hand: run_device's decision loop (span_max, the oc search under the 40 / 48 KiB caps, the fallback from the
row-block-major to the segment-major kernel, dword_store, the segments per workgroup, both grids, the three-way vertical
if-chain), PostLayout, scene_run_device's batch arithmetic and the slice expressions of the four host-frame loops were
copied line by line into a throw-away host program, launches replaced by recording their arguments; its printed answers
are the literals below.  The same program agreed with preproc_plan.h, table for table and field for field, on 13,951,100
combinations at the time: both Pillow filters x h in {1, 5, 37, 1080} x w from 1 to 6000 (every w below 70, then steps of 13,
then of 97) x out_w from 1 to 1024 (every one below 40, then steps of 7, then of 61) x five crops (whole, a window at
out_w / 4, the last column alone, crop_left = 1 with crop_w = out_w - 3, crop_left = 3 with crop_w % 4 == 0) x
n in {1, 3, 64, 65535} x {no switch, seg, 32 KB, 64 KB, spw 1, spw 3} with mixed base alignments, and the small plans on
their own grids.  test_every_plan_keeps_the_kernels_preconditions repeats a 100,000-plan product of that grid on the library alone,
against Pillow's bounds as restated here."""
import ctypes
import itertools

import numpy as np
import pytest

BILINEAR, BICUBIC = 2, 3
KB = 1024
# the parity cases of tests/test_gpu_parity.py::test_resample_ragged_sizes_filters_crops_vs_oracle: (h, w, out_w, out_h); each runs
# whole and with the window (out_h // 3, out_w // 4, max(1, out_h // 2), max(1, out_w // 2)), in both filters, on 3 frames (1 of a
# large size).
RAGGED_CASES = [(37, 53, 224, 224), (300, 400, 201, 640), (2, 3, 7, 5), (1, 1, 4, 4), (500, 224, 224, 100), (64, 64, 64, 17),
                (1080, 1920, 398, 224), (719, 405, 224, 397), (5, 5461, 31, 9), (480, 640, 640, 480)]
# (n, h, w, out_w, out_h): several segments per workgroup.  A workgroup walks more than one segment only when row blocks x frames
# exceed 4 * 768 / segments, which a few frames of a few hundred pixels never do (the benchmark's 64 frames of 1080p do): the
# smallest such call is many tiny frames scaled up to 32 segments.
MANY_FRAMES_CASE = (100, 2, 16, 1024, 2)


def ragged_frames(h, w):
    return 3 if h * w < 200000 else 1


def ragged_window(ow, oh):
    return oh // 3, ow // 4, max(1, oh // 2), max(1, ow // 2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    return _lib.load()


def plan(lib, h, w, filt, out_h, out_w, crop=None, n=1, tmp_align=0, dst_align=0, seg=0, lds_kb=0, spw=0):
    """The vq_resample_plan, or the error text."""
    from video_quierer_amd._lib import ResamplePlanC
    out = ResamplePlanC()
    top, left, ch, cw = crop if crop is not None else (0, 0, out_h, out_w)
    rc = lib.vq_debug_resample_plan(h, w, filt, out_h, out_w, top, left, ch, cw, n, tmp_align, dst_align, seg, lds_kb, spw, ctypes.byref(out))
    if rc != 0:
        assert rc == -1          # VQ_ERR_INVALID
        return lib.vq_last_error().decode()
    return out


def fields(p):
    return (p.row_first, p.rows_needed, p.tmp_bytes, p.hx, p.oc, p.pitch_dw, p.tile_pitch, p.lds, p.dword_store, p.spw,
            (p.hgrid_x, p.hgrid_y, p.hgrid_z), p.vvec, (p.vgrid_x, p.vgrid_y, p.vgrid_z))


# (h, w, filter, out_h, out_w, crop, n, tmp_align, dst_align, seg, lds_kb, spw):
#     (row_first, rows_needed, tmp_bytes, hx, oc, pitch_dw, tile_pitch, lds, dword_store, spw, horizontal grid, vertical width, vertical grid)
PINNED = {
    # the benchmark's leg
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 0, 0, 0, 0): (0, 1080, 46448640, 1, 16, 123, 52, 36096, 1, 5, (3, 17, 64), 16, (37, 1, 64)),
    # the CLIP processor's bicubic 398 x 224 with its centre crop
    (1080, 1920, 3, 224, 398, (0, 87, 224, 224), 64, 0, 0, 0, 0, 0): (0, 1080, 46448640, 1, 28, 125, 84, 40064, 1, 3, (3, 17, 64), 16, (37, 1, 64)),
    (1080, 1920, 3, 224, 398, (0, 87, 224, 224), 1, 0, 0, 0, 0, 0): (0, 1080, 725760, 1, 28, 125, 84, 40064, 1, 1, (8, 17, 1), 16, (37, 1, 1)),
    # a single output column too wide for a request: segment-major
    (5, 5461, 2, 9, 31, (0, 0, 9, 31), 1, 0, 0, 0, 0, 0): (0, 5, 465, 0, 1, 271, 4, 71056, 0, 1, (31, 1, 1), 1, (1, 9, 1)),
    (5, 5461, 3, 9, 31, (0, 0, 9, 31), 1, 0, 0, 0, 0, 0): (0, 5, 465, 0, 1, 535, 4, 140048, 0, 1, (31, 1, 1), 1, (1, 9, 1)),
    (2, 3, 2, 5, 7, (0, 0, 5, 7), 3, 0, 0, 0, 0, 0): (0, 2, 126, 1, 32, 15, 100, 10752, 0, 1, (1, 1, 3), 1, (1, 5, 3)),
    (1, 1, 3, 4, 4, (0, 0, 4, 4), 3, 0, 0, 0, 0, 0): (0, 1, 36, 1, 32, 13, 100, 10752, 1, 1, (1, 1, 3), 4, (1, 4, 3)),
    # one row per switch value: $VQ_AMD_RSH=seg, $VQ_AMD_RSH_LDS_KB=32 / 64, $VQ_AMD_RSH_SPW=1 / 3
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 0, 1, 0, 0): (0, 1080, 46448640, 0, 20, 141, 60, 41536, 1, 1, (12, 17, 64), 16, (37, 1, 64)),
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 0, 0, 32, 0): (0, 1080, 46448640, 1, 12, 97, 36, 28096, 1, 7, (3, 17, 64), 16, (37, 1, 64)),
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 0, 0, 64, 0): (0, 1080, 46448640, 1, 28, 199, 84, 58560, 1, 3, (3, 17, 64), 16, (37, 1, 64)),
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 0, 0, 0, 1): (0, 1080, 46448640, 1, 16, 123, 52, 36096, 1, 1, (14, 17, 64), 16, (37, 1, 64)),
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 0, 0, 0, 3): (0, 1080, 46448640, 1, 16, 123, 52, 36096, 1, 3, (5, 17, 64), 16, (37, 1, 64)),
    # the frame limit; the A/B line where planning dominates; the table-cache test's geometry
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 65535, 0, 0, 0, 0, 0): (0, 1080, 47562681600, 1, 16, 123, 52, 36096, 1, 14, (1, 17, 65535), 16, (37, 1, 65535)),
    (90, 160, 2, 224, 224, (0, 0, 224, 224), 8, 0, 0, 0, 0, 0): (0, 90, 483840, 1, 32, 31, 100, 14848, 1, 1, (7, 2, 8), 16, (37, 1, 8)),
    (37, 53, 2, 24, 40, (0, 0, 24, 40), 3, 0, 0, 0, 0, 0): (0, 37, 13320, 1, 32, 45, 100, 18944, 1, 1, (2, 1, 3), 4, (1, 24, 3)),
    # a caller's output / an intermediate that is not 16-byte aligned: 4-byte accesses
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 0, 4, 0, 0, 0): (0, 1080, 46448640, 1, 16, 123, 52, 36096, 1, 5, (3, 17, 64), 4, (1, 224, 64)),
    (1080, 1920, 2, 224, 224, (0, 0, 224, 224), 64, 8, 0, 0, 0, 0): (0, 1080, 46448640, 1, 16, 123, 52, 36096, 1, 5, (3, 17, 64), 4, (1, 224, 64)),
    # an upscale with a window
    (300, 400, 3, 640, 201, (213, 50, 320, 100), 3, 0, 0, 0, 0, 0): (98, 154, 138600, 1, 32, 65, 100, 24576, 1, 1, (4, 3, 3), 4, (1, 320, 3)),
}


def test_plans_of_todays_shapes(lib):
    for (h, w, filt, oh, ow, crop, n, ta, da, seg, kb, spw), want in PINNED.items():
        p = plan(lib, h, w, filt, oh, ow, crop, n, ta, da, seg, kb, spw)
        assert not isinstance(p, str), p
        assert fields(p) == want, (h, w, filt, oh, ow, crop, n, ta, da, seg, kb, spw)
        assert p.row_bytes == crop[3] * 3 and p.ksize_h % 4 == 0 and p.ksize_v % 4 == 0


def pillow_bounds(in_size, out_size, filt, _cache={}):
    """Pillow's precompute_coeffs bounds, restated here from Resample.c: (first tap, one past the last tap) per output index."""
    key = (in_size, out_size, filt)
    if key not in _cache:
        scale = in_size / out_size
        support = (2.0 if filt == BICUBIC else 1.0) * max(scale, 1.0)
        centers = [(x + 0.5) * scale for x in range(out_size)]
        first = np.array([max(int(c - support + 0.5), 0) for c in centers])
        end = np.array([min(int(c + support + 0.5), in_size) for c in centers])
        _cache[key] = (first, end)
    return _cache[key]


def check_invariants(p, case, geometry, crop, n, default_switches):
    h, w, filt, out_h, out_w = geometry
    top, left, crop_h, crop_w = crop
    lds_max, slack = (96 * KB, 48) if p.hx else (150 * KB, 24)
    assert 0 < p.lds <= lds_max, case                                            # the kernel's dynamic-LDS limit
    assert p.lds == 64 * p.pitch_dw * 4 + 64 * p.tile_pitch + p.oc * p.ksize_h * 4, case
    assert p.pitch_dw % 2 == 1 and (p.tile_pitch // 4) % 2 == 1 and p.tile_pitch % 4 == 0 and p.tile_pitch >= p.oc * 3, case
    if p.hx:
        assert p.pitch_dw * 4 <= 1024 and p.oc * p.ksize_h <= 4 * 256, case      # one request per staged row; weights in four registers
    elif default_switches:
        assert p.oc == 1, case       # only a column wider than a request leaves the row-block-major kernel, and it fills 48 KiB alone
    assert 1 <= p.oc <= 32 and p.spw >= 1 and (p.hx or p.spw == 1), case
    # every segment's source span, from Pillow's bounds as restated above (not from the plan's own tables), fits the staged row
    first, end = pillow_bounds(w, out_w, filt)
    starts = np.arange(0, crop_w, p.oc)
    span = int((np.maximum.reduceat(end[left:left + crop_w], starts) - first[left + starts]).max())
    assert span * 3 + slack <= p.pitch_dw * 4 and p.span == span and end.max() <= w, (case, span)
    assert int((end - first).max()) <= p.ksize_h, case                           # a table row holds every tap
    # ... and the rows the vertical pass reads are the rows the horizontal pass produces
    vfirst, vend = pillow_bounds(h, out_h, filt)
    assert p.row_first == vfirst[top] and p.rows_needed == vend[top + crop_h - 1] - vfirst[top], case
    assert vfirst[top:top + crop_h].min() >= p.row_first and vend[top:top + crop_h].max() <= p.row_first + p.rows_needed <= h, case
    if p.dword_store:
        assert crop_w % 4 == 0 and p.oc % 4 == 0, case
    nseg = -(-crop_w // p.oc)
    assert p.hgrid_x * p.spw >= nseg > (p.hgrid_x - 1) * p.spw, case
    assert p.hgrid_y * 64 >= p.rows_needed > (p.hgrid_y - 1) * 64 and p.hgrid_z == n, case
    assert p.tmp_bytes == n * p.rows_needed * crop_w * 3 and p.row_bytes == crop_w * 3, case
    assert p.vvec in (16, 4, 1) and p.row_bytes % p.vvec == 0 and p.vgrid_z == n, case
    if p.vvec == 16:
        assert p.vgrid_x * 256 * 16 >= p.row_bytes * crop_h and p.vgrid_y == 1, case
    else:
        assert p.vgrid_x * 256 * p.vvec >= p.row_bytes and p.vgrid_y == crop_h, case
    assert max(p.hgrid_y, p.hgrid_z, p.vgrid_y, p.vgrid_z) <= 65535, case


def test_every_plan_keeps_the_kernels_preconditions(lib):
    """The issue's grid as a product: per (w, out_w) every filter x crop x n x switch.  h and out_h walk a handful of values with
    the pair; the base alignments with the widths."""
    widths = sorted(set(range(1, 12)) | {13, 16, 20, 31, 53, 64, 720, 2160, 97, 160, 224, 405, 640, 1000, 1280, 1920, 2731, 3840, 4096, 5461, 6000})
    out_widths = (1, 2, 3, 4, 5, 7, 9, 16, 31, 33, 64, 100, 201, 224, 398, 640, 1024)
    switches = ((0, 0, 0), (1, 0, 0), (0, 32, 0), (0, 64, 0), (0, 0, 1), (0, 0, 3))
    plans = refused = 0
    for (iw, w), (io, ow) in itertools.product(enumerate(widths), enumerate(out_widths)):
        h, oh = (1, 5, 37, 1080)[(iw + io) % 4], (1, 9, 224)[(iw + 2 * io) % 3]
        top, ch = oh // 3, max(1, oh // 2)
        ta, da = (8 if w % 3 == 0 else 0), (4 if ow % 5 == 0 else 1 if ow % 7 == 0 else 0)
        crops = {(0, ow), (ow // 4, max(1, ow // 2)), (ow - 1, 1)}       # whole, a window, the last column alone
        if ow > 9:
            crops |= {(1, ow - 3), (3, (ow - 3) // 4 * 4)}              # crop_left > 0 with crop_w % 4 != 0, and with crop_w % 4 == 0
        for filt, (left, cw), n, (seg, kb, spw) in itertools.product((BILINEAR, BICUBIC), sorted(crops), (1, 3, 64, 65535), switches):
            case = (h, w, filt, oh, ow, (top, left, ch, cw), n, ta, da, seg, kb, spw)
            p = plan(lib, *case)
            if isinstance(p, str):       # a column no LDS image holds is refused, as the resize refuses it
                assert "bytes of LDS per workgroup" in p and f"a {w} -> {ow} pixel row" in p, (case, p)
                refused += 1
                continue
            check_invariants(p, case, (h, w, filt, oh, ow), (top, left, ch, cw), n, (seg, kb, spw) == (0, 0, 0))
            plans += 1
    assert plans + refused >= 100_000 and 0 < refused < plans // 10, (plans, refused)


def test_parity_cases_reach_every_launch_form(lib):
    """The GPU parity cases (the ragged list with its windows, and the golden cases) between them launch the row-block-major
    kernel with both stores and with one and several segments per workgroup, the segment-major kernel, and all three widths
    of the vertical pass.  The segment-major kernel with a dword store is out of reach of any geometry: without $VQ_AMD_RSH=seg it
    runs with one column per segment (asserted over the sweep above); the pinned table covers it through the switch, and no GPU
    test runs resample_h_kernel<true>, before this layer or after.  The golden cases run one frame per call, as planned here."""
    from conftest import RESAMPLE_CASES
    reached = set()
    n, h, w, ow, oh = MANY_FRAMES_CASE
    for filt in (BILINEAR, BICUBIC):
        p = plan(lib, h, w, filt, oh, ow, None, n)
        assert p.hx and p.spw == 2 and p.hgrid_x == 16, (filt, p.spw)
        check_invariants(p, MANY_FRAMES_CASE, (h, w, filt, oh, ow), (0, 0, oh, ow), n, True)
        reached.add(("hx", "dword" if p.dword_store else "byte", "spw>1", p.vvec))
    for (h, w, ow, oh) in RAGGED_CASES:
        for filt in (BILINEAR, BICUBIC):
            for crop in (None, ragged_window(ow, oh)):
                p = plan(lib, h, w, filt, oh, ow, crop, ragged_frames(h, w))
                assert not isinstance(p, str), p
                check_invariants(p, (h, w, ow, oh, filt, crop), (h, w, filt, oh, ow), crop or (0, 0, oh, ow), ragged_frames(h, w), True)
                reached.add(("hx" if p.hx else "seg", "dword" if p.dword_store else "byte", "spw>1" if p.spw > 1 else "spw=1", p.vvec))
    for (_, h, w, _, mode) in RESAMPLE_CASES:
        if mode == "stretch":
            p = plan(lib, h, w, BILINEAR, 224, 224)
        else:
            rh, rw, top, left = (ctypes.c_int() for _ in range(4))
            assert lib.vq_clip_processor_geometry(h, w, 224, 224, *(ctypes.byref(v) for v in (rh, rw, top, left))) == 0
            p = plan(lib, h, w, BICUBIC, rh.value, rw.value, (top.value, left.value, 224, 224))
        assert not isinstance(p, str), p
        reached.add(("hx" if p.hx else "seg", "dword" if p.dword_store else "byte", "spw>1" if p.spw > 1 else "spw=1", p.vvec))
    forms = {(k, s) for (k, s, _, _) in reached}
    assert forms == {("hx", "dword"), ("hx", "byte"), ("seg", "byte")}, forms
    assert {m for (k, _, m, _) in reached if k == "hx"} == {"spw>1", "spw=1"}, reached
    assert {v for (_, _, _, v) in reached} == {16, 4, 1}, reached


def test_misuse(lib):
    for args in ((0, 4, 2, 4, 4), (4, 4, 1, 4, 4), (4, 4, 100, 4, 4), (4, 4, 2, 0, 4)):
        assert "vq_debug_resample_plan" in plan(lib, *args)
    assert "does not fit" in plan(lib, 4, 4, 2, 4, 4, (2, 0, 3, 4))
    assert "vq_debug_resample_plan" in plan(lib, 4, 4, 2, 4, 4, n=0)
    out = (ctypes.c_int64 * 9)()
    assert lib.vq_debug_preproc_small_plans(0, 1, 1, 1, 1, 1, 1, 1, out) == -1


def small(lib, n=1, frame_bytes=1, slice_budget=1, m=1, tiles=1, scratch_budget=1, post_m=1, post_bands=1):
    out = (ctypes.c_int64 * 9)()
    assert lib.vq_debug_preproc_small_plans(n, frame_bytes, slice_budget, m, tiles, scratch_budget, post_m, post_bands, out) == 0
    return list(out)


def test_small_plans(lib):
    MiB = 1 << 20
    # frames per slice: (n, frame_bytes, budget).  The budgets tests/test_frame_postprocess.py::test_host_slices and
    # tests/test_scene_scores.py::test_host_slices set, then the 512 MiB default
    for (n, fb, budget), want in {(10, 5883, 23632): 4, (10, 5883, 1): 1, (7, 5883, 17749): 3, (5, 12288, 36864): 3,
                                  (64, 6220800, 512 * MiB): 64, (100, 6220800, 512 * MiB): 86, (3, 1 << 31, 512 * MiB): 1,
                                  (65535, 3, 512 * MiB): 65535}.items():
        assert small(lib, n=n, frame_bytes=fb, slice_budget=budget)[0] == want, (n, fb, budget)
    # the scene batch: (m, tiles, budget) -> (batch, hist_bytes, ssd_bytes).  Budget 1 is tests/test_scene_scores.py::test_scratch_batches
    for (m, tiles, budget), want in {(20, 1, 1): (8, 9216, 32), (20, 3, 1): (8, 27648, 96), (7, 1, 1): (7, 8192, 28),
                                     (64, 254, 256 * MiB): (64, 16906240, 65024), (5000, 254, 256 * MiB): (1032, 268679168, 1048512),
                                     (65535, 2048, 256 * MiB): (128, 270532608, 1048576), (9, 1, 8192): (8, 9216, 32),
                                     (17, 1, 16389): (16, 17408, 64)}.items():
        assert tuple(small(lib, m=m, tiles=tiles, scratch_budget=budget)[1:4]) == want, (m, tiles, budget)
    # PostLayout: (frames, bands) -> offsets of partials, res, prefix, keep, and the total
    for (m, nb), want in {(1, 1): (0, 24, 56, 64, 72), (3, 7): (0, 504, 584, 600, 608), (10, 1): (0, 240, 488, 528, 544),
                          (64, 7): (0, 10752, 12296, 12552, 12616), (65535, 32): (0, 50330880, 51903728, 52165872, 52231408),
                          (4, 2): (0, 192, 296, 312, 320)}.items():
        assert tuple(small(lib, post_m=m, post_bands=nb)[4:]) == want, (m, nb)
