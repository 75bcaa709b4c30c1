"""GPU (`-m gpu`): vq_frame_postprocess_u8 / FramePreprocessor.postprocess — resize, quality verdict and compaction of a
batch in one device pass — and OptimizedFrameExtractor on top of it.  Everything is compared with `==`: the resize is
the integer arithmetic of oracle.cv_resize_oracle, the three sums are integers (restated here with Python integers
over oracle.quality_oracle's grey conversion and Laplacian), the verdict is an integer comparison.  Frames are tiny:
the shapes are the smallest at which the kernel's paths differ (copy / 2x / linear, byte / 4-byte / 16-byte rows, one
band / several, a last band of one row, a width the on-chip plan cannot hold)."""
import ctypes

import numpy as np
import pytest
import torch        # before the library binds the GPU: torch brings its own copy of the HIP runtime

from oracle.cv_resize_oracle import resize_linear_u8
from oracle.quality_oracle import bgr_to_gray, is_low_quality, laplacian_f64

pytestmark = pytest.mark.gpu

# source (h, w) -> frame_size (width, height) | None.  The reference resizes unless frame.shape[:2] == frame_size.
RESIZE_CASES = [((37, 53), (32, 24)),        # down-scale, linear
                ((9, 11), (32, 24)),         # up-scale, linear
                ((48, 64), (32, 24)),        # exact 2x: the 2x2 average
                ((24, 32), (24, 32)),        # shape[:2] == frame_size: no resize
                ((24, 32), (32, 24)),        # resized to width 32, height 24: the shape it already has
                ((32, 24), (32, 24)),        # the quirk: 32 rows x 24 columns equals frame_size, so it stays 32 rows x 24 columns
                ((37, 53), None)]


def resized(frames, frame_size):
    out = []
    for f in frames:
        if frame_size is not None and f.shape[:2] != tuple(frame_size):
            f = resize_linear_u8(f, frame_size[0], frame_size[1])
        out.append(f)
    return np.stack(out)


def int_sums(f):
    """(sum of bytes, sum L, sum L^2) of one frame as Python integers."""
    lap = laplacian_f64(bgr_to_gray(f))
    li = lap.astype(np.int64)
    assert np.array_equal(li, lap)
    return int(f.astype(np.int64).sum()), int(li.sum()), int((li * li).sum())


def int_verdict(f):
    """True = kept.  The integer form of _is_low_quality, checked against the float oracle."""
    sb, s1, s2 = int_sums(f)
    n = f.shape[0] * f.shape[1]
    low = sb < 20 * 3 * n or sb > 235 * 3 * n or n * s2 - s1 * s1 < 100 * n * n
    assert low == is_low_quality(f)
    return not low


def restate(frames, frame_size, quality_filter=True):
    """→ (kept frames, keep bool[n], sums int64[n, 3]) by the oracles."""
    out = resized(frames, frame_size)
    keep = np.array([(not quality_filter) or int_verdict(f) for f in out], bool)
    sums = np.array([int_sums(f) for f in out], np.int64).reshape(len(out), 3)
    return out[keep], keep, sums


def same(got, want):
    for g, w, name in zip(got, want, ("frames", "keep", "sums")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:4])


@pytest.fixture(scope="module")
def pre(gpu_lib):
    from video_quierer_amd.preprocess import FramePreprocessor
    p = FramePreprocessor()
    yield p
    p.close()


@pytest.fixture(scope="module")
def peek(gpu_lib):
    """peek(ptr, n, h, w): n device-resident frames as a host array, read through a second handle (a result left on the
    device is valid until the next call on the handle that made it)."""
    from video_quierer_amd.preprocess import FramePreprocessor
    p = FramePreprocessor()
    yield lambda ptr, n, h, w: p.postprocess_device(ptr, n, h, w, None, quality_filter=False, keep_on_device=False)[0]
    p.close()


def noise(seed, n, h, w):
    return np.random.default_rng([20261019, seed, n, h, w]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def mixed(seed, n, h, w):
    """Noise frames (kept) among low-contrast (f // 32 + 100) and nearly black ones (dropped), at least one of each."""
    frames = noise(seed, n, h, w)
    for i in range(1, n, 3):
        frames[i] = frames[i] // 32 + 100
    for i in range(2, n, 5):
        frames[i] = frames[i] // 32
    return frames


@pytest.mark.parametrize("shape,frame_size", RESIZE_CASES)
def test_resize_paths_with_statistics(pre, shape, frame_size):
    frames = mixed(1, 7, *shape)
    want = restate(frames, frame_size)
    assert 0 < want[1].sum() < 7
    got = pre.postprocess(frames, frame_size)
    same(got, want)
    if (shape, frame_size) == ((24, 32), (32, 24)):
        assert got[0].shape[1:] == (24, 32, 3)                 # cv2.resize(frame, (32, 24)): width 32, height 24
    if (shape, frame_size) == ((32, 24), (32, 24)):
        assert got[0].shape[1:] == (32, 24, 3) and np.array_equal(got[0], frames[want[1]])
    assert np.array_equal(~got[1], np.array([is_low_quality(f) for f in resized(frames, frame_size)]))
    # A random frame is kept and its low-contrast form f // 32 + 100 is dropped, at this resize.  f // 16 + 100 has a
    # Laplacian variance of 190-230 as it stands (20 x the grey variance of 16 equally likely levels, about 9.5) and falls
    # under 100 only where a resize averages it (89.9, 4.6 and 51.5 at the first three cases): the oracle decides.
    rnd = noise(2, 3, *shape)
    rnd[1] = rnd[1] // 32 + 100
    rnd[2] = rnd[2] // 16 + 100
    soft_kept = not is_low_quality(resized(rnd[2:], frame_size)[0])
    assert soft_kept == (frame_size is None or shape == tuple(frame_size) or shape == tuple(frame_size)[::-1])
    assert pre.postprocess(rnd, frame_size)[1].tolist() == [True, False, soft_kept]
    # quality_filter=False keeps everything and still reports the sums
    same(pre.postprocess(frames, frame_size, quality_filter=False), restate(frames, frame_size, quality_filter=False))
    # the bytes are today's cv_resize
    if frame_size is not None:
        assert np.array_equal(pre.postprocess(frames, frame_size, quality_filter=False, always_resize=True)[0],
                              pre.cv_resize(frames, frame_size))


@pytest.mark.parametrize("out_w", [1, 2, 7, 16, 32, 1024])
def test_band_edges(pre, out_w):
    """Heights around the plan's band: one row (reflect of n == 1), two rows (a halo that is the same row twice), a last
    band of one row.  Widths: rows of 3, 6 and 21 bytes (byte stores), 48 and 96 bytes (16-byte loads and stores)."""
    from video_quierer_amd.preprocess import postprocess_plan
    rows, _, fused = postprocess_plan(1, out_w)
    assert fused and (rows == 32 or out_w == 1024)
    for out_h in sorted({1, 2, rows - 1, rows, rows + 1, 2 * rows + 1}):
        assert postprocess_plan(out_h, out_w)[:2] == (rows, -(-out_h // rows))
        frames = noise(3, 3, out_h, out_w)
        frames[1] = frames[1] // 32 + 100
        same(pre.postprocess(frames, None), restate(frames, None))                        # copy
        if out_w <= 32:
            src = noise(4, 3, out_h + 3, out_w + 5)                                        # linear, into the same output size
            same(pre.postprocess(src, (out_w, out_h)), restate(src, (out_w, out_h)))
            src = noise(5, 2, 2 * out_h, 2 * out_w)                                        # exact 2x
            same(pre.postprocess(src, (out_w, out_h)), restate(src, (out_w, out_h)))


def test_width_beyond_the_plan_runs_unfused(pre):
    from video_quierer_amd.preprocess import postprocess_plan
    out_w = 6000
    assert postprocess_plan(2, out_w) == (2, 1, False) and postprocess_plan(2, 4096)[2]
    frames = mixed(6, 4, 2, out_w)
    same(pre.postprocess(frames, None), restate(frames, None))
    same(pre.postprocess(frames[:, :1], None), restate(frames[:, :1], None))
    src = mixed(7, 4, 3, 5000)
    same(pre.postprocess(src, (out_w, 2)), restate(src, (out_w, 2)))


def stripes(a, b, h=24, w=32):
    """Columns alternating between two grey values, the three channels equal (so grey == the value)."""
    f = np.empty((h, w, 3), np.uint8)
    f[:, 0::2] = a
    f[:, 1::2] = b
    return f


def test_thresholds(pre):
    """Frames that sit exactly on a threshold are kept; one step beyond it they are dropped."""
    var_100, var_64 = stripes(100, 105), stripes(100, 104)
    mean_20, mean_235 = stripes(0, 40), stripes(215, 255)
    below, above, blunted = mean_20.copy(), mean_235.copy(), var_100.copy()
    below[5, 7, 1] = 39            # a pixel of the 40-columns
    above[5, 6, 1] = 216           # a pixel of the 215-columns
    blunted[5, 7] = 104            # one 105-pixel: variance 99.92
    frames = np.stack([var_100, var_64, mean_20, below, mean_235, above, blunted])
    from oracle.quality_oracle import quality
    assert quality(var_100) == (102.5, 100.0) and quality(var_64)[1] == 64.0
    assert quality(mean_20)[0] == 20.0 and quality(mean_235)[0] == 235.0
    assert quality(below)[0] < 20.0 < quality(below)[1] and quality(above)[0] > 235.0
    assert 99.9 < quality(blunted)[1] < 100.0
    want = restate(frames, None)
    assert want[1].tolist() == [True, False, True, False, True, False, False]
    same(pre.postprocess(frames, None), want)
    same(pre.postprocess(frames, (24, 32)), want)                                          # equal to frame_size: not resized
    assert np.array_equal(~want[1], pre.is_low_quality(frames))                              # the float verdict of the same handle


@pytest.fixture(scope="module")
def tiny_pool():
    """1,025 noise frames of 4 x 4 that the oracle keeps, and a flat one that it drops."""
    cand = noise(8, 1400, 4, 4)
    good = cand[np.array([int_verdict(f) for f in cand])][:1025]
    assert len(good) == 1025
    flat = np.full((4, 4, 3), 90, np.uint8)
    assert not int_verdict(flat)
    return good, flat


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025])
def test_compaction(pre, tiny_pool, n):
    good, flat = tiny_pool
    patterns = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0,
                "first": np.arange(n) == 0, "last": np.arange(n) == n - 1}
    for name, kept in patterns.items():
        frames = np.where(kept[:, None, None, None], good[:n], flat[None])
        out, keep, sums = pre.postprocess(frames, None)
        assert np.array_equal(keep, kept), name
        assert out.shape == (int(kept.sum()), 4, 4, 3) and np.array_equal(out, frames[kept]), name
        assert np.array_equal(sums[0], int_sums(frames[0])) and np.array_equal(sums[-1], int_sums(frames[-1]))
        out, keep, _ = pre.postprocess(frames, None, quality_filter=False)
        assert keep.all() and np.array_equal(out, frames), name


def test_host_slices(pre, peek, monkeypatch):
    frames = mixed(9, 10, 37, 53)
    frames[9] //= 32                                                                         # a drop in the last slice too
    want = restate(frames, (32, 24))
    assert [int(want[1][a:b].sum()) for a, b in ((0, 4), (4, 8), (8, 10))] == [2, 2, 1]      # drops and survivors in each slice
    one = pre.postprocess(frames, (32, 24))
    same(one, want)
    monkeypatch.setenv("VQ_AMD_POSTPROC_SLICE_BYTES", str(4 * 37 * 53 * 3 + 100))           # slices 4 + 4 + 2
    same(pre.postprocess(frames, (32, 24)), one)
    same(pre.postprocess_list(list(frames), (32, 24)), one)
    same(pre.postprocess(frames, (32, 24), quality_filter=False), restate(frames, (32, 24), quality_filter=False))
    monkeypatch.setenv("VQ_AMD_POSTPROC_SLICE_BYTES", "1")                                    # smaller than a frame: one per slice
    same(pre.postprocess(frames, (32, 24)), one)
    ptr, keep, _ = pre.postprocess(frames, (32, 24), keep_on_device=True)                     # sliced, result left on the device
    assert np.array_equal(peek(ptr, int(keep.sum()), 24, 32), one[0])


def test_forms(pre, peek):
    frames = mixed(10, 9, 37, 53)
    want = restate(frames, (32, 24))
    same(pre.postprocess(frames, (32, 24)), want)
    same(pre.postprocess_list([f.copy() for f in frames], (32, 24)), want)                    # separately allocated
    same(pre.postprocess_list(list(frames), (32, 24)), want)                                  # contiguous: one upload
    assert [a.shape for a in pre.postprocess_list([])] == [(0, 0, 0, 3), (0,), (0, 3)]
    out, keep, sums = pre.postprocess(frames[:0], (32, 24))
    assert out.shape == (0, 24, 32, 3) and keep.shape == (0,) and sums.shape == (0, 3)
    n, h, w = frames.shape[:3]
    for size, data in (((32, 24), frames), (None, noise(11, 5, 16, 16))):                    # linear from bytes; copy with 16-byte rows
        n, h, w = data.shape[:3]
        want = restate(data, size)
        d = torch.from_numpy(data).cuda()
        flat = torch.empty(data.size + 1, dtype=torch.uint8, device="cuda")
        off = flat[1:]
        off.copy_(d.reshape(-1))
        torch.cuda.synchronize()
        assert off.data_ptr() % 16 == 1
        for p in (d.data_ptr(), off.data_ptr()):                                              # aligned, and one byte off
            same(pre.postprocess_device(p, n, h, w, size, keep_on_device=False), want)
            ptr, keep, sums = pre.postprocess_device(p, n, h, w, size)
            assert np.array_equal(keep, want[1]) and np.array_equal(sums, want[2])
            assert np.array_equal(peek(ptr, len(want[0]), *want[0].shape[1:3]), want[0])


def test_device_result_into_the_encoder(pre, b32_weights):
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    frames = mixed(12, 5, 250, 300)
    want = restate(frames, (224, 224))
    kept = int(want[1].sum())
    assert 0 < kept < 5
    enc = VitEncoder(VIT_B_32, b32_weights, max_batch=8)
    try:
        ptr, keep, _ = pre.postprocess(frames, (224, 224), keep_on_device=True)
        assert np.array_equal(keep, want[1])
        out = torch.empty((kept, 512), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        enc.encode_device(ptr, kept, out.data_ptr(), swap_rb=True)
        enc.synchronize()
        assert np.array_equal(out.cpu().numpy(), enc.encode(want[0], swap_rb=True))
    finally:
        enc.close()


def test_calls_on_one_handle_are_independent(pre, peek):
    frames = mixed(13, 6, 90, 160)
    q0, s0, c0 = pre.quality(frames), pre.stretch(frames), pre.scene_change_scores(frames)
    want = restate(frames, (32, 24))
    for _ in range(2):
        same(pre.postprocess(frames, (32, 24)), want)
        q, c = pre.quality(frames), pre.scene_change_scores(frames)
        assert all(np.array_equal(a, b) for a, b in zip(q + c, q0 + c0))
        same(pre.postprocess(frames, None), restate(frames, None))
        assert np.array_equal(pre.stretch(frames), s0)
        ptr = pre.stretch(frames, keep_on_device=True)                                        # the device output follows the last call
        assert np.array_equal(peek(ptr, len(s0), 224, 224), s0)


def test_misuse(pre, gpu_lib):
    with pytest.raises(ValueError, match="too large"):
        pre.postprocess(np.zeros((1, 2, 2, 3), np.uint8), (2048, 1025))                       # 2^21 + 2048 output pixels
    with pytest.raises(ValueError, match="too large"):
        pre.postprocess(np.zeros((1, 1025, 2048, 3), np.uint8), None)
    with pytest.raises(ValueError, match="65535"):
        pre.postprocess(np.zeros((65536, 1, 1, 3), np.uint8), None)
    with pytest.raises(ValueError):
        pre.postprocess(np.zeros((1, 2, 2, 3), np.uint8), (-4, 4))
    with pytest.raises(ValueError):
        pre.postprocess(np.zeros((2, 4, 4, 4), np.uint8))
    with pytest.raises(TypeError):
        pre.postprocess(np.zeros((2, 4, 4, 3), np.float32))
    lib = gpu_lib.load()
    buf, keep, kept = np.zeros(48, np.uint8), np.full(4, 9, np.uint8), ctypes.c_int64(-5)
    vp = ctypes.c_void_p

    def rc(frames, n, h, w, out_h, out_w, keep_p=keep.ctypes.data_as(vp), kept_p=ctypes.byref(kept)):
        return lib.vq_frame_postprocess_u8(pre._h, frames, n, h, w, 0, out_h, out_w, 1, None, kept_p, keep_p, None)

    fp = buf.ctypes.data_as(vp)
    assert rc(fp, 1, 4, 4, -1, 4) == -1 and rc(fp, 1, 4, 4, 0, 4) == -1 and rc(fp, 1, 0, 4, 0, 0) == -1
    assert rc(fp, -1, 4, 4, 0, 0) == -1 and rc(None, 1, 4, 4, 0, 0) == -1 and rc(fp, 1, 4, 4, 0, 0, keep_p=None) == -1
    assert rc(fp, 1, 4, 4, 0, 0, kept_p=None) == -1 and "vq_frame_postprocess_u8" in lib.vq_last_error().decode()
    assert keep.tolist() == [9] * 4 and kept.value == -5                                     # nothing was written
    assert rc(None, 0, 4, 4, 0, 0, keep_p=None) == 0 and kept.value == 0                     # n == 0: a no-op


def test_extractor_end_to_end():
    """OptimizedFrameExtractor with its default scorer and preprocessor (both on the GPU) gives the adaptive sampler's
    records filtered and resized by the oracles."""
    from video_quierer_amd.core.frame_extractor import AdaptiveFrameSampler, OptimizedFrameExtractor
    frames = mixed(14, 70, 37, 53)
    fps = 4.0                                                   # at least int(0.5 * 4) = 2 frames between taken frames
    ex = OptimizedFrameExtractor(strategy="adaptive", frame_size=(32, 24))
    recs = ex.extract_frames("clip.mp4", reader=lambda path: (fps, iter([frames[:33], frames[33:34], frames[34:]])))
    sampled = AdaptiveFrameSampler().sample(frames, fps, "clip.mp4")
    assert len(sampled) >= 20
    want = [dict(r, frame=resize_linear_u8(r["frame"], 32, 24)) for r in sampled]
    want = [r for r in want if not is_low_quality(r["frame"])]
    assert 0 < len(want) < len(sampled)
    assert [r["frame_number"] for r in recs] == [r["frame_number"] for r in want]
    for g, w in zip(recs, want):
        assert set(g) == set(w) | {"processing_time"}
        assert np.array_equal(g["frame"], w["frame"]) and g["frame"].shape == (24, 32, 3)
        assert (g["timestamp"], g["scene_change_score"], g["video_path"]) == (w["timestamp"], w["scene_change_score"], "clip.mp4")
    times = [r["processing_time"] for r in recs]
    assert times == sorted(times)
    same_again = ex.process_records(sampled)
    assert [r["frame_number"] for r in same_again] == [r["frame_number"] for r in want]
    ex.preprocessor.close()
