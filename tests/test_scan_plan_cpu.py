"""CPU (`-m "not gpu"`): what the fp16 search (csrc/scan_plan.h) launches, as a value.

vq_debug_scan_plan returns plan_scan's answer for this build and this process's environment without touching a device.
The table pins the choices today's shapes get (read off search_fp16 before it was split into plan and launch, and compared
with a verbatim copy of that arithmetic over twenty million shape / switch combinations at the time); the grid checks that
every plan pads, chunks and covers its work consistently.

The five switches are read from the environment, so the table asserts that none of them is set."""
import ctypes
import os

import pytest

TILE128, PHASE4, STREAM, DEEP, FOLD = 1, 2, 3, 4, 5
BATCH8, LARGE4, XLARGE4, LARGE1, XLARGE1, SMALL32, SMALL64 = range(7)
SWITCHES = ("VQ_AMD_SCAN", "VQ_AMD_SCAN_SMALL", "VQ_AMD_SCAN_RB", "VQ_AMD_RESCORE_QPW4", "VQ_AMD_RESCORE_SMALL64")
DEFAULT_ENV = not any(os.environ.get(k) for k in SWITCHES)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    return _lib.load()


def plan(lib, dim, n, nq, k, force=0):
    """The vq_scan_plan, or the error text."""
    from video_quierer_amd._lib import ScanPlanC
    out = ScanPlanC()
    rc = lib.vq_debug_scan_plan(dim, n, nq, k, force, ctypes.byref(out))
    if rc != 0:
        assert rc == -1          # VQ_ERR_INVALID
        return lib.vq_last_error().decode()
    return out


def is_product(lib):
    return not hasattr(lib, "vq_debug_gemm_bench")       # a `make DIAG=1` / EXPERIMENTS=1 / STAMPS=1 library carries it


def test_plans_of_todays_shapes(lib):
    assert DEFAULT_ENV, f"the table holds for the default switches: unset {SWITCHES}"
    # the headline batch: 10k queries over 1M x 512
    p = plan(lib, 512, 1_000_000, 10_000, 10)
    assert (p.scan, p.qt, p.range, p.n_pad, p.streams, p.q_chunk, p.chunks) == (FOLD, 256, 2048, 1_001_472, 7_824, 10_240, 1)
    assert (p.ranges, p.q_tiles, p.rb, p.scan_grid_x, p.scan_grid_y) == (489, 40, 2, 123 * 5 * 32, 1)
    assert (p.rescore, p.layout, p.rescore_grid, p.rescore_files_flags, p.scan_lds) == (BATCH8, 2, 1_250, 0, 160 << 10)
    # the reference caller's one query
    p = plan(lib, 512, 20_001, 1, 10)
    assert (p.scan, p.nqg, p.fused_q, p.streams, p.scan_grid_x, p.scan_grid_y) == (STREAM, 1, 1, 157, 40, 1)
    assert (p.rescore, p.layout, p.rescore_grid, p.rescore_files_flags) == (SMALL32, 3, 1, 1)
    assert p.rescore_lds == (32 * (512 + 4) + 512) * 4
    # two groups of 16 queries per pass; k in (20, 40]: the 64-candidate one-query kernel, its flags collected for 40 queries
    p = plan(lib, 512, 20_001, 40, 21)
    assert (p.scan, p.nqg, p.fused_q, p.q_pad, p.q_tiles) == (STREAM, 2, 0, 64, 2)
    assert (p.rescore, p.rescore_grid, p.rescore_files_flags) == (SMALL64, 40, 0)
    assert p.rescore_lds == (64 * (512 + 4) + 512) * 4
    assert plan(lib, 768, 16_500, 20, 10).nqg == 1                       # 768-d: registers for one group only
    assert plan(lib, 768, 16_500, 20, 21).rescore == LARGE1              # ... and no 64-candidate kernel
    # dim % 128 != 0: the 128 x 1024 tile and key layout 1
    p = plan(lib, 192, 16_500, 130, 10)
    assert (p.scan, p.qt, p.range, p.n_pad, p.streams, p.scan_grid_x, p.scan_lds) == (TILE128, 128, 1024, 17_408, 136, 34, 0)
    assert (p.rescore, p.layout, p.rescore_grid) == (BATCH8, 1, 17)
    assert plan(lib, 128, 16_400, 3, 5).scan == FOLD                     # dims other than 256, 512 and 768 never stream
    assert plan(lib, 512, 20_001, 97, 10).scan == FOLD                   # nor do more than 96 queries
    # re-score kinds
    for k, kind in ((20, SMALL32), (21, SMALL64), (40, SMALL64), (41, LARGE1), (64, LARGE1), (65, XLARGE1), (100, XLARGE1)):
        assert plan(lib, 512, 20_001, 1, k).rescore == kind, k
    for k, kind, grid in ((20, BATCH8, 17), (21, LARGE4, 33), (32, LARGE4, 33), (64, LARGE4, 33), (65, XLARGE4, 33), (100, XLARGE4, 33)):
        p = plan(lib, 512, 20_001, 130, k)
        assert (p.rescore, p.rescore_grid, p.layout) == (kind, grid, 2), k
    # the key budget chunks the queries
    p = plan(lib, 768, 8_000_000, 100_000, 10)
    assert (p.scan, p.q_chunk, p.chunks) == (FOLD, 2_048, 49)


def test_kinds_a_product_build_does_not_carry(lib):
    for args in ((0, 1, 1, 1), (512, 0, 1, 1), (512, 1, 0, 1), (512, 1, 1, 101), (100, 1, 1, 1)):
        assert "vq_debug_scan_plan" in plan(lib, *args)
    assert plan(lib, 512, 20_001, 130, 10, force=1).scan == TILE128
    assert plan(lib, 512, 20_001, 130, 10, force=7).scan == FOLD         # an unknown value is the default
    if not is_product(lib):
        return              # the diagnostic libraries carry 51-53, the EXPERIMENTS=1 one 2 and 4 too
    for dim, n, nq in ((512, 1_000_000, 10_000), (512, 20_001, 1), (192, 16_500, 130)):
        for force in (PHASE4, DEEP):
            got = plan(lib, dim, n, nq, 10, force)
            assert "EXPERIMENTS=1" in got and f"VQ_AMD_SCAN={force} " in got
        for force in (51, 52, 53):
            got = plan(lib, dim, n, nq, 10, force)
            assert "DIAG=1" in got and f"VQ_AMD_SCAN={force} " in got


def test_every_plan_pads_chunks_and_covers(lib):
    assert DEFAULT_ENV, f"the grid's expectations hold for the default switches: unset {SWITCHES}"
    ns = (1, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 16_383, 16_384, 16_500, 20_001, 1_001_471, 1_001_472, 1_001_473, 3_000_000)
    nqs = (1, 4, 5, 16, 17, 32, 33, 96, 97, 128, 130, 257, 10_000, 200_000)
    for dim in (64, 128, 192, 256, 512, 768, 1024):
        for n in ns:
            for nq in nqs:
                for k in (1, 20, 21, 40, 41, 64, 65, 100):
                    p = plan(lib, dim, n, nq, k)
                    case = (dim, n, nq, k)
                    assert not isinstance(p, str), (case, p)
                    stream = nq <= 96 and dim in (256, 512, 768)
                    assert p.scan == (STREAM if stream else TILE128 if dim % 128 else FOLD), case
                    assert p.n_pad >= n and p.n_pad - n < p.range and p.streams * 128 == p.n_pad and p.ranges * p.range == p.n_pad, case
                    # the chunks cover nq exactly once: `chunks` of q_chunk queries, the last one short but not empty
                    assert p.q_chunk % p.qt == 0 and p.q_chunk >= p.qt, case
                    assert (p.chunks - 1) * p.q_chunk < nq <= p.chunks * p.q_chunk, case
                    assert p.streams * p.q_chunk <= 1 << 27 or p.q_chunk == p.qt, case
                    cur = min(p.q_chunk, nq)
                    assert p.q_pad == -(-cur // p.qt) * p.qt and p.q_tiles * p.qt == p.q_pad, case
                    # the grid holds a workgroup for every (range, query tile); the streaming scan's take four 128-row ranges each
                    assert p.scan_grid_x * p.scan_grid_y * (4 if p.scan == STREAM else 1) >= p.ranges * p.q_tiles, case
                    assert p.rescore_grid * p.rescore_qpw >= cur > (p.rescore_grid - 1) * p.rescore_qpw, case
                    assert p.layout == {STREAM: 3, TILE128: 1, FOLD: 2}[p.scan], case
                    assert p.fused_q == (stream and nq <= 4) and p.nqg == (2 if stream and nq > 16 and dim <= 512 else 1), case
                    one_wg = p.rescore in (SMALL32, SMALL64)
                    assert p.rescore_files_flags == (nq == 1 and p.scan == STREAM and one_wg), case
                    assert (p.rescore_lds > 0) == one_wg and (not one_wg or p.scan == STREAM), case
                    assert p.rescore in ((BATCH8, SMALL32) if k <= 20 else (LARGE4, LARGE1, SMALL64) if k <= 64 else (XLARGE4, XLARGE1)), case
