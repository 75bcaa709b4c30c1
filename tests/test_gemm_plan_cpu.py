"""CPU (`-m "not gpu"`): what the GEMM dispatch (csrc/gemm_dispatch.h) chooses, as a value.

vq_debug_gemm_plan returns plan_gemm's answer for this build and this process's environment without touching a
device.  The table pins the choices the encoder's shapes get today (read off the dispatcher before it was split into
plan and launch, and compared with it over two million shape / id / build / switch combinations at the time); the
grid checks that every plan covers its rows exactly once with shapes its kernels accept.

The switches are read once per process, so the two that the table depends on are honoured here: run the module once
with VQ_AMD_GEMM_TAIL=0 and once with VQ_AMD_GEMM160=0 to see the other halves of those decisions."""
import ctypes
import os

import pytest

TILE128, PHASE4, RING160, AUTO_NO160, DEEP, DEEP_GLOBAL_LDS, MULTI_WHERE_WORTH, MULTI, ASM256 = 1, 2, 5, 6, 8, 11, 15, 16, 24
EXPERIMENTS = (3, 4, 7, 9, 10, 12, 13, 20, 21)


def _off(name):
    v = os.environ.get(name)
    if v is None:
        return False
    try:
        return int(v) == 0
    except ValueError:          # atoi("junk") == 0
        return True


TAIL = not _off("VQ_AMD_GEMM_TAIL")
USE160 = not _off("VQ_AMD_GEMM160")
DEFAULT_ENV = not any(os.environ.get(k) for k in ("VQ_AMD_GEMM256", "VQ_AMD_GEMM_MULTI", "VQ_AMD_GEMM_MULTI_MIN", "VQ_AMD_GEMM_TPW"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    return _lib.load()


def plan(lib, M, N, K, row_in=0, force=0, lda=None, ldw=None):
    """[(kernel, rows, row0, tiles_per_wg), ...], or the error text."""
    n = ctypes.c_int(0)
    k, r, r0, t = ((ctypes.c_int * 2)() for _ in range(4))
    rc = lib.vq_debug_gemm_plan(M, N, K, K if lda is None else lda, K if ldw is None else ldw, row_in, force,
                                ctypes.byref(n), k, r, r0, t)
    if rc != 0:
        assert rc == -1          # VQ_ERR_INVALID
        return lib.vq_last_error().decode()
    return [(k[i], r[i], r0[i], t[i]) for i in range(n.value)]


def is_product(lib):
    return not hasattr(lib, "vq_debug_gemm_bench")       # a `make DIAG=1` / EXPERIMENTS=1 / STAMPS=1 library carries it


def test_plans_of_the_encoder_shapes(lib):
    assert DEFAULT_ENV, "the table holds for the default switches (VQ_AMD_GEMM_TAIL and VQ_AMD_GEMM160 excepted)"
    one = lambda kernel, M, tpw=1: [(kernel, M, 0, tpw)]
    split = lambda M, main: [(DEEP, main, 0, 1), (TILE128, M - main, main, 1)] if TAIL else one(DEEP, M)
    assert plan(lib, 512, 256, 384) == one(TILE128, 512)
    assert plan(lib, 7680, 2560, 128) == split(7680, 6400)                              # 300 tiles, remainder 44
    assert plan(lib, 12800, 768, 768) == (one(RING160, 12800) if USE160 else one(DEEP, 12800))      # 240 workgroups of 160 rows
    assert plan(lib, 12800, 768, 768, force=AUTO_NO160) == one(DEEP, 12800)             # 150 tiles, no tail split
    assert plan(lib, 12800, 2304, 768, row_in=1) == one(DEEP, 12800)                    # 450 tiles, remainder 194
    assert plan(lib, 12800, 2304, 768, row_in=1, force=AUTO_NO160) == one(MULTI, 12800, 3)
    assert plan(lib, 12800, 3072, 768, row_in=1) == split(12800, 10752)                 # 600 tiles, remainder 88
    assert plan(lib, 12800, 3072, 768, row_in=1, force=AUTO_NO160) == one(MULTI, 12800, 3)
    assert plan(lib, 18688, 3072, 1024, row_in=1, force=AUTO_NO160) == one(MULTI, 18688, 4)         # 73 x 12 tiles
    for N, tpw in ((768, 3), (512, 2), (1024, 4)):
        assert plan(lib, 512, N, 640, force=MULTI) == one(MULTI, 512, tpw)
    for force in (PHASE4, DEEP, DEEP_GLOBAL_LDS):
        assert plan(lib, 512, 256, 384, force=force) == one(force, 512)


def test_plans_the_encoder_stage_cases_rely_on(lib):
    """tests/test_encoder_stages.py (GPU) has cases written for ONE kernel each and asserts these plans itself before it runs;
    pinned here so that a dispatch change fails without a GPU first.  If one of these moves, move the stage case it names to a
    shape that still gets the kernel the case is about (its _multi_cases / _split_multi_cases say how the batch was chosen)."""
    assert DEFAULT_ENV, "the pins hold for the default switches"
    one = lambda kernel, M, tpw=1: [(kernel, M, 0, tpw)]
    W = MULTI_WHERE_WORTH
    for M, why in ((3840, "t50 n=72 gemm15: the smallest batch on gemm_tn256dm"), (4096, "16 tile rows (t50 n=77)")):
        assert plan(lib, M, 2304, 768, row_in=1, force=W) == one(MULTI, M, 3), f"q|k|v, {why}"
        assert plan(lib, M, 3072, 768, row_in=1, force=W) == one(MULTI, M, 3), f"fc1, {why}"
        for K in (768, 3072):
            assert plan(lib, M, 768, K, force=W) == one(TILE128, M), f"out_proj / fc2, {why}"
    assert plan(lib, 3584, 2304, 768, row_in=1, force=W) == one(TILE128, 3584), "t50 n=71 (126 tiles) would do: lower the n=72 cases"
    why = "text512 n=70 gemm15"
    assert plan(lib, 5632, 1536, 512, row_in=1, force=W) == one(MULTI, 5632, 3), f"q|k|v (two workgroups per tile row), {why}"
    assert plan(lib, 5632, 2048, 512, row_in=1, force=W) == one(DEEP, 5632), f"fc1 (tiles_n = 8), {why}"
    assert plan(lib, 5376, 1536, 512, row_in=1, force=W) == one(TILE128, 5376), "text512 n=69 (126 tiles) would do: lower the n=70 cases"
    for K in (512, 2048):
        assert plan(lib, 5632, 512, K, force=W) == one(TILE128, 5632), f"out_proj / fc2, {why}"
    why = "t50 n=220 concurrent: the benchmark's own dispatch"
    assert plan(lib, 11008, 2304, 768, row_in=1, force=AUTO_NO160) == one(MULTI, 11008, 3), f"q|k|v, {why}"
    assert plan(lib, 11008, 3072, 768, row_in=1, force=AUTO_NO160) == one(MULTI, 11008, 3), f"fc1, {why}"
    assert plan(lib, 10752, 2304, 768, row_in=1, force=AUTO_NO160) == one(DEEP, 10752), "42 tile rows would do: lower the n=220 case"
    for K in (768, 3072):
        assert plan(lib, 11008, 768, K, force=AUTO_NO160) == one(DEEP, 11008), f"out_proj / fc2 / patch embedding (K = 3072), {why}"
    why = "t50 n=77 gemm8"
    for N, K, row_in in ((2304, 768, 1), (3072, 768, 1), (768, 768, 0), (768, 3072, 0)):
        assert plan(lib, 4096, N, K, row_in=row_in, force=DEEP) == one(DEEP, 4096), f"{N} x {K}, {why}"
    # the child of test_multi_tile_tiles_per_workgroup_in_a_child ($VQ_AMD_GEMM_TPW there; three per workgroup without it)
    assert plan(lib, 2816, 3072, 1024, row_in=1, force=W) == one(MULTI, 2816, 3)
    assert plan(lib, 2816, 4096, 1024, row_in=1, force=W) == one(DEEP, 2816)
    for K in (1024, 4096):
        assert plan(lib, 2816, 1024, K, force=W) == one(TILE128, 2816)


def test_ids_a_product_build_does_not_carry(lib):
    """Non-row-stat epilogues refuse every experiment id; row-stat epilogues refuse those that have a row-stat form
    (9, 12, 13, 20, 21) and give the others (3, 4, 7, 10) the 256x256 deep kernel or the 128x128 one, as before the
    dispatcher was split: an encoder run with such an id still stops at its first out_proj."""
    if not is_product(lib):
        return              # the diagnostic libraries carry id 24, the EXPERIMENTS=1 one the rest
    for M, N, K in ((512, 256, 384), (12800, 3072, 768), (384, 128, 64)):
        for row_in in (0, 1):
            assert "DIAG=1" in plan(lib, M, N, K, row_in, ASM256)
            for force in EXPERIMENTS:
                got = plan(lib, M, N, K, row_in, force)
                if row_in and force in (3, 4, 7, 10):
                    assert got == [(DEEP if (M, N, K) == (12800, 3072, 768) else TILE128, M, 0, 1)]
                else:
                    assert "EXPERIMENTS=1" in got and f"kernel {force} " in got


def accepts(kernel, rows, N, K, lda, ldw, tpw):
    """The shape checks (VQ_CHECK) of the launcher a step names."""
    if lda % 8 or ldw % 8 or rows <= 0:
        return False
    if kernel == TILE128:
        return rows % 128 == 0 and N % 128 == 0 and K % 64 == 0 and K >= 64
    if kernel == RING160:
        return rows % 160 == 0 and N % 256 == 0 and K % 32 == 0 and K >= 128
    tiles256 = rows % 256 == 0 and N % 256 == 0 and K % 128 == 0
    if kernel in (PHASE4, DEEP, DEEP_GLOBAL_LDS):
        return tiles256 and tpw == 1
    if kernel == MULTI:
        return tiles256 and tpw >= 1 and (N // 256) % tpw == 0 and lda % 64 == 0 and ldw % 64 == 0
    return False


def test_every_plan_covers_its_rows_with_shapes_its_kernels_accept(lib):
    for M in range(128, 20480 + 1, 128):
        for N in (256, 512, 768, 1024, 1280, 2304, 2560, 3072, 4096):
            for K in (128, 384, 640, 768, 1024, 3072, 4096):
                for row_in in (0, 1):
                    for force in (0, AUTO_NO160):
                        steps = plan(lib, M, N, K, row_in, force)
                        case = (M, N, K, row_in, force, steps)
                        assert isinstance(steps, list) and 1 <= len(steps) <= 2, case
                        assert sum(s[1] for s in steps) == M, case
                        row = 0
                        for kernel, rows, row0, tpw in steps:
                            assert row0 == row, case
                            assert accepts(kernel, rows, N, K, K, K, tpw), case
                            row += rows
                        if row_in:
                            assert all(s[0] in (TILE128, DEEP, MULTI) for s in steps), case     # the kernels with a row-stat prologue
