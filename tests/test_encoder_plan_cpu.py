"""CPU (`-m "not gpu"`): what the encoder's host layer (csrc/encoder_plan.h) decides, as values.

vq_debug_encoder_plan returns plan_forward's answer and the buffer layout for a handle that is never made, for this build
and this process's environment, without touching a device.

The pinned tables hold what the encoder launched BEFORE the plan existed (commit f911a98), read off that commit's
run_forward by hand: its closures (pad_rows, use24, gemm_rows, gf, the mutating resid_mode), the attention and patchify
if-chains and the split-K condition were ported line by line into a throw-away script, whose answers are the literals
below; the same script agreed with this library on 420,000 (geometry, max_batch, n, flags, layer limit, switch)
combinations at the time.  The layout literals are that commit's arena_bytes() / add() sums and take<> sequences,
evaluated the same way.

The GEMM dispatch reads its switches once per process, so the one the tables depend on is honoured: run the module once
with VQ_AMD_GEMM160=0 to see the other half of the 160-row decision."""
import ctypes
import types

import pytest

import encoder_stage_ref as R
from test_gemm_plan_cpu import USE160, accepts
from test_gemm_plan_cpu import plan as gemm_plan
from video_quierer_amd.weights import TEXT_B_32, VIT_B_32, VIT_L_14_336, TextConfig, VitConfig

FP16, CONCURRENT = 1, 2                                     # VQ_ENC_FP16, VQ_ENC_CONCURRENT
AUTO, AUTO_NO160, DEEP = 0, 6, 8                            # GemmKernel ids (csrc/gemm_dispatch.h)
PATCHIFY_NONE, PATCHIFY_U8, PATCHIFY_GENERIC = 0, 1, 2
AK_TEXT, AK_TILE50, AK_T64, AK_STREAM, AK_WG32, AK_WG64 = range(6)
IN_SPLIT, OUT_SPLIT, OUT_F32 = 1, 2, 4                      # residual epilogue mode bits (csrc/encoder_kernels.h)
SWITCHES = ("VQ_AMD_GEMM", "VQ_AMD_RESID", "VQ_AMD_ATTN", "VQ_AMD_FULL_LAST_LAYER", "VQ_AMD_DTYPE", "VQ_AMD_GEMM24")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from video_quierer_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:                                   # read at every call, as at every handle's creation
        monkeypatch.delenv(name, raising=False)


def plan(lib, cfg, max_batch, n, flags=FP16, shared=0, run_layers=-1, keep_stream=0):
    """(vq_encoder_plan, [mode of out_proj, mode of fc2] per block that runs on every row)."""
    from video_quierer_amd import _lib
    out = _lib.EncoderPlanC()
    modes = (ctypes.c_int * (2 * cfg.layers))()
    if isinstance(cfg, TextConfig):
        c = _lib.TextConfigC(cfg.vocab, cfg.max_positions, cfg.hidden, cfg.mlp, cfg.layers, cfg.heads, cfg.proj_dim, cfg.eos_token_id, cfg.ln_eps)
        vit, text = None, ctypes.byref(c)
    else:
        c = _lib.VitConfigC(cfg.image_size, cfg.patch_size, cfg.hidden, cfg.mlp, cfg.layers, cfg.heads, cfg.proj_dim, cfg.ln_eps)
        vit, text = ctypes.byref(c), None
    rc = lib.vq_debug_encoder_plan(vit, text, max_batch, n, flags, shared, run_layers, keep_stream, ctypes.byref(out), modes)
    assert rc == 0, lib.vq_last_error().decode()
    m = list(modes)
    assert all(v == -1 for v in m[2 * next((i for i in range(cfg.layers) if m[2 * i] < 0), cfg.layers):])     # -1 only behind the last full-row block
    return out, [v for v in m if v >= 0]


def rows_of(p):
    return (p.rows_gemm, p.rows_out, p.rows_fc2, p.rows_cls)


# ---------------------------------------------------------------- pinned: the row counts a lone handle with max_batch = n gets
ROWS = [    # (config, n, rows_gemm, out_proj, fc2, CLS block) with the 160-row tiles on
    (VIT_B_32, 1, 128, 128, 128, 128), (VIT_B_32, 5, 256, 256, 256, 128), (VIT_B_32, 6, 384, 384, 384, 128),
    (VIT_B_32, 7, 384, 480, 480, 128), (VIT_B_32, 64, 3328, 3200, 3200, 128), (VIT_B_32, 256, 12800, 12800, 12800, 256),
    (VIT_L_14_336, 5, 3072, 3040, 3040, 128), (TEXT_B_32, 5, 512, 480, 480, None),
]


@pytest.mark.parametrize("cfg,n,rows_gemm,rows_out,rows_fc2,rows_cls", ROWS, ids=lambda v: str(v) if isinstance(v, (int, type(None))) else type(v).__name__)
def test_row_counts_of_a_lone_and_of_a_concurrent_handle(lib, cfg, n, rows_gemm, rows_out, rows_fc2, rows_cls):
    is_text = isinstance(cfg, TextConfig)
    tokens = cfg.max_positions if is_text else cfg.tokens
    p, _ = plan(lib, cfg, n, n)
    assert p.rows == n * tokens and p.rows_gemm == rows_gemm
    assert (p.rows_out, p.rows_fc2) == ((rows_out, rows_fc2) if USE160 else (rows_gemm, rows_gemm))
    assert p.cls_only_last == (0 if is_text else 1)
    if rows_cls is not None:
        assert p.rows_cls == rows_cls
    assert (p.k_patch, p.k_qkv, p.k_out, p.k_fc1, p.k_fc2, p.k_cls) == (AUTO,) * 6
    if not is_text:                                         # concurrent handles keep 256- / 128-row tiles everywhere
        q, _ = plan(lib, cfg, n, n, flags=FP16 | CONCURRENT)
        assert (q.rows_gemm, q.rows_out, q.rows_fc2) == (rows_gemm,) * 3 and q.rows_cls == rows_cls
        assert (q.k_patch, q.k_qkv, q.k_out, q.k_fc1, q.k_fc2, q.k_cls) == (AUTO_NO160,) * 6
    else:                                                   # the text tower has no concurrent mode: the flag changes nothing
        q, _ = plan(lib, cfg, n, n, flags=FP16 | CONCURRENT)
        assert rows_of(q)[:3] == rows_of(p)[:3] and q.k_out == AUTO


def _vit(image_size, patch_size, **kw):
    return VitConfig(image_size=image_size, patch_size=patch_size, **kw)


def test_attention_and_patchify_kernels(lib, monkeypatch):
    towers = {37: _vit(192, 32), 50: _vit(224, 32), 65: _vit(112, 14), 197: _vit(224, 16)}
    want = {    # $VQ_AMD_ATTN -> attention kernel per T
        None: {37: AK_T64, 50: AK_TILE50, 65: AK_WG32, 197: AK_WG32},
        "simple": {37: AK_T64, 50: AK_TILE50, 65: AK_STREAM, 197: AK_STREAM},
        "q64": {37: AK_T64, 50: AK_TILE50, 65: AK_WG64, 197: AK_WG64},
        "t64": {37: AK_T64, 50: AK_T64, 65: AK_WG32, 197: AK_WG32},
        "nonsense": {37: AK_T64, 50: AK_TILE50, 65: AK_WG32, 197: AK_WG32},
    }
    for switch, per_t in want.items():
        if switch is not None:
            monkeypatch.setenv("VQ_AMD_ATTN", switch)
        for T, cfg in towers.items():
            assert cfg.tokens == T
            p, _ = plan(lib, cfg, 4, 3)
            assert p.attention == per_t[T], (switch, T)
            assert p.patchify == (PATCHIFY_GENERIC if cfg.patch_size == 14 else PATCHIFY_U8)      # 14: not whole 8-pixel runs, K 588 padded to 640
        p, _ = plan(lib, TEXT_B_32, 4, 3)                   # no attention switch on the text tower
        assert (p.attention, p.patchify, p.prows, p.prows_gemm) == (AK_TEXT, PATCHIFY_NONE, 0, 0)
    p, _ = plan(lib, VIT_L_14_336, 8, 8)
    assert (p.attention, p.patchify, p.prows, p.prows_gemm) == (AK_WG32, PATCHIFY_GENERIC, 8 * 576, 4608)


def test_last_block_split_k_and_the_switches(lib, monkeypatch):
    full = [OUT_SPLIT] + [IN_SPLIT | OUT_SPLIT] * 20 + [IN_SPLIT | OUT_F32]      # 11 full-row blocks, then the CLS-only one
    p, modes = plan(lib, VIT_B_32, 256, 256)
    assert (p.layers_run, p.cls_only_last, p.fc2_splits, p.rows_cls, p.split, p.stream_left_split) == (12, 1, 8, 256, 1, 0)
    assert modes == full
    p, _ = plan(lib, VIT_B_32, 64, 64)
    assert (p.fc2_splits, p.rows_cls) == (8, 128)
    p, _ = plan(lib, VIT_B_32, 7, 7)                        # eight partial planes of 128 rows do not fit the q|k|v buffer of 512 rows
    assert (p.fc2_splits, p.rows_cls) == (0, 128)
    monkeypatch.setenv("VQ_AMD_FULL_LAST_LAYER", "1")       # twelve full-row blocks; the last fc2 writes the fp32 x for the pooling head
    p, modes = plan(lib, VIT_B_32, 256, 256)
    assert (p.layers_run, p.cls_only_last, p.split, p.stream_left_split) == (12, 0, 1, 0)
    assert modes == [OUT_SPLIT] + [IN_SPLIT | OUT_SPLIT] * 22 + [IN_SPLIT | OUT_F32]
    monkeypatch.delenv("VQ_AMD_FULL_LAST_LAYER")
    monkeypatch.setenv("VQ_AMD_RESID", "f32")
    p, modes = plan(lib, VIT_B_32, 256, 256)
    assert (p.split, p.stream_left_split, p.cls_only_last, p.fc2_splits) == (0, 0, 1, 8) and modes == [OUT_F32] * 22
    monkeypatch.delenv("VQ_AMD_RESID")
    p, modes = plan(lib, VIT_B_32, 256, 256, flags=0)       # bf16 operands: xh has 8 bits, no split stream
    assert (p.split, p.stream_left_split) == (0, 0) and modes == [OUT_F32] * 22
    p, modes = plan(lib, VIT_B_32, 256, 256, flags=0x200 | 0x400 | 0x1000)      # fp16 q|k|v, attention and fc2, but a bf16 fc1 operand: xh is bf16 after out_proj
    assert p.split == 0 and modes == [OUT_F32] * 22
    monkeypatch.setenv("VQ_AMD_DTYPE", "bf16")              # the variable wins over the flags
    assert plan(lib, VIT_B_32, 256, 256)[0].split == 0
    monkeypatch.delenv("VQ_AMD_DTYPE")
    monkeypatch.setenv("VQ_AMD_GEMM", str(DEEP))            # the forced 256x256 kernel: every GEMM gets the id, no 160-row tiles, no split-K
    p, modes = plan(lib, VIT_B_32, 256, 256)
    assert (p.k_patch, p.k_qkv, p.k_out, p.k_fc1, p.k_fc2, p.k_cls) == (DEEP,) * 6
    assert (p.rows_gemm, p.rows_out, p.rows_fc2, p.rows_cls, p.fc2_splits) == (12800, 12800, 12800, 256, 0) and modes == full
    p, _ = plan(lib, VIT_B_32, 7, 7)
    assert (p.rows_out, p.rows_fc2) == (384, 384)
    p, _ = plan(lib, VIT_B_32, 7, 7, flags=FP16 | CONCURRENT)                   # the variable wins over the concurrent flag's id
    assert p.k_out == DEEP


@pytest.mark.parametrize("layers", (2, 3))
@pytest.mark.parametrize("tower", ("image", "text"))
def test_residual_modes_follow_the_stream_forms(lib, tower, layers):
    """encoder_stage_ref.split_forms is the form the stream is left in after k blocks; the modes must chain through it."""
    cfg = VitConfig(layers=layers) if tower == "image" else TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, layers=layers)
    forms = R.split_forms(types.SimpleNamespace(is_text=tower == "text", layers=layers))
    full_blocks = layers - 1 if tower == "image" else layers
    for k in range(layers + 1):
        p, modes = plan(lib, cfg, 5, 5, run_layers=k, keep_stream=1)        # the full pass cut short
        assert p.layers_run == k and p.stream_left_split == int(forms[k]), (k, forms)
        assert len(modes) == 2 * min(k, full_blocks)
        held = False                                        # the embedding kernel writes the fp32 x
        for i, m in enumerate(modes):
            assert bool(m & IN_SPLIT) == held, (k, i, modes)
            assert bool(m & OUT_SPLIT) != bool(m & OUT_F32), (k, i, modes)
            held = bool(m & OUT_SPLIT)
            if i % 2:                                       # behind fc2 of block i // 2
                assert held == forms[i // 2 + 1], (k, i, modes)
            else:
                assert held, "out_proj never writes the fp32 x back"
        assert held == forms[k] or k > full_blocks
        p, modes = plan(lib, cfg, 5, 5, run_layers=k, keep_stream=0)        # a plain layer-limited pass keeps the fp32 x and every row
        if k < layers:
            assert (p.split, p.stream_left_split, p.cls_only_last) == (0, 0, 0) and modes == [OUT_F32] * (2 * k)
    p, modes = plan(lib, cfg, 5, 5)                         # the product pass: the same modes as the cut-short pass of every block
    assert modes == plan(lib, cfg, 5, 5, run_layers=layers, keep_stream=1)[1] and p.stream_left_split == 0 and p.split == 1
    assert modes[0] == OUT_SPLIT and modes[-1] == IN_SPLIT | OUT_F32 and all(m == IN_SPLIT | OUT_SPLIT for m in modes[1:-1])
    assert plan(lib, cfg, 5, 5, run_layers=layers + 3)[0].layers_run == layers


# ---------------------------------------------------------------- grid: every row count fits its buffer and its kernel
def _check_gemm(lib, M, N, K, row_in, force, live, pad, what):
    assert live <= M <= pad, what
    steps = gemm_plan(lib, M, N, K, row_in, force)
    assert isinstance(steps, list) and sum(s[1] for s in steps) == M, (what, steps)
    for kernel, rows, row0, tpw in steps:
        assert accepts(kernel, rows, N, K, K, K, tpw), (what, steps)


@pytest.mark.parametrize("cfg", (VIT_B_32, VIT_L_14_336, TEXT_B_32), ids=("vit_b32", "vit_l14_336", "text"))
def test_every_row_count_fits_its_buffer_and_its_kernel(lib, cfg):
    is_text = isinstance(cfg, TextConfig)
    H, mlp = cfg.hidden, cfg.mlp
    for max_batch in (1, 7, 64, 256):
        for flags in (FP16,) if is_text else (FP16, FP16 | CONCURRENT):
            for n in range(1, max_batch + 1):
                p, _ = plan(lib, cfg, max_batch, n, flags=flags)
                what = (max_batch, n, flags)
                assert p.rows == n * (cfg.max_positions if is_text else cfg.tokens)
                _check_gemm(lib, p.rows_gemm, 3 * H, H, 1, p.k_qkv, p.rows, p.rows_pad, ("qkv",) + what)
                _check_gemm(lib, p.rows_out, H, H, 0, p.k_out, p.rows, p.rows_pad, ("out_proj",) + what)
                _check_gemm(lib, p.rows_gemm, mlp, H, 1, p.k_fc1, p.rows, p.rows_pad, ("fc1",) + what)
                _check_gemm(lib, p.rows_fc2, H, mlp, 0, p.k_fc2, p.rows, p.rows_pad, ("fc2",) + what)
                if is_text:
                    assert (p.cls_only_last, p.prows_gemm, p.prow_pad) == (0, 0, 0)
                    continue
                patch_k = (3 * cfg.patch_size ** 2 + 127) // 128 * 128
                assert p.prows == n * (cfg.tokens - 1) and p.prows_gemm <= p.prow_pad
                _check_gemm(lib, p.prows_gemm, H, patch_k, 0, p.k_patch, p.prows, p.prow_pad, ("patch",) + what)
                assert p.cls_only_last == 1
                _check_gemm(lib, p.rows_cls, H, H, 0, p.k_cls, n, p.rows_pad, ("cls out_proj",) + what)
                _check_gemm(lib, p.rows_cls, mlp, H, 1, p.k_cls, n, p.rows_pad, ("cls fc1",) + what)
                if p.fc2_splits:                            # launch_gemm_tn_splitk: 128-row tiles, K in 8 slices of whole 64-column steps; planes in q|k|v
                    assert p.fc2_splits == 8 and p.rows_cls % 128 == 0 and mlp % (8 * 64) == 0 and H % 128 == 0, what
                    assert 8 * p.rows_cls * H * 4 <= p.rows_pad * 3 * H * 2, what
                else:
                    _check_gemm(lib, p.rows_cls, H, mlp, 0, p.k_cls, n, p.rows_pad, ("cls fc2",) + what)


# ---------------------------------------------------------------- layout
# arena bytes, rows_pad, and the offsets of input (frames / ids), rowidx, ps, x, d_out, h, xl, qkv, att, mlp, end of mlp: f911a98's sums and take<> sequences
LAYOUT = {
    ("vit_b32", 256, 0): (458305536, 13056, 176922624, -1, 215457792, 217128960, 257236992, 257761280, 277815296, 287842304, 348004352, 368058368, 448274432),
    ("vit_b32", 256, 1): (281382912, 13056, 0, -1, 38535168, 40206336, 80314368, 80838656, 100892672, 110919680, 171081728, 191135744, 271351808),
    ("vit_l14_336", 8, 0): (735295488, 4864, 612397056, -1, 615106560, 615729152, 635652096, 635676672, 645638144, 650618880, 680503296, 690464768, 730310656),
    ("vit_l14_336", 8, 1): (122898432, 4864, 0, -1, 2709504, 3332096, 23255040, 23279616, 33241088, 38221824, 68106240, 78067712, 117913600),
    ("text", 64, 0): (242013696, 5120, 178288640, 178308352, 178308608, 178963968, 189449728, 189580800, 194823680, 197445120, 213173760, 218416640, 239388160),
}
CONFIGS = {"vit_b32": VIT_B_32, "vit_l14_336": VIT_L_14_336, "text": TEXT_B_32}


@pytest.mark.parametrize("key", list(LAYOUT), ids=lambda k: f"{k[0]}-{k[1]}-{'shared' if k[2] else 'own'}")
def test_layout_is_the_parents(lib, key):
    name, max_batch, shared = key
    cfg = CONFIGS[name]
    is_text = name == "text"
    for flags in (FP16, 0, FP16 | CONCURRENT):              # the layout does not depend on the flags
        p, _ = plan(lib, cfg, max_batch, 1, flags=flags, shared=shared)
        offs = (p.off_input, p.off_rowidx, p.off_ps, p.off_x, p.off_out, p.off_h, p.off_xl, p.off_qkv, p.off_att, p.off_mlp)
        assert (p.arena_bytes, p.rows_pad) + offs + (p.workspace_end,) == LAYOUT[key]
    H, R_ = cfg.hidden, p.rows_pad
    T = cfg.max_positions if is_text else cfg.tokens
    assert R_ % 256 == 0 and R_ >= max_batch * T + 159      # room for 256- and 160-row padding
    patch_k = 0 if is_text else (3 * cfg.patch_size ** 2 + 127) // 128 * 128
    need = [max_batch * T * 4 if is_text else max_batch * cfg.image_size ** 2 * 3, max_batch * 4 if is_text else None,
            16 * R_ * 8, R_ * H * 4, max_batch * cfg.proj_dim * 4, R_ * H * 2, R_ * H, R_ * 3 * H * 2, R_ * H * 2,
            max(R_ * cfg.mlp, p.prow_pad * patch_k) * 2]    # what the kernels address: xl one byte per element, mlp also the patch rows
    spans = [(o, o + b) for o, b in zip(offs, need) if b is not None]
    assert all(o % 256 == 0 for o, _ in spans)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "buffers overlap or are out of order"
    assert spans[-1][1] == p.workspace_end <= p.arena_bytes
    assert p.arena_bytes - p.workspace_end == 4096 + R_ * H      # the named tail: 4096 bytes + the former over-count of xl
    assert (spans[0][0] == 0) == bool(shared)               # a shared handle's arena holds the workspace only


def test_refusals(lib):
    from video_quierer_amd import _lib
    out = _lib.EncoderPlanC()
    c = _lib.VitConfigC(224, 32, 768, 3072, 12, 12, 512, 1e-5)
    t = _lib.TextConfigC(49408, 77, 512, 2048, 12, 8, 512, 49407, 1e-5)
    for args in ((None, None, 8, 1, 1, 0), (ctypes.byref(c), ctypes.byref(t), 8, 1, 1, 0), (None, ctypes.byref(t), 8, 1, 1, 1),
                 (ctypes.byref(c), None, 8, 9, 1, 0), (ctypes.byref(c), None, 0, 1, 1, 0), (ctypes.byref(c), None, 9000, 1, 1, 0)):
        assert lib.vq_debug_encoder_plan(*args, -1, 0, ctypes.byref(out), None) == -1       # VQ_ERR_INVALID
    bad = _lib.VitConfigC(224, 30, 768, 3072, 12, 12, 512, 1e-5)
    assert lib.vq_debug_encoder_plan(ctypes.byref(bad), None, 8, 1, 1, 0, -1, 0, ctypes.byref(out), None) == -1
    assert "image 224 is not a multiple of patch 30" in lib.vq_last_error().decode()
