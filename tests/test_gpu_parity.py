"""GPU parity tests: the HIP path (through the C ABI) against the oracles and the
golden vectors.  Run on the MI355X box with `-m gpu`."""
import os
import sys
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLDEN, INDEX_SEED, synth_frames
from oracle import clip_vit_oracle, knn_oracle

pytestmark = pytest.mark.gpu

# tolerance of the north star: cosine scores within 1e-3 (fp32)
COS_TOL = 1e-3


# ------------------------------------------------------------------ GEMM mainloop
from video_quierer_amd import _lib as _vq_lib_for_collection
HAS_DIAG = hasattr(_vq_lib_for_collection.load(), "vq_debug_gemm_bench")      # a `make DIAG=1` library ($VQ_AMD_LIB): carries kernel 24 since round 4
GEMM_KERNELS = [1, 2, 5, 8, 11, 16] + ([24] if HAS_DIAG else [])  # 24 = four waves, K loop scheduled by hand as one asm text (gemm_asm256.h)  (9 and 13 were measured and rejected: `make EXPERIMENTS=1` builds only, with 3, 4, 7, 10)  16 = deep-prefetch 256x256 with several tiles per workgroup (next tile's first K-tile lands under the epilogue); 13 = 128x256 tiles, 4 waves, 3-slot ring, two workgroups per CU; 9 = two phases of 32 MFMAs per K-tile (half the barriers), buffer_load..lds staging; 8 stages with buffer_load..lds, 11 = 8 with global_load_lds staging; 1 = 128x128, 2 = 256x256 four-phase, 5 = 160x256 ring, 8 = 256x256 four-phase with the deep prefetch  (3 ring, 4 persistent, 7 four-wave, 10 register-double-buffered ring: `make EXPERIMENTS=1` builds only)


@pytest.mark.parametrize("kernel", GEMM_KERNELS)
def test_gemm_mfma_integer_exact(gpu_lib, kernel):
    from video_quierer_amd.encoder import debug_gemm
    rng = np.random.default_rng(0)
    m, n, k = (640 if kernel == 5 else 512), 256, 384
    a = np.zeros((m, k), np.float32)
    a[np.arange(m), np.arange(m) % k] = 1.0                  # row i picks column i % k  ("A = I" check)
    w = rng.integers(-8, 9, (n, k)).astype(np.float32)       # asymmetric W catches a transposed C write
    c = debug_gemm(a, w, kernel=kernel)
    assert np.array_equal(c, a @ w.T)
    a = rng.integers(-4, 5, (m, k)).astype(np.float32)
    for f16 in (False, True):
        assert np.array_equal(debug_gemm(a, w, use_f16=f16, kernel=kernel), a @ w.T)   # small ints: exact
    # many k-tiles and several workgroups per XCD: exercises the steady-state pipeline and the tile remap
    m, n, k = (960 if kernel == 5 else 1024), 768, 3072
    a = rng.integers(-2, 3, (m, k)).astype(np.float32)
    w = rng.integers(-2, 3, (n, k)).astype(np.float32)
    assert np.array_equal(debug_gemm(a, w, kernel=kernel), a @ w.T)


def test_gemm_auto_tail_split_is_exact(gpu_lib):
    """300 tiles of 256x256 = one full round of 256 CUs + 44: the auto dispatch sends the thin round's rows to the
    128x128 kernel (two launches); integer data -> exact, and identical to the single-kernel result."""
    from video_quierer_amd.encoder import debug_gemm
    rng = np.random.default_rng(2)
    m, n, k = 7680, 2560, 128
    a = rng.integers(-3, 4, (m, k)).astype(np.float32)
    w = rng.integers(-3, 4, (n, k)).astype(np.float32)
    c = debug_gemm(a, w, kernel=0)
    assert np.array_equal(c, a @ w.T)
    ar = rng.standard_normal((m, k)).astype(np.float32)
    wr = rng.standard_normal((n, k)).astype(np.float32)
    assert np.array_equal(debug_gemm(ar, wr, kernel=0), debug_gemm(ar, wr, kernel=2))      # bit-identical to one 256x256 launch


def test_gemm_multi_tile_workgroups_are_exact(gpu_lib):
    """Kernel 16 with three, two and four tiles of a tile row per workgroup (n = 768 / 512 / 1024; four is what ViT-L/14@336's
    q|k|v GEMM takes when batches run concurrently): the next tile's first K-tile lands in buffer 0 while the epilogue of the
    current one still reads its strips — small integers make any mix-up visible."""
    from video_quierer_amd.encoder import debug_gemm
    rng = np.random.default_rng(5)
    for n in (768, 512, 1024):
        a = rng.integers(-4, 5, (512, 640)).astype(np.float32)
        w = rng.integers(-8, 9, (n, 640)).astype(np.float32)
        for f16 in (False, True):
            c = debug_gemm(a, w, use_f16=f16, kernel=16)
            assert np.array_equal(c, a @ w.T), (n, f16)
            assert np.array_equal(c, debug_gemm(a, w, use_f16=f16, kernel=8))


def test_gemm_mainloops_at_their_shortest_k(gpu_lib):
    """The 256x256 pipelines at K = 128: two K-tiles, all of which the prologue has staged - `next2` is never true and the loop
    body runs once - and at K = 256, the first length with a steady-state trip; the 128x128 kernel at the one K-tile its launcher
    accepts (K % 64 == 0, K >= 64).  Every 256-row / 256-column tile count up to 3 x 6: under id 16 that is 1, 2, 3, 4 and 3 tiles
    per workgroup, and N = 1536 puts two workgroups on a tile row.  Small integers, asymmetric W: every result is exact, and the
    multi-tile kernel's is the deep kernel's bit for bit."""
    from video_quierer_amd.encoder import debug_gemm
    from encoder_stage_run import MULTI, plan_kernels
    lib = gpu_lib.load()
    for m in (256, 768):        # id 16 must BE the multi-tile kernel at these counts, or "16 equals 8" below compares 8 with itself
        for n, tpw in ((256, 1), (512, 2), (768, 3), (1024, 4), (1536, 3)):
            for k in (128, 256):
                assert plan_kernels(lib, m, n, k, MULTI) == [(MULTI, m, 0, tpw)], (m, n, k)
    rng = np.random.default_rng(9)
    a_all = rng.integers(-4, 5, (768, 256)).astype(np.float32)
    w_all = rng.integers(-8, 9, (1536, 256)).astype(np.float32)
    for k in (128, 256):
        for m in (256, 768):
            for n in (256, 512, 768, 1024, 1536):
                a, w = np.ascontiguousarray(a_all[:m, :k]), np.ascontiguousarray(w_all[:n, :k])
                ref = a @ w.T
                for f16 in (False, True):
                    got = {kernel: debug_gemm(a, w, use_f16=f16, kernel=kernel) for kernel in (2, 8, 11, 16)}
                    for kernel, c in got.items():
                        assert np.array_equal(c, ref), (kernel, m, n, k, f16)
                    assert np.array_equal(got[16], got[8]), (m, n, k, f16)
    for m in (256, 768):
        for n in (256, 1536):
            a, w = np.ascontiguousarray(a_all[:m, :64]), np.ascontiguousarray(w_all[:n, :64])
            for f16 in (False, True):
                assert np.array_equal(debug_gemm(a, w, use_f16=f16, kernel=1), a @ w.T), (1, m, n, 64, f16)


@pytest.mark.parametrize("kernel", GEMM_KERNELS)
def test_gemm_mfma_random(gpu_lib, kernel):
    from video_quierer_amd.encoder import debug_gemm
    rng = np.random.default_rng(1)
    m, n, k = (640 if kernel == 5 else 512), 256, 3072
    a = rng.standard_normal((m, k)).astype(np.float32)
    w = rng.standard_normal((n, k)).astype(np.float32)
    ab = torch.from_numpy(a).bfloat16().float().numpy()
    wb = torch.from_numpy(w).bfloat16().float().numpy()
    ref = ab.astype(np.float64) @ wb.astype(np.float64).T
    c = debug_gemm(a, w, kernel=kernel)
    assert np.abs(c - ref).max() <= 2e-3 * np.sqrt(k)        # fp32 accumulation of exact bf16 products
    # repeated launches give identical bits (no race between the DMA ring and the fragment reads)
    for _ in range(5):
        assert np.array_equal(debug_gemm(a, w, kernel=kernel), c)


# ------------------------------------------------------------------ encoder
@pytest.fixture(scope="module")
def encoder(gpu_lib, b32_weights):
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    enc = VitEncoder(VIT_B_32, b32_weights, max_batch=64)
    yield enc
    enc.close()


def _oracle_hidden(frames, weights, layers):
    W = {k: torch.from_numpy(v) for k, v in weights.items()}
    with torch.no_grad():
        px = clip_vit_oracle.preprocess_u8(frames, True)
        return clip_vit_oracle.vit_forward(px, W, patch=32, heads=12, layers=layers, return_hidden=True).numpy()


@pytest.mark.parametrize("layers", [0, 1, 12])
def test_encoder_residual_stream_layerwise(encoder, b32_weights, layers):
    frames = synth_frames(4, seed=99)
    encoder.debug_set_layers(layers)
    try:
        encoder.encode(frames)
        x = encoder.debug_read("x", 4 * 50).reshape(4, 50, 768)
    finally:
        encoder.debug_set_layers(-1)
    ref = _oracle_hidden(frames, b32_weights, layers)
    rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    assert rel < (2e-3 if layers == 0 else 1.5e-2), f"residual stream after {layers} layers: rel err {rel}"


def test_encoder_matches_golden_embeddings(encoder, golden_encoder):
    emb = encoder.encode(synth_frames(64))
    assert emb.shape == (64, 512) and emb.dtype == np.float32
    assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)
    cos = np.sum(emb * golden_encoder["embeddings"], axis=1)
    assert cos.min() >= 1.0 - COS_TOL, f"min cosine vs transformers fp32 = {cos.min()}"
    # cosine scores against arbitrary index rows, all 64,000 pairs: the north star's "cosine scores within 1e-3"
    rows = knn_oracle.normalize_rows(np.random.default_rng(INDEX_SEED).standard_normal((1000, 512)).astype(np.float32))
    diff = np.abs(emb @ rows.T - golden_encoder["embeddings"] @ rows.T)
    print(f"encoder ({encoder.compute_dtype}) vs golden: min cos {cos.min():.7f}, "
          f"score diff rms {np.sqrt((diff**2).mean()):.2e} max {diff.max():.2e}")
    assert diff.max() <= COS_TOL


def test_encoder_parity_with_outlier_channels(gpu_lib):
    """Weights with the outlier structure of trained checkpoints (conftest.outlier_weights: massive-activation channels
    in the residual stream, log-normal LayerNorm gains, heavy-tailed linear weights): the default operand types still
    hold the north star's 1e-3 on every score, against the fp32 oracle run here on the same frames."""
    from conftest import outlier_weights
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    W = outlier_weights()
    frames = synth_frames(32, seed=4242)
    ref = clip_vit_oracle.encode_frames(frames, W, batch_size=16)
    hid = _oracle_hidden(frames[:4], W, 3)
    ratio = np.abs(hid).max() / np.median(np.abs(hid))
    assert ratio > 30, f"the fixture lost its outliers: max/median |x| = {ratio}"       # the residual stream really has them
    rows = knn_oracle.normalize_rows(np.random.default_rng(INDEX_SEED).standard_normal((1000, 512)).astype(np.float32))
    for dt in ("mixed", "fp16"):
        enc = VitEncoder(VIT_B_32, W, max_batch=32, compute_dtype=dt)
        emb = enc.encode(frames)
        enc.close()
        cos = np.sum(emb * ref, axis=1)
        diff = np.abs(emb @ rows.T - ref @ rows.T)
        print(f"outlier weights ({dt}): residual max/median {ratio:.0f}, min cos {cos.min():.7f}, score diff max {diff.max():.2e}")
        assert np.all(np.isfinite(emb)) and cos.min() >= 1.0 - COS_TOL
        assert diff.max() <= COS_TOL


def test_encoder_fp16_operands_are_8x_closer(gpu_lib, b32_weights, golden_encoder):
    """compute_dtype="fp16": same kernels instantiated for fp16 MFMA operands (what ViT-L/14@336 is specified
    with); the embedding error drops from ~5e-3 (bf16) to <1e-3 in L2 and every pairwise score is within 3e-4."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    enc = VitEncoder(VIT_B_32, b32_weights, max_batch=64, compute_dtype="fp16")
    emb = enc.encode(synth_frames(64))
    enc.close()
    err = np.linalg.norm(emb - golden_encoder["embeddings"], axis=1)
    assert err.max() <= 1.5e-3, err.max()
    rows = knn_oracle.normalize_rows(np.random.default_rng(INDEX_SEED).standard_normal((1000, 512)).astype(np.float32))
    diff = np.abs(emb @ rows.T - golden_encoder["embeddings"] @ rows.T)
    assert diff.max() <= 3e-4
    print(f"fp16 operands: max L2 err {err.max():.2e}, max score diff {diff.max():.2e}")


@pytest.mark.skipif(not HAS_DIAG, reason="kernel 24 is compiled into diagnostic libraries only (make DIAG=1; VQ_AMD_LIB=...)")
def test_encoder_hand_scheduled_gemms_are_bit_identical(gpu_lib, b32_weights, monkeypatch):
    """$VQ_AMD_GEMM24 = 31 sends every full-batch GEMM of the tower (patch embedding, qkv, out_proj, fc1, fc2) through the
    four-wave kernel whose K loop is one hand-scheduled asm text (csrc/gemm_asm256.h): same MFMA order per accumulator and the
    same epilogue arithmetic, so 256 frames must encode to the SAME bits as the default kernels - with each of the tower's
    epilogues (LayerNorm-consuming 16-bit stores, residual + LayerNorm partials, position embedding) reading its accumulators
    out of the AGPR half pass by pass."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    frames = synth_frames(256, seed=24)
    out = {}
    for mask in ("0", "31"):
        monkeypatch.setenv("VQ_AMD_GEMM24", mask)
        for concurrent in (False, True):
            enc = VitEncoder(VIT_B_32, b32_weights, max_batch=256, concurrent=concurrent)
            out[mask, concurrent] = enc.encode(frames)
            enc.close()
    assert np.array_equal(out["31", True], out["0", True])
    assert np.array_equal(out["31", False], out["31", True])
    assert np.abs(out["31", False] - out["0", False]).max() <= 2e-3      # a lone handle's default uses 160-row tiles: other padding rows
    ref = clip_vit_oracle.encode_frames(frames[:8], b32_weights, batch_size=8)
    assert np.sum(out["31", True][:8] * ref, axis=1).min() >= 1.0 - COS_TOL


def test_encoder_split_residual_stream(gpu_lib, b32_weights, golden_encoder, monkeypatch):
    """[r04] Between the residual epilogues the stream lives as xh = fp16(x) (the next GEMM's operand, written anyway) and a low half
    xl = x - xh instead of the fp32 x (EpiBiasResidualLnF32 modes).  xl is ONE byte since the round's second session (fp8 e4m3 of
    xl * 512; fp16 before that): 3 bytes in + 3 out per element instead of 4 + 6, the pair carries x to ~15 bits - 16 times finer than
    the fp16 rounding every GEMM applies to its operand.  Against the all-fp32 stream ($VQ_AMD_RESID=f32) the embeddings move by less
    than the fp16 operands' own rounding noise (measured 7.5e-5 per element with either low half; the fp16 path's own error against the
    fp32 oracle is 6.8e-4), and both stay inside the golden tolerance with the same score error; outlier channels included."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    from conftest import outlier_weights
    frames = synth_frames(64)
    for W, gold in ((b32_weights, golden_encoder["embeddings"]), (outlier_weights(), None)):
        out = {}
        for mode in ("f32", "split"):
            monkeypatch.setenv("VQ_AMD_RESID", mode)
            enc = VitEncoder(VIT_B_32, W, max_batch=64)
            out[mode] = enc.encode(frames)
            if mode == "split":                                            # the low half is in use: its bytes are not all zero
                assert enc.debug_read("xl", 64 * 50).any()
            enc.close()
        monkeypatch.delenv("VQ_AMD_RESID")
        d = float(np.abs(out["split"] - out["f32"]).max())
        print(f"split (fp16 + fp8) residual stream vs fp32 stream: max |delta embedding| = {d:.2e}")
        assert d <= 3e-4, d
        assert not np.array_equal(out["split"], out["f32"])               # (the switch does switch)
        if gold is not None:
            err = {m: float(np.abs(o @ gold.T - gold @ gold.T).max()) for m, o in out.items()}     # all 64 x 64 scores against the fp32 pipeline's
            print("max score error against transformers' fp32 pipeline:", err)
            assert max(err.values()) <= COS_TOL and err["split"] <= 1.5 * err["f32"] + 2e-5


def test_encoder_single_tile_attention_forms_agree(gpu_lib, b32_weights, golden_encoder, monkeypatch):
    """[r04] ViT-B/32's 50-token attention runs in attention_tile_kernel<50> (compile-time T: descriptor-ranged loads, V by LDS-DMA
    into a swizzled tile, dead key registers skipped, exp2 in the log2 domain); $VQ_AMD_ATTN=t64 selects the run-time-T kernel of
    rounds 1-3.  Same MFMA operand layouts and accumulation order: the embeddings differ only by exp2(fma(s, log2e, -m log2e))
    against exp(s - m) and an approximate reciprocal - well inside the fp16 operands' noise; both stay inside the golden tolerance.
    Outlier channels and a ragged batch (padding rows of the GEMMs next to the last image) included."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    from conftest import outlier_weights
    for W, gold, n in ((b32_weights, golden_encoder["embeddings"], 64), (outlier_weights(), None, 37)):
        frames = synth_frames(n)
        out = {}
        for form in ("t64", "tile"):
            monkeypatch.setenv("VQ_AMD_ATTN", form)
            enc = VitEncoder(VIT_B_32, W, max_batch=64)
            out[form] = enc.encode(frames)
            enc.close()
        monkeypatch.delenv("VQ_AMD_ATTN")
        assert np.isfinite(out["tile"]).all()
        d = float(np.abs(out["tile"] - out["t64"]).max())
        print(f"compile-time-T attention vs run-time-T attention ({n} frames): max |delta embedding| = {d:.2e}")
        assert d <= 3e-4, d
        assert not np.array_equal(out["tile"], out["t64"])                 # (the switch does switch)
        if gold is not None:
            err = {m: float(np.abs(o @ gold.T - gold @ gold.T).max()) for m, o in out.items()}
            print("max score error against transformers' fp32 pipeline:", err)
            assert max(err.values()) <= COS_TOL and err["tile"] <= 1.5 * err["t64"] + 2e-5


def test_shared_weight_handles(gpu_lib, b32_weights):
    """vq_encoder_create_shared: clones run on the parent's device weights with their own stream and workspace; results
    are bit-identical to the parent's (same kernels), concurrent use is safe, and either side may be closed first."""
    from concurrent.futures import ThreadPoolExecutor
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    parent = VitEncoder(VIT_B_32, b32_weights, max_batch=16, concurrent=True)
    a, b = parent.clone(), parent.clone(max_batch=8)
    frames = synth_frames(16, seed=21)
    want = parent.encode(frames)
    with ThreadPoolExecutor(3) as pool:
        got = list(pool.map(lambda h: h.encode(frames), (parent, a, b)))       # b runs two passes of 8
    assert all(np.array_equal(g, want) for g in got[:2])
    assert np.abs(got[2] - want).max() <= 2e-3                                  # batch 8: other GEMM row padding
    parent.close()                                                              # the clones keep the weights alive
    assert np.array_equal(a.encode(frames), want)
    c = a.clone()
    a.close()
    assert np.array_equal(c.encode(frames), want)
    b.close(); c.close()


def test_encoder_batch_shapes_and_paths(encoder, b32_weights):
    frames = synth_frames(70, seed=3)                 # > max_batch=64: two device passes, ragged tail of 6
    full = encoder.encode(frames)
    assert full.shape == (70, 512)
    one = encoder.encode(frames[17:18])
    assert np.abs(one[0] - full[17]).max() <= 2e-3    # batch composition only changes GEMM padding rows
    again = encoder.encode(frames)
    assert np.array_equal(full, again)                # deterministic
    rgb = encoder.encode(np.ascontiguousarray(frames[:5, ..., ::-1]), swap_rb=False)   # PIL path
    assert np.array_equal(rgb, full[:5])
    assert encoder.encode(frames[:0]).shape == (0, 512)
    ref = clip_vit_oracle.encode_frames(frames[:8], b32_weights, batch_size=8)
    assert np.sum(full[:8] * ref, axis=1).min() >= 1.0 - COS_TOL
    with pytest.raises(ValueError):
        encoder.encode(np.zeros((1, 200, 224, 3), np.uint8))


@pytest.mark.parametrize("tower,n,full_last", [("image", 5, False), ("image", 5, True), ("text", 3, False)])
def test_encoder_runs_what_its_plan_says(gpu_lib, monkeypatch, tower, n, full_last):
    """One profiled pass: the event brackets per kernel class are the counts that follow from vq_debug_encoder_plan's scalars
    (one bracket per full-row GEMM per block, three for a CLS-only last block), for a 3-block T = 50 image tower - with and
    without the CLS-only last block - and the 2-block text tower."""
    import ctypes
    import encoder_stage_ref as R
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.text_encoder import TextEncoder
    from video_quierer_amd.weights import TextConfig, VitConfig
    for name in ("VQ_AMD_GEMM", "VQ_AMD_RESID", "VQ_AMD_ATTN", "VQ_AMD_FULL_LAST_LAYER", "VQ_AMD_DTYPE"):
        monkeypatch.delenv(name, raising=False)
    if full_last:
        monkeypatch.setenv("VQ_AMD_FULL_LAST_LAYER", "1")
    lib = gpu_lib.load()
    plan = gpu_lib.EncoderPlanC()
    if tower == "text":
        cfg = TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, layers=2)
        c = gpu_lib.TextConfigC(cfg.vocab, cfg.max_positions, cfg.hidden, cfg.mlp, cfg.layers, cfg.heads, cfg.proj_dim, cfg.eos_token_id, cfg.ln_eps)
        assert lib.vq_debug_encoder_plan(None, ctypes.byref(c), n, n, 1, 0, -1, 0, ctypes.byref(plan), None) == 0
        enc = TextEncoder(cfg, R.make_weights(tower, cfg, "seeded"), max_batch=n, compute_dtype="fp16")
        run = enc.encode_ids
    else:
        cfg = VitConfig(layers=3)
        c = gpu_lib.VitConfigC(cfg.image_size, cfg.patch_size, cfg.hidden, cfg.mlp, cfg.layers, cfg.heads, cfg.proj_dim, cfg.ln_eps)
        assert lib.vq_debug_encoder_plan(ctypes.byref(c), None, n, n, 1, 0, -1, 0, ctypes.byref(plan), None) == 0
        enc = VitEncoder(cfg, R.make_weights(tower, cfg, "seeded"), max_batch=n, compute_dtype="fp16")
        run = enc.encode
    assert (plan.layers_run, plan.cls_only_last) == (cfg.layers, int(tower == "image" and not full_last))
    full = plan.layers_run - plan.cls_only_last             # blocks that run on every row
    image = int(tower == "image")
    want = {"patchify_u8": image, "gemm_patch_embed": image, "embed_finish_ln": 1, "layernorm_bf16": 0, "gemm_qkv": plan.layers_run,
            "attention": plan.layers_run, "gemm_out_proj_residual": full, "gemm_fc1_quickgelu": full, "gemm_fc2_residual": full,
            "pool_project": 1, "last_block_cls_rows": 3 * plan.cls_only_last}
    ms, cnt = (ctypes.c_float * gpu_lib.ENC_NCLASS)(), (ctypes.c_int * gpu_lib.ENC_NCLASS)()
    try:
        inp = R.make_input(tower, cfg, n)
        plain = run(inp)
        gpu_lib.check(lib.vq_encoder_profile_begin(enc._h))
        emb = run(inp)
        gpu_lib.check(lib.vq_encoder_profile_end(enc._h, ms, cnt))
    finally:
        enc.close()
    got = {lib.vq_encoder_profile_class_name(i).decode(): cnt[i] for i in range(gpu_lib.ENC_NCLASS)}
    assert got == want
    assert all(ms[i] > 0.0 for i in range(gpu_lib.ENC_NCLASS) if cnt[i])
    assert np.array_equal(emb, plain) and np.all(np.isfinite(emb))      # the brackets change nothing


def test_feature_extractor_api(gpu_lib, b32_weights):
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    fx = FeatureExtractor(model_name="seed:1234", batch_size=32, device_batch=64)
    assert fx.output_dim == 512 and fx.batch_size == 32 and str(fx.device).startswith("cuda")
    assert fx.get_stats() == {"total_processed": 0, "avg_extraction_time": 0, "throughput": 0}
    assert fx.extract_batch([]).shape == (0,)
    frames = synth_frames(70, seed=21)
    fd = [{"frame": f, "timestamp": i / 30.0, "frame_number": i} for i, f in enumerate(frames)]
    out = fx.extract_from_video_frames(fd)
    assert len(out) == 70 and [o["frame_number"] for o in out] == list(range(70))
    assert "features" not in fd[0] and out[0]["features"].shape == (512,) and out[0]["features"].dtype == np.float32
    assert all(o["feature_extraction_time"] >= 0 for o in out)
    ref = clip_vit_oracle.extract_from_video_frames(fd[:6], b32_weights, batch_size=32)
    for o, r in zip(out[:6], ref):
        assert float(np.dot(o["features"], r["features"])) >= 1.0 - COS_TOL
    single = fx.extract_features(frames[3])
    assert float(np.dot(single, out[3]["features"])) >= 1.0 - 1e-4
    from PIL import Image
    pil = fx.extract_features(Image.fromarray(np.ascontiguousarray(frames[3][..., ::-1])))   # RGB PIL == BGR ndarray
    assert np.allclose(pil, single, atol=2e-3)
    st = fx.get_stats()
    assert set(st) == {"total_processed", "avg_extraction_time", "throughput_images_per_sec", "device",
                       "model_name", "output_dimension"} and st["total_processed"] == 72
    with pytest.raises(NotImplementedError):
        fx.extract_text_features("a cat")          # seeded model: no tokenizer files
    with pytest.raises(RuntimeError):
        FeatureExtractor(model_name="seed:1234", device="cpu")
    fx.thread_pool.shutdown()


# ------------------------------------------------------------------ index
def _mk_index(vecs, ids=None):
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=vecs.shape[1], M=16, ef_construction=200, ef_search=50, max_M=16)
    idx.add_batch(list(vecs), list(range(len(vecs))) if ids is None else ids)
    return idx


def test_index_config1_matches_reference_and_oracle(gpu_lib, golden_knn, golden_encoder):
    vecs = np.random.default_rng(INDEX_SEED).standard_normal((1000, 512)).astype(np.float32)
    idx = _mk_index(vecs)
    assert idx.size() == 1000
    assert np.array_equal(idx._export(), golden_knn["stored"])          # stored rows == reference .data
    qs = golden_encoder["embeddings"]
    unit_q = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    for k in (5, 10):
        res = idx.search_batch(list(qs), k)
        ids = np.array([[r["id"] for r in rr] for rr in res], dtype=np.int32)
        d = np.array([[r["distance"] for r in rr] for rr in res], dtype=np.float32)
        sc = np.array([[r["score"] for r in rr] for rr in res], dtype=np.float32)
        oid, od = knn_oracle.topk(golden_knn["stored"], unit_q, k)
        assert np.array_equal(ids, oid) and np.array_equal(d, od)       # bit-exact vs the oracle
        assert np.array_equal(ids, golden_knn[f"ids_ef1000_k{k}"])      # identical lists vs the exhaustive reference
        assert np.abs(d - golden_knn[f"dist_ef1000_k{k}"]).max() <= 2e-7
        assert np.abs(sc - golden_knn[f"score_ef1000_k{k}"]).max() <= 2e-7
        one = idx.search(qs[5], k)
        assert [r["id"] for r in one] == list(ids[5]) and type(one[0]["distance"]) is np.float32
    st = idx.get_stats()
    assert st["element_count"] == 1000 and st["total_searches"] == 64 * 2 + 2 and st["M"] == 16 and st["ef_search"] == 50
    idx.thread_pool.shutdown()


@pytest.mark.parametrize("n", [10_000, 100_000])
def test_index_matches_the_real_reference_above_1k_rows_with_the_callers_string_ids(gpu_lib, n):
    """configs[2] / north_star "top-k recall@10 = 1.0 vs reference", pinned against the REAL OptimizedHNSWIndex at 10k and 100k
    rows (tests/golden/knn_ref_<n>.npz, `make_golden.py knn_big <n>`: config 3's recipe at prefix size, built in the
    container under the caller's string ids, with planted duplicate frames).  The reference at ef_search = N is exhaustive
    (64/64 of its lists equal the exact answer); the drop-in, called the way video_search_system.py:164-181, :297 calls it
    — one add_batch per video, string ids, one query at a time, k*2 results — returns the identical id lists."""
    import hashlib
    from conftest import knn_big_ids, knn_big_inputs
    from video_quierer_amd.indexes.hnsw import MODE_FP16, OptimizedHNSWIndex
    path = os.path.join(GOLDEN, f"knn_ref_{n}.npz")
    if not os.path.exists(path):
        pytest.skip(f"{os.path.basename(path)} not captured")
    ref = np.load(path)
    rows, qs = knn_big_inputs(n)
    ids = knn_big_ids(n)
    row_of = {s: r for r, s in enumerate(ids)}
    idx = OptimizedHNSWIndex(dimension=512, M=16, ef_construction=200, ef_search=50, max_M=16)
    per = n // 4
    for v in range(4):                                                    # one add_batch per video (video_search_system.py:181)
        idx.add_batch(rows[v * per:(v + 1) * per], ids[v * per:(v + 1) * per])
    stored = idx._export()
    assert hashlib.sha256(stored.tobytes()).hexdigest() == str(ref["stored_sha256"])      # stored rows == the reference's .data, all of them
    assert np.array_equal(stored[:64], ref["stored_head"]) and np.array_equal(stored[-64:], ref["stored_tail"])
    unit_q = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    modes = (idx.search_mode,) if n >= 16384 else (idx.search_mode, MODE_FP16)       # 10k rows: auto = the exact scan; force the fp16 path too
    for mode in modes:
        idx.search_mode = mode
        for k in (10, 20):
            one = [idx.search(q, k) for q in qs]                          # the caller's call: one query at a time (:297)
            got = np.array([[row_of[r["id"]] for r in rr] for rr in one], dtype=np.int32)
            d = np.array([[r["distance"] for r in rr] for rr in one], dtype=np.float32)
            assert np.array_equal(got, ref[f"rows_ef{n}_k{k}"]), (mode, k)                 # identical lists vs the exhaustive reference
            assert np.abs(d - ref[f"dist_ef{n}_k{k}"]).max() <= 3e-7
            assert np.array_equal(got, ref["rows_exact_k20"][:, :k])                       # == the exact answer in (distance, id) order
            assert np.array_equal(d, ref["dist_exact_k20"][:, :k])                         # bit-exact vs the C oracle's distances
            recall = np.mean([len(set(got[j]) & set(ref[f"rows_ef{n}_k{k}"][j])) / k for j in range(len(qs))])
            assert recall == 1.0
            batch = idx.search_batch(list(qs), k)
            assert [[r["id"] for r in rr] for rr in batch] == [[r["id"] for r in rr] for rr in one]
            assert type(one[0][0]["distance"]) is np.float32 and type(one[0][0]["id"]) is str
    # the planted duplicate frames head their queries' lists in STRING order: "video0_10" before "video0_2"
    assert [r["id"] for r in idx.search(qs[0], 10)[:2]] == ["video0_10", "video0_2"]
    assert [r["id"] for r in idx.search(qs[1], 10)[:3]] == ["video0_100", "video0_20", "video0_3"]
    for k in (10, 20):
        print(f"N={n}: reference default-ef (50) recall@{k} against the exact list = {float(ref[f'default_ef_recall_k{k}']):.4f} "
              f"({float(ref[f'ms_per_query_ef50_k{k}']):.1f} ms/query; exhaustive ef=N: {float(ref[f'ms_per_query_ef{n}_k{k}']):.0f} ms/query); "
              f"this build: 1.0000")
    idx.close()


def test_index_edge_cases(gpu_lib, tmp_path):
    from video_quierer_amd.indexes.hnsw import HNSWIndex, OptimizedHNSWIndex
    rng = np.random.default_rng(5)
    empty = HNSWIndex(dimension=64)
    assert empty.search(rng.standard_normal(64).astype(np.float32), 3) == [] and empty.size() == 0
    assert empty.search_batch([rng.standard_normal(64).astype(np.float32)] * 2, 3) == [[], []]

    vecs = rng.standard_normal((37, 64)).astype(np.float32)          # ragged: not a multiple of any tile
    idx = _mk_index(vecs)
    q = rng.standard_normal(64).astype(np.float32)
    res = idx.search(q, 50)                                           # k > n → n results
    assert len(res) == 37 and sorted(r["id"] for r in res) == list(range(37))
    d = [r["distance"] for r in res]
    assert d == sorted(d)

    # exact duplicates: ties broken by the smaller id — numeric ids and (lexicographic) string ids
    dup = np.concatenate([vecs, vecs[:4]])
    idx2 = _mk_index(dup)
    r2 = idx2.search(vecs[2], 2)
    assert [r["id"] for r in r2] == [2, 39] and r2[0]["distance"] == r2[1]["distance"]
    names = [f"v_{i}" for i in range(len(dup))]
    names[2], names[39] = "z_2", "a_39"                              # the LATER row carries the smaller id
    idx3 = _mk_index(dup, ids=names)
    r3 = idx3.search(vecs[2], 2)
    assert [r["id"] for r in r3] == ["a_39", "z_2"] and r3[0]["distance"] == r3[1]["distance"]
    r3b = idx3.search(vecs[2], 1)                                     # tie group cut at rank k: still the smaller id
    assert r3b[0]["id"] == "a_39"
    assert idx3.search(vecs[3], 1)[0]["id"] == "v_3"                  # "v_3" < "v_40"

    # incremental adds, re-add of an existing id replaces its vector
    idx.add(vecs[0] * 3.0, 100)
    assert idx.size() == 38 and idx.search(vecs[0], 2)[1]["id"] in (0, 100)
    idx.add(vecs[5], 1)                                               # id 1 now holds vecs[5]
    top = idx.search(vecs[5], 2)
    assert {top[0]["id"], top[1]["id"]} == {1, 5}

    # save / load round trip (pickle + sha256 sidecar, reference keys)
    path = os.path.join(tmp_path, "sub", "index.pkl")
    idx3.save(path)
    with open(path, "rb") as f:
        blob = pickle.load(f)
    for key in ("dimension", "M", "max_M", "ef_construction", "ef_search", "level_generation_factor", "data",
                "levels", "graph", "entry_point", "element_count"):
        assert key in blob
    fresh = OptimizedHNSWIndex(dimension=64)
    fresh.load(path)
    assert fresh.size() == idx3.size()
    assert [r["id"] for r in fresh.search(vecs[2], 2)] == [r["id"] for r in r3]
    with open(path, "ab") as f:
        f.write(b"x")
    with pytest.raises(ValueError):
        OptimizedHNSWIndex(dimension=64).load(path)
    with pytest.raises(ValueError):
        idx.search(np.zeros(32, np.float32), 1)                       # wrong dimension
    assert idx.search(vecs[0], 0) == [] and idx.search_batch([vecs[0], vecs[1]], 0) == [[], []]      # k = 0: reference slices [:0]


def test_index_readd_replaces_rows_in_place(gpu_lib):
    """hnsw.py:160 `self.data[node_id] = vector`: re-adding ids that are already stored replaces their rows in place
    (vq_index_update_rows: fp32 master + fp16 scan copy + norm range) — 1,000 of 100,000 rows re-ingested in one
    add_batch, one id twice (the later vector stays), mixed with 50 new ids.  The index must equal a fresh build of the
    updated matrix bit for bit, and its searches (fp16 scan, single query and batch) the oracle on that matrix."""
    rng = np.random.default_rng(160)
    n, d = 100_000, 512
    vecs = rng.standard_normal((n, d)).astype(np.float32)
    idx = _mk_index(vecs)
    redo = rng.choice(n, 1000, replace=False)
    newv = rng.standard_normal((1000, d)).astype(np.float32)
    extra = rng.standard_normal((50, d)).astype(np.float32)
    again = rng.standard_normal(d).astype(np.float32)                     # a second vector for redo[7] in the same call
    batch = np.concatenate([newv[:500], extra[:20], newv[500:], again[None], extra[20:]])
    ids = list(redo[:500]) + list(range(n, n + 20)) + list(redo[500:]) + [int(redo[7])] + list(range(n + 20, n + 50))
    idx.add_batch(list(batch), [int(i) for i in ids])
    want = np.concatenate([vecs, extra])
    want[redo] = newv
    want[redo[7]] = again
    assert len(idx._ids) == n + 50 and idx.size() == idx.element_count == n + len(ids)     # the reference's size() counts every add (:229, :302)
    stored = np.stack([v / np.linalg.norm(v) for v in want]).astype(np.float32)
    assert np.array_equal(idx._export(), stored)
    fresh = _mk_index(want)
    qs = np.concatenate([newv[:40], again[None], rng.standard_normal((87, d)).astype(np.float32)])
    uq = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    oid, od = knn_oracle.topk(stored, uq, 10)
    for index in (idx, fresh):
        res = index.search_batch(list(qs), 10)
        assert np.array_equal(np.array([[r["id"] for r in rr] for rr in res]), oid)
        assert np.array_equal(np.array([[r["distance"] for r in rr] for rr in res], dtype=np.float32), od)
    one = idx.search(again, 10)                                           # streaming scan (one query) reads the fp16 copy too
    assert [r["id"] for r in one] == list(oid[40]) and one[0]["id"] == int(redo[7])
    with pytest.raises(ValueError):                                       # a row outside the index is refused by the library
        idx._overwrite([n + 50], stored[:1])
    idx.close(); fresh.close()


def test_search_unnormalised_queries_at_any_scale(gpu_lib):
    """Raw C-ABI callers may hand over queries that are not unit vectors (the Python hosts normalise, hnsw.py:250).
    The fp16 scans' error bound is relative to |q| only while the query's elements stay in fp16's normal range; outside
    0.25 <= |q|^2 <= 4 (fp16 subnormals / flush at 1e-5, inf at 1e5) the re-score kernels must not call a result
    proven: such queries go to the exact fallback.  mode 2 (fp16 scan forced), single query and batches, ids and
    distances bit-exact against the oracle on the SAME un-normalised queries."""
    from video_quierer_amd import _lib
    import ctypes
    lib = _lib.load()
    rng = np.random.default_rng(2501)
    n, d, k = 20_000, 512, 10
    rows = knn_oracle.normalize_rows(rng.standard_normal((n, d)).astype(np.float32))
    h = ctypes.c_void_p()
    _lib.check(lib.vq_index_create(d, ctypes.byref(h)))
    _lib.check(lib.vq_index_add(h, _lib.fptr(rows), n, 0))
    base = knn_oracle.normalize_rows(rng.standard_normal((300, d)).astype(np.float32))
    for scale in (1e-8, 1e-5, 1e-3, 0.3, 1.0, 1.9, 2.5, 1e5):
        for nq in (1, 40):                                   # streaming scan / (33+: two passes) and its re-score kernels
            q = np.ascontiguousarray(base[:nq] * np.float32(scale), dtype=np.float32)
            ids = np.empty((nq, k), np.int32); dist = np.empty((nq, k), np.float32)
            _lib.check(lib.vq_index_search(h, _lib.fptr(q), nq, k, 2, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _lib.fptr(dist)))
            oid, od = knn_oracle.topk(rows, q, k)
            assert np.array_equal(ids, oid), f"scale {scale} nq {nq}"
            assert np.array_equal(dist, od), f"scale {scale} nq {nq}"
            st = (ctypes.c_int64 * 3)()
            _lib.check(lib.vq_index_last_search_stats(h, st))
            if not (0.25 <= scale * scale <= 4.0):
                assert st[2] == nq, f"scale {scale}: {st[2]} of {nq} queries took the exact fallback"      # none may be 'proven'
            elif scale == 1.0:
                assert st[2] == 0
    q = np.ascontiguousarray(base * np.float32(1e-5))     # the MFMA-tile scan + batch re-score kernel
    q[::2] *= np.float32(1e5)                                                   # every other query back at unit scale
    ids = np.empty((300, k), np.int32); dist = np.empty((300, k), np.float32)
    _lib.check(lib.vq_index_search(h, _lib.fptr(q), 300, k, 2, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _lib.fptr(dist)))
    oid, od = knn_oracle.topk(rows, q, k)
    assert np.array_equal(ids, oid) and np.array_equal(dist, od)
    st = (ctypes.c_int64 * 3)()
    _lib.check(lib.vq_index_last_search_stats(h, st))
    assert st[2] >= 150
    lib.vq_index_destroy(h)


def test_index_device_normalise_matches_oracle(gpu_lib):
    from video_quierer_amd import _lib
    import ctypes
    rng = np.random.default_rng(8)
    raw = (rng.standard_normal((300, 512)) * 3).astype(np.float32)
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vq_index_create(512, ctypes.byref(h)))
    _lib.check(lib.vq_index_add(h, _lib.fptr(raw), 300, 1))            # normalize on the device
    out = np.empty_like(raw)
    _lib.check(lib.vq_index_export(h, _lib.fptr(out)))
    lib.vq_index_destroy(h)
    assert np.array_equal(out, knn_oracle.normalize_rows(raw))         # same fixed-order definition, bit-exact


def test_index_larger_ragged_vs_oracle(gpu_lib):
    rng = np.random.default_rng(12)
    vecs = rng.standard_normal((4001, 512)).astype(np.float32)        # config-4 sized, ragged
    idx = _mk_index(vecs)
    qs = rng.standard_normal((130, 512)).astype(np.float32)
    res = idx.search_batch(list(qs), 10)
    stored = np.stack([v / np.linalg.norm(v) for v in vecs]).astype(np.float32)
    uq = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    oid, od = knn_oracle.topk(stored, uq, 10)
    assert np.array_equal(np.array([[r["id"] for r in rr] for rr in res]), oid)
    assert np.array_equal(np.array([[r["distance"] for r in rr] for rr in res], dtype=np.float32), od)


# ------------------------------------------------------------------ end to end (config 1)
def test_config1_end_to_end(gpu_lib, encoder, golden_knn, golden_encoder):
    emb = encoder.encode(synth_frames(64))
    vecs = np.random.default_rng(INDEX_SEED).standard_normal((1000, 512)).astype(np.float32)
    idx = _mk_index(vecs)
    res = idx.search_batch(list(emb), 5)
    ids = np.array([[r["id"] for r in rr] for rr in res], dtype=np.int32)
    sc = np.array([[r["score"] for r in rr] for rr in res], dtype=np.float32)
    # exactness of the search on the GPU embeddings themselves
    uq = np.stack([q / np.linalg.norm(q) for q in emb]).astype(np.float32)
    oid, od = knn_oracle.topk(golden_knn["stored"], uq, 5)
    assert np.array_equal(ids, oid)
    # against the all-reference pipeline (transformers fp32 embeddings + exhaustive hnsw.py, hnsw.py:517-523
    # score = 1 - distance): EVERY returned (id, score), at k = 5 and k = 10, is within 1e-3 of the reference
    # pipeline's own score for that id; id lists are identical wherever the reference's gaps exceed the tolerance
    ref_emb, stored = golden_encoder["embeddings"], golden_knn["stored"]
    ref_ids, ref_sc = golden_knn["ids_ef1000_k5"], golden_knn["score_ef1000_k5"]
    ref_d10 = golden_knn["dist_ef1000_k10"]
    res10 = idx.search_batch(list(emb), 10)
    worst = 0.0
    for kk, rr_all in ((5, res), (10, res10)):
        for i, rr in enumerate(rr_all):
            assert len(rr) == kk
            for r in rr:
                ref_score = np.float32(1.0) - (np.float32(1.0) - np.float32(np.dot(stored[r["id"]], ref_emb[i])))
                worst = max(worst, abs(float(r["score"]) - float(ref_score)))
    assert worst <= COS_TOL, f"a returned score is {worst:.2e} away from the reference pipeline's score for the same id"
    # id lists: identical to the reference's for every query whose reference gaps (between any two neighbours among its
    # first six distances) exceed twice the score error MEASURED above — not twice the 1e-3 tolerance
    same = 0
    for i in range(64):
        if np.diff(ref_d10[i][:6]).min() > 2 * max(worst, 1e-6):
            assert list(ids[i]) == list(ref_ids[i]), f"query {i}: {list(ids[i])} vs reference {list(ref_ids[i])}"
            assert np.abs(sc[i] - ref_sc[i]).max() <= COS_TOL
            same += 1
    # whatever differs from the reference's list is a near-tie: the reference's own score for the id this build
    # returned is within 2e-3 of the reference's k-th score
    for i in range(64):
        kth = ref_sc[i][-1]
        for j in ids[i]:
            assert np.dot(stored[j], ref_emb[i]) >= kth - 2 * COS_TOL
    recall = np.mean([len(set(a) & set(b)) / 5 for a, b in zip(ids, ref_ids)])
    print(f"config1 ({encoder.compute_dtype}): worst |score - reference score| {worst:.2e} over 64x(5+10) results; "
          f"{same}/64 queries gap-checked identical; recall@5 vs reference pipeline {recall:.4f}")
    # the default operand type (all fp16, power-of-two scaled patch weights) reproduces every reference list on config 1
    assert recall == 1.0 if encoder.compute_dtype == "fp16" else recall >= 0.95


def test_config1_recall_by_operand_type(gpu_lib, b32_weights, golden_knn, golden_encoder):
    """recall@5 of the whole pipeline against the all-reference pipeline, per operand-type choice (printed for
    DESIGN.md §2); every choice must keep every returned score within 1e-3 except plain bf16, which is the
    measured reason the default is not plain bf16."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    vecs = np.random.default_rng(INDEX_SEED).standard_normal((1000, 512)).astype(np.float32)
    idx = _mk_index(vecs)
    rows = golden_knn["stored"]
    for dt in ("bf16", "mixed", "fp16"):
        enc = VitEncoder(VIT_B_32, b32_weights, max_batch=64, compute_dtype=dt)
        emb = enc.encode(synth_frames(64))
        enc.close()
        ids = np.array([[r["id"] for r in rr] for rr in idx.search_batch(list(emb), 5)])
        recall = np.mean([len(set(a) & set(b)) / 5 for a, b in zip(ids, golden_knn["ids_ef1000_k5"])])
        diff = np.abs(emb @ rows.T - golden_encoder["embeddings"] @ rows.T)
        print(f"operands {dt:5s}: recall@5 vs reference pipeline {recall:.4f}, max score diff {diff.max():.2e}")
        if dt != "bf16":
            assert diff.max() <= COS_TOL
    idx.close()


# ------------------------------------------------------------------ end to end (config 4 on one GPU)
def test_config4_end_to_end_on_one_gpu(gpu_lib):
    """configs[3]: 4 videos x 1000 synthetic frames (host uint8 frame dicts, as frame_extractor.py yields them) ->
    FeatureExtractor.extract_from_video_frames -> OptimizedHNSWIndex.add_batch with the caller's string ids
    f"{video_id}_{i}" (video_search_system.py:164-181) -> 1000 queries, k = 10, against the exact oracle on the stored
    rows in the reference's (distance, id) order — ids are strings, so ties sort lexicographically, not by row.
    (The 8-GPU form shards the same frame ranges over ranks and all-gathers the rows: tests/test_distributed_cpu.py,
    test_native_comm_world_of_one_over_rccl.)"""
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    videos, per, nq, k = 4, 1000, 1000, 10
    rng = np.random.default_rng(1000)
    frames = rng.integers(0, 255, (videos * per, 224, 224, 3), dtype=np.uint8)
    frames[10] = frames[9]                     # "video0_10" sorts before "video0_9": a tie the row order would get wrong
    fds = [{"frame": frames[g], "timestamp": (g % per) / 30.0, "frame_number": g % per, "video_id": f"video{g // per}"}
           for g in range(videos * per)]
    fx = FeatureExtractor(model_name="seed:1234", batch_size=32, device_batch=256)
    out = fx.extract_from_video_frames(fds)
    assert [o["frame_number"] for o in out] == [g % per for g in range(videos * per)] and "features" in out[0]
    emb = np.stack([o["features"] for o in out])
    assert emb.shape == (4000, 512) and np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)
    assert np.array_equal(emb[9], emb[10])
    ids = [f"{fd['video_id']}_{fd['frame_number']}" for fd in fds]
    idx = OptimizedHNSWIndex(dimension=512)
    idx.add_batch(list(emb), ids)
    assert idx.size() == 4000
    qrng = np.random.default_rng(5)
    src = qrng.integers(0, len(emb), nq)
    src[0] = 9
    queries = emb[src] + 0.05 * qrng.standard_normal((nq, 512)).astype(np.float32)
    queries[0] = emb[9]
    res = idx.search_batch(list(queries), k)
    stored = idx._export()
    uq = np.stack([q / np.linalg.norm(q) for q in queries]).astype(np.float32)
    rows, dist = knn_oracle.topk(stored, uq, k + 8)                      # a few extra so that a tie group at rank k is whole
    for i in range(nq):
        want = sorted((d, ids[r]) for r, d in zip(rows[i], dist[i]))[:k]
        assert [r["id"] for r in res[i]] == [w[1] for w in want], i
        assert np.array_equal(np.array([r["distance"] for r in res[i]], dtype=np.float32), np.array([w[0] for w in want], dtype=np.float32))
    assert [r["id"] for r in res[0][:2]] == ["video0_10", "video0_9"] and res[0][0]["distance"] == res[0][1]["distance"]
    single = idx.search(queries[5], k)                                   # the one-query call the reference makes (:297)
    assert [r["id"] for r in single] == [r["id"] for r in res[5]]
    idx.close()
    fx.thread_pool.shutdown()


# ------------------------------------------------------------------ fp16 MFMA scan + exact re-score
def _expected_in_id_order(stored, unit_q, ids, k):
    """What the reference returns once its walk is exhaustive: ``sorted((distance, id) ...)[:k]`` (hnsw.py:269 / :518) over the
    oracle's exact distances — the ids compared as Python compares them, only where distances tie."""
    out = []
    for q in unit_q:
        d = knn_oracle.distances(stored, q)
        kth = np.partition(d, min(k, len(d)) - 1)[min(k, len(d)) - 1]
        cand = np.nonzero(d <= kth)[0]                                   # every row that can be in the list, tie groups whole
        out.append(sorted((d[r], ids[r]) for r in cand)[:k])
    return out


def _scan_vs_oracle(vecs, qs, k, expect_fallback=None, ids=None, mode=None):
    """ids=None: integer ids = row numbers, compared with the C oracle's (distance, row) lists.  ids given (the caller's
    strings, video_search_system.py:164-166): compared with the (distance, id) order built from the oracle's distances."""
    from video_quierer_amd.indexes.hnsw import MODE_FP16, OptimizedHNSWIndex
    idx = OptimizedHNSWIndex(dimension=vecs.shape[1])
    idx.add_batch(list(vecs), list(range(len(vecs))) if ids is None else list(ids))
    idx.search_mode = MODE_FP16 if mode is None else mode
    res = idx.search_batch(list(qs), k) if len(qs) != 1 else [idx.search(qs[0], k)]
    st = idx.last_search_stats()
    stored = idx._export()
    uq = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    if ids is not None:
        assert idx._tie_order == "device"
        want = _expected_in_id_order(stored, uq, ids, k)
        for j, (rr, ww) in enumerate(zip(res, want)):
            assert [r["id"] for r in rr] == [i for _, i in ww], f"query {j}: ids differ from the (distance, id) order (stats {st})"
            assert [r["distance"] for r in rr] == [d for d, _ in ww], f"query {j}: distances differ from the oracle (stats {st})"
    else:
        oid, od = knn_oracle.topk(stored, uq, k)
        got = np.array([[r["id"] for r in rr] + [-1] * (k - len(rr)) for rr in res], dtype=np.int32)
        d = np.array([[r["distance"] for r in rr] + [np.inf] * (k - len(rr)) for rr in res], dtype=np.float32)
        assert np.array_equal(got, oid), f"ids differ from the oracle (stats {st})"
        assert np.array_equal(d, od), f"distances differ from the oracle (stats {st})"
    assert st["verified"] + st["rescanned"] + st["exact_fallback"] == len(qs)
    idx.close()
    return st


def test_fp16_scan_random_matches_oracle_bit_exact(gpu_lib):
    rng = np.random.default_rng(31)
    vecs = rng.standard_normal((20001, 512)).astype(np.float32)       # ragged: 19.53 ranges of 1024
    qs = rng.standard_normal((130, 512)).astype(np.float32)           # ragged query tile
    st = _scan_vs_oracle(vecs, qs, 10)
    print("fp16 scan, random data:", st)
    assert st["exact_fallback"] <= 2                                   # random data: the proof closes almost always
    _scan_vs_oracle(vecs[:16500], qs[:17], 1)
    for k in (21, 32, 40, 64):                                         # the caller's k * 2 (video_search_system.py:297): wide candidate pool, MFMA-tile scan
        _scan_vs_oracle(vecs, qs, k)
    # dim % 128 != 0: the 128 x 1024 MFMA tile and key layout 1 (16.1 ranges of 1024, 1.02 query tiles of 128)
    vecs192 = rng.standard_normal((16500, 192)).astype(np.float32)
    qs192 = rng.standard_normal((130, 192)).astype(np.float32)
    for k in (10, 32):
        _scan_vs_oracle(vecs192, qs192, k)


@pytest.mark.parametrize("dim,n,nq,k", [(512, 20001, 130, 10), (512, 20001, 3, 10), (192, 16500, 130, 10)])
def test_search_runs_what_its_plan_says(gpu_lib, monkeypatch, dim, n, nq, k):
    """One profiled fp16 search: the scan, re-score and query-conversion brackets are the counts that follow from
    vq_debug_scan_plan's scalars (one scan and one re-score per chunk, no conversion where the streaming scan rounds the queries
    itself) for the batch scan, the fused streaming scan and the 128 x 1024 tile; the brackets change nothing in the answer."""
    import ctypes
    from video_quierer_amd.indexes.hnsw import MODE_FP16, OptimizedHNSWIndex
    for name in ("VQ_AMD_SCAN", "VQ_AMD_SCAN_SMALL", "VQ_AMD_SCAN_RB", "VQ_AMD_RESCORE_QPW4", "VQ_AMD_RESCORE_SMALL64"):
        monkeypatch.delenv(name, raising=False)
    plan = gpu_lib.ScanPlanC()
    assert gpu_lib.load().vq_debug_scan_plan(dim, n, nq, k, 0, ctypes.byref(plan)) == 0
    assert (plan.scan, plan.fused_q, plan.chunks) == ({130: 5 if dim == 512 else 1, 3: 3}[nq], int(nq == 3), 1)
    rng = np.random.default_rng(47)
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = OptimizedHNSWIndex(dimension=dim)
    try:
        idx.add_batch(list(vecs), list(range(n)))
        idx.search_mode = MODE_FP16
        plain = idx.search_batch(list(qs), k)
        idx.profile_begin()
        res = idx.search_batch(list(qs), k)
        prof = idx.profile_end()
    finally:
        idx.close()
    got = {name: prof[name]["launches"] for name in ("scan_f16_mfma_top2", "rescore_verify", "rows_to_f16")}
    assert got == {"scan_f16_mfma_top2": plan.chunks, "rescore_verify": plan.chunks, "rows_to_f16": 0 if plan.fused_q else plan.chunks}
    assert prof["scan_f16_mfma_top2"]["ms"] > 0.0 and prof["rescore_verify"]["ms"] > 0.0
    assert res == plain and all(len(r) == k for r in res)


def test_small_batch_streaming_scan_matches_oracle_bit_exact(gpu_lib):
    """Batches of <= 96 queries (the reference searches one query at a time, video_search_system.py:297) take the
    HBM-bound streaming scan (scan3_f16_top2_kernel, 16 or 32 queries per pass): same proof, same bit-exact answers."""
    rng = np.random.default_rng(41)
    vecs = rng.standard_normal((20001, 512)).astype(np.float32)       # ragged last stream (33 rows)
    qs = rng.standard_normal((96, 512)).astype(np.float32)
    for nq, k in ((1, 10), (1, 1), (1, 32), (5, 20), (16, 10), (17, 10), (32, 10), (33, 5), (64, 32), (96, 10), (1, 64), (40, 21), (3, 48)):   # > 16: two query groups per pass
        st = _scan_vs_oracle(vecs, qs[:nq], k)
        # (k > 20 on a 157-stream index: several of the best k rows share a 128-row stream, beyond the 4 stream rescans a query may
        #  ask for, so the exact fallback answers — still bit-exact; at 1M rows those proofs close: test_config3_full_size_properties)
        assert k > 20 or st["exact_fallback"] <= 1, (nq, k, st)
    _scan_vs_oracle(vecs[:16400, :256], qs[:3, :256], 5)                # dim 256 instantiation
    _scan_vs_oracle(vecs[:16400, :256], qs[:21, :256], 5)
    _scan_vs_oracle(vecs[:16400, :128], qs[:3, :128], 5)                # other dims keep the MFMA-tile scan
    wide = rng.standard_normal((16500, 768)).astype(np.float32)         # ViT-L/14's embedding width (configs[4]): one group of 16 per pass
    wq = rng.standard_normal((20, 768)).astype(np.float32)
    _scan_vs_oracle(wide, wq[:1], 10)
    _scan_vs_oracle(wide, wq, 10)
    # near-duplicate runs: stream rescans and the exact fallback behind the streaming scan
    centers = rng.standard_normal((200, 512)).astype(np.float32)
    dup = (np.repeat(centers, 100, axis=0) + 1e-3 * rng.standard_normal((20000, 512))).astype(np.float32)
    st = _scan_vs_oracle(dup, centers[:9] + 0, 10)
    print("streaming scan, clustered data:", st)


def test_small_batch_rescore_across_index_sizes(gpu_lib):
    """The single-query re-score pass picks its candidates through a per-wave threshold: the geometry changes with the number of
    128-row streams (< 35: every key is collected; < 512: streams interleaved over the waves; beyond: by thread id) and the
    candidates are re-scored in two passes (the best max(16, k+6) first).  Bit-exact against the oracle on every side of those."""
    rng = np.random.default_rng(43)
    vecs = rng.standard_normal((70000, 512)).astype(np.float32)
    qs = rng.standard_normal((33, 512)).astype(np.float32)
    for n in (1, 9, 100, 4300, 4500, 33000, 65500, 65700, 70000):      # 1 .. 547 streams
        for nq, k in ((1, 10), (7, 1), (33, 32), (2, 20)):
            st = _scan_vs_oracle(vecs[:n], qs[:nq], k)
            # (two keys per 128-row stream: an index of fewer than 64 k rows cannot offer k candidates, the exact fallback answers)
            assert k > 20 or n < 64 * k or st["exact_fallback"] <= 1, (n, nq, k, st)
    # exact ties across streams (every row appears 3 times): equal keys at the selection threshold and at the k-th place
    tied = np.concatenate([vecs[:3000]] * 3)
    _scan_vs_oracle(tied, qs[:3], 10)
    _scan_vs_oracle(tied, vecs[:2] + 0, 6)                                # the query IS a stored row: distance ~0 three times
    st = _scan_vs_oracle(tied, vecs[:1] + 0, 32)                          # ONE query whose proof cannot close (k = every candidate slot, ties):
    assert st["exact_fallback"] == 1, st                                  # its own workgroup files it for the exact fallback


def test_fp16_scan_clustered_and_degenerate_data_stay_exact(gpu_lib):
    rng = np.random.default_rng(32)
    # video-like: runs of 40 near-duplicate neighbours (adjacent rows), 1e-3 apart
    centers = rng.standard_normal((420, 256)).astype(np.float32)
    vecs = (np.repeat(centers, 40, axis=0) + 1e-3 * rng.standard_normal((16800, 256))).astype(np.float32)
    qs = centers[:48] + 1e-3 * rng.standard_normal((48, 256)).astype(np.float32)
    st = _scan_vs_oracle(vecs, qs, 10)
    print("fp16 scan, clustered data:", st)
    # exact duplicates everywhere: every distance ties, order is by row id; nothing can be proven -> exact fallback
    same = np.tile(rng.standard_normal((1, 128)).astype(np.float32), (16400, 1))
    st = _scan_vs_oracle(same, same[:3] + 0, 5)
    print("fp16 scan, all-identical rows:", st)
    assert st["exact_fallback"] == 3
    # the device-side fallback with many flagged queries: several groups of 8 per row split, both slot lanes, a ragged
    # last group, a ragged last row split, k = 32 (full lists) - every query through the exact fallback, bit-exact
    same = np.tile(rng.standard_normal((1, 128)).astype(np.float32), (18001, 1))
    same[::7] *= 1.0 + 1e-7 * rng.standard_normal((len(same[::7]), 1)).astype(np.float32)      # a few distinct distances among the ties
    st = _scan_vs_oracle(same, same[:301] + 0, 32)
    assert st["exact_fallback"] == 301
    st = _scan_vs_oracle(same[:16385], same[:70] + 0, 3)      # batch path (> 64 queries), 9 row splits of 2048 with a 1-row tail
    assert st["exact_fallback"] == 70


def test_tie_order_follows_the_callers_ids_on_every_search_path(gpu_lib):
    """hnsw.py:269 / :518 sort (distance, id) tuples, and the caller's ids are strings f"{video_id}_{i}"
    (video_search_system.py:164-166): duplicate frames come back in STRING order ("video0_10" before "video0_2"), which is
    not row order.  The device orders by (distance, rank of the id) itself (vq_index_set_id_ranks) — checked here on every
    path a search can take: the exact scan, the single-query / small-batch / MFMA-tile fp16 scans with their 32-, 80- and
    128-candidate re-score kernels, stream rescans, and the device-side exact fallback."""
    from video_quierer_amd.indexes.hnsw import MODE_EXACT, MODE_FP16
    from conftest import knn_big_ids
    rng = np.random.default_rng(47)
    base = rng.standard_normal((6000, 256)).astype(np.float32)
    tied = np.concatenate([base] * 3)                                   # every row three times, 6,000 rows apart
    ids = knn_big_ids(len(tied))                                        # "video0_0" ... "video3_4499"
    qs = np.concatenate([base[:200] + 0, rng.standard_normal((120, 256)).astype(np.float32)])
    for mode in (MODE_EXACT, MODE_FP16):
        for nq, k in ((1, 2), (1, 10), (1, 20), (1, 32), (5, 10), (33, 7), (33, 40), (97, 10), (320, 4), (130, 20), (130, 64), (100, 100)):
            _scan_vs_oracle(tied, qs[:nq], k, ids=ids, mode=mode)
    # tie groups larger than any candidate pool: nothing can be proven, the exact fallback orders by id rank too
    same = np.tile(rng.standard_normal((1, 128)).astype(np.float32), (16400, 1))
    same[::5] *= 1.0 + 1e-7 * rng.standard_normal((len(same[::5]), 1)).astype(np.float32)
    sids = knn_big_ids(len(same))
    for nq, k in ((1, 5), (3, 32), (70, 3), (301, 10)):
        st = _scan_vs_oracle(same, same[:nq] + 0, k, ids=sids, mode=MODE_FP16)
        assert st["exact_fallback"] == nq, st
    # integer ids that are not the row numbers (reversed): ties by the smaller INTEGER, i.e. the later row
    rev = list(range(len(tied) - 1, -1, -1))
    _scan_vs_oracle(tied, qs[:40], 10, ids=rev, mode=MODE_FP16)
    _scan_vs_oracle(tied, qs[:1], 10, ids=rev, mode=MODE_EXACT)


def test_id_ranks_c_abi_contract(gpu_lib):
    """vq_index_set_id_ranks through the C ABI: a non-permutation is refused, ranks go stale when rows are added (the next
    search fails loudly instead of ordering ties by garbage), n = 0 restores row order, vq_index_update_rows keeps them."""
    from ctypes import POINTER, byref, c_float, c_int32, c_int64, c_void_p
    lib = gpu_lib.load()
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((40, 64)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[30] = rows[7]                                                  # one tie
    h = c_void_p()
    gpu_lib.check(lib.vq_index_create(64, byref(h)))
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows), 40, 0))
    ids, dist = np.empty((1, 3), np.int32), np.empty((1, 3), np.float32)

    def search():
        return lib.vq_index_search(h, gpu_lib.fptr(rows[7:8].copy()), 1, 3, 0, ids.ctypes.data_as(POINTER(c_int32)), gpu_lib.fptr(dist))
    gpu_lib.check(search())
    assert list(ids[0, :2]) == [7, 30]                                  # row order
    rank = np.arange(40, dtype=np.int32)[::-1].copy()                   # reversed id order: row 30's id sorts first
    gpu_lib.check(lib.vq_index_set_id_ranks(h, rank.ctypes.data_as(POINTER(c_int32)), 40))
    gpu_lib.check(search())
    assert list(ids[0, :2]) == [30, 7] and dist[0, 0] == dist[0, 1]
    bad = rank.copy(); bad[3] = bad[4]
    assert lib.vq_index_set_id_ranks(h, bad.ctypes.data_as(POINTER(c_int32)), 40) < 0 and b"permutation" in lib.vq_last_error()
    assert lib.vq_index_set_id_ranks(h, rank.ctypes.data_as(POINTER(c_int32)), 39) < 0
    gpu_lib.check(search())                                             # a refused call leaves the old ranks in place
    assert list(ids[0, :2]) == [30, 7]
    rn = (c_int64 * 1)(12)
    gpu_lib.check(lib.vq_index_update_rows(h, gpu_lib.fptr(rows[5:6].copy()), rn, 1, 0))      # same ids: ranks stay valid
    gpu_lib.check(search())
    assert list(ids[0, :2]) == [30, 7]
    gpu_lib.check(lib.vq_index_add(h, gpu_lib.fptr(rows[:2].copy()), 2, 0))
    assert search() < 0 and b"id ranks" in lib.vq_last_error()          # stale: refused
    gpu_lib.check(lib.vq_index_set_id_ranks(h, None, 0))
    gpu_lib.check(search())
    assert list(ids[0, :2]) == [7, 30]                                  # back to row order
    gpu_lib.check(lib.vq_index_destroy(h))


@pytest.mark.timeout(240)
def test_search_fuzz_against_the_reference_order(gpu_lib):
    """scripts/fuzz_search.py for 20 s on a fixed seed (its long runs: 3,035 random cases / 104,723 result lists, all identical):
    index size, dimension, k, batch size, duplicate rows, id kind (row numbers / shuffled integers / the caller's strings) and
    search mode at random; every list equals `sorted((distance, id) ...)[:k]` over the C oracle's distances, bit for bit."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_search.py"), "20", "4"],
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all identical" in r.stdout


# ------------------------------------------------------------------ live system's brute-force index ("next" #2)
def test_simple_video_index_matches_the_real_class(gpu_lib, tmp_path):
    """tests/golden/simple_index.npz holds what the REAL SimpleVideoIndex (video_search_overhaul.py:23-64, lifted out
    of the reference source by make_golden.py) returns on these seeded rows: 100 un-normalised rows, two pairs of
    exact duplicates, queries scaled by 2.5.  Frame ids identical (ties included), scores within fp32 rounding."""
    from video_quierer_amd.overhaul_index import SimpleVideoIndex
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simple_index.npz"))
    rng = np.random.default_rng(77)
    emb = rng.standard_normal((300, 512)).astype(np.float32)
    emb[:200] /= np.linalg.norm(emb[:200], axis=1, keepdims=True)      # the last 100 rows stay un-normalised
    emb[250] = emb[230]
    emb[20] = emb[10]
    idx = SimpleVideoIndex()
    assert idx.search(emb[0], 3) == []
    for i, e in enumerate(emb):
        idx.add_frame(e, f"video_{i // 100}.mp4", i * 0.5)
    for k in (1, 5, 12):
        for row, qi in enumerate(gold["query_rows"]):
            got = idx.search(emb[qi] * np.float32(gold["query_scale"]), k)
            assert [g["frame_id"] for g in got] == list(gold[f"frame_id_k{k}"][row]), (k, qi)
            ref_sc = gold[f"score_k{k}"][row]
            assert np.abs(np.array([g["score"] for g in got]) - ref_sc).max() <= 4e-6 * max(1.0, np.abs(ref_sc).max())
            assert [g["timestamp"] for g in got] == list(gold[f"timestamp_k{k}"][row])
            assert sorted(got[0]) == list(gold["keys"]) and isinstance(got[0]["score"], float)
    # a cache file written by the real class loads here and answers like the real class did
    fresh = SimpleVideoIndex()
    assert fresh.load_from_disk(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_simple_index_cache.pkl"))
    assert fresh.video_hashes == {"clip_0.mp4": "abc", "clip_1.mp4": "def"} and len(fresh.embeddings) == 12
    assert [g["frame_id"] for g in fresh.search(emb[5], 3)] == list(gold["cache_frame_id_k3"])
    path = tmp_path / "cache.pkl"
    assert idx.save_to_disk(path)
    again = SimpleVideoIndex()
    assert again.load_from_disk(path) and not again.load_from_disk(tmp_path / "missing.pkl")
    assert [g["frame_id"] for g in again.search(emb[123], 5)] == [g["frame_id"] for g in idx.search(emb[123], 5)]
    with open(path, "rb") as f:
        assert sorted(pickle.load(f)) == ["embeddings", "metadata", "version", "video_hashes"]     # reference layout :68-73
    idx.add_frame(emb[123] * 3, "late.mp4", 1.0)                         # incremental add after a search
    assert idx.search(emb[123], 1)[0]["frame_id"] == 300


# ------------------------------------------------------------------ persistence interop (K10)
def _interop_vectors():
    rng = np.random.default_rng(11)                                      # make_golden.py interop_vectors()
    vecs = (rng.standard_normal((50, 64)) * 2.5).astype(np.float32)
    ids = [f"video{i // 25}_{i % 25}" for i in range(50)]
    qs = rng.standard_normal((8, 64)).astype(np.float32)
    return vecs, ids, qs


def test_index_loads_a_file_written_by_the_reference(gpu_lib):
    """tests/golden/ref_index_50.pkl(.sha256) was written by the REAL HNSWIndex.save (hnsw.py:306-339); the result
    lists next to it are what the real class returns after loading it (ef_search 50 >= N: exhaustive)."""
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    gold = np.load(os.path.join(gdir, "ref_index_50_results.npz"))
    vecs, ids, qs = _interop_vectors()
    idx = HNSWIndex(dimension=512)                                       # load() adopts the file's dimension (64)
    idx.load(os.path.join(gdir, "ref_index_50.pkl"))
    assert idx.dimension == 64 and idx.size() == 50 and idx.M == 16 and idx.ef_search == 50
    assert idx.entry_point in ids and set(idx.data) == set(ids)
    view = idx.data                                                     # hnsw.py:44 `self.data`: a read-only view of the device matrix
    assert len(view) == len(ids) and ids[3] in view and "no such id" not in view
    assert np.array_equal(view[ids[3]], idx._export()[3]) and np.array_equal(dict(view.items())[ids[0]], idx._export()[0])
    with pytest.raises(KeyError):
        view["no such id"]
    for i, q in enumerate(qs):
        res = idx.search(q, 5)
        assert [r["id"] for r in res] == list(gold["ids"][i])
        assert np.abs(np.array([r["distance"] for r in res]) - gold["dist"][i]).max() <= 3e-7
        assert np.abs(np.array([r["score"] for r in res]) - gold["score"][i]).max() <= 3e-7
    assert [[r["id"] for r in rr] for rr in idx.search_batch(list(qs), 5)] == [list(r) for r in gold["ids"]]
    idx.close()


def test_index_save_writes_the_reference_layout(gpu_lib, tmp_path):
    """The other direction: the file this build writes.  tests/test_oracle_golden.py loads the committed copy
    (tests/golden/build_index_50.pkl, written by this test with VQ_WRITE_FIXTURES=1 on the GPU box) with the REAL
    class in the build container."""
    from video_quierer_amd.indexes.hnsw import HNSWIndex
    vecs, ids, qs = _interop_vectors()
    idx = HNSWIndex(dimension=64)
    idx.add_batch(list(vecs), ids)
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out") \
        if os.environ.get("VQ_WRITE_FIXTURES") == "1" else str(tmp_path)
    path = os.path.join(out_dir, "build_index_50.pkl")
    idx.save(path)
    with open(path, "rb") as f:
        s = pickle.load(f)
    assert {"dimension", "M", "max_M", "ef_construction", "ef_search", "level_generation_factor", "data", "levels",
            "graph", "entry_point", "element_count"} <= set(s)                # hnsw.py:311-324
    stored = np.stack([s["data"][i] for i in ids])
    assert np.array_equal(stored, np.stack([v / np.linalg.norm(v) for v in vecs]).astype(np.float32))   # hnsw.py:157
    idx.close()


# ------------------------------------------------------------------ native exchange (vq_comm, RCCL)
def _device_search(idx, q_t, k):
    ids = torch.empty((q_t.shape[0], k), dtype=torch.int32, device="cuda")
    dd = torch.empty((q_t.shape[0], k), dtype=torch.float32, device="cuda")
    idx.search_device(q_t.data_ptr(), q_t.shape[0], k, ids.data_ptr(), dd.data_ptr())
    idx.synchronize()
    return ids, dd


def test_merge_of_two_row_shards_on_one_device_is_the_single_index_answer(gpu_lib):
    """The search exchange without the wire: two indexes hold the two row shards of one matrix (ragged split, an exact
    tie across the boundary, a shard smaller than k), their device results get global ids and go through the
    library's merge kernel (vq_merge_topk_device) — bit-identical to the oracle on the whole matrix."""
    from video_quierer_amd.comm import merge_topk_device
    rng = np.random.default_rng(100)
    n, nq, k, d = 1003, 37, 10, 64
    rows = knn_oracle.normalize_rows(rng.standard_normal((n, d)).astype(np.float32))
    rows[700] = rows[3]                                  # an exact tie across the shard boundary
    qs = knn_oracle.normalize_rows(rng.standard_normal((nq, d)).astype(np.float32))
    qs[0] = rows[3]
    q_t = torch.from_numpy(qs).cuda()
    for cut in (502, 998):                               # second split: shard 1 has 5 rows < k -> -1 / +inf padding
        parts, stored = [], []
        for lo, hi in ((0, cut), (cut, n)):
            idx = _mk_index(rows[lo:hi])
            stored.append(idx._export())                 # add_batch re-normalises with numpy (hnsw.py:157)
            ids, dd = _device_search(idx, q_t, k)
            parts.append((torch.where(ids >= 0, ids + lo, ids), dd))
            idx.close()
        oid, od = knn_oracle.topk(np.concatenate(stored), qs, k)
        all_ids = torch.stack([p[0] for p in parts]).contiguous()
        all_d = torch.stack([p[1] for p in parts]).contiguous()
        out_ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        out_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        merge_topk_device(all_ids.data_ptr(), all_d.data_ptr(), 2, nq, k, out_ids.data_ptr(), out_d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out_ids.cpu().numpy(), oid) and np.array_equal(out_d.cpu().numpy(), od)
        assert list(out_ids[0, :2].cpu().numpy()) == [3, 700]


def test_sharded_search_at_the_scale_config_geometry(gpu_lib):
    """configs[4]'s index geometry on one device at reduced size: 768-d rows (ViT-L/14 embeddings), two row shards large
    enough for the fp16 MFMA scan (>= 16,384 rows each), a 300-query batch and a single query, merged by the library's
    merge kernel — ids and distances bit-identical to the exact oracle over the whole matrix."""
    from video_quierer_amd.comm import merge_topk_device
    rng = np.random.default_rng(768)
    n, d, k = 34000, 768, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[20000] = rows[5]                                 # a tie across the shard boundary
    qs = rng.standard_normal((300, d)).astype(np.float32)
    qs[0] = rows[5]
    shards, stored = [], []
    for lo, hi in ((0, 17000), (17000, n)):
        idx = _mk_index(rows[lo:hi])
        stored.append(idx._export())
        shards.append((lo, idx))
    uq = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    oid, od = knn_oracle.topk(np.concatenate(stored), uq, k)
    for nq in (300, 1):
        q_t = torch.from_numpy(uq[:nq]).cuda()
        parts = []
        for lo, idx in shards:
            ids, dd = _device_search(idx, q_t, k)
            parts.append((torch.where(ids >= 0, ids + lo, ids), dd))
        all_ids = torch.stack([p[0] for p in parts]).contiguous()
        all_d = torch.stack([p[1] for p in parts]).contiguous()
        out_ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        out_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        merge_topk_device(all_ids.data_ptr(), all_d.data_ptr(), 2, nq, k, out_ids.data_ptr(), out_d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out_ids.cpu().numpy(), oid[:nq]) and np.array_equal(out_d.cpu().numpy(), od[:nq])
    assert list(oid[0, :2]) == [5, 20000]
    for _, idx in shards:
        idx.close()


@pytest.mark.timeout(180)
def test_native_comm_world_of_one_over_rccl(gpu_lib):
    """vq_comm_* with a real RCCL communicator of one rank (all a one-GPU box can hold): the all-gather of rows is the
    identity and the sharded search returns the single-index answer with global ids.  What ONE rank cannot reach: the ragged
    branch of vq_allgather_rows (pad, gather, compact — counts differ only between ranks) and ncclCommInitRank across processes;
    RCCL refuses two ranks on one device, so those first run on the driver's multi-GPU node (bench.py gives that bring-up a
    deadline and a torch-exchange relaunch)."""
    from video_quierer_amd.comm import Comm
    import socket
    import torch.distributed as dist
    # the bootstrap bench.py uses: rank 0's unique id travels through torch.distributed's store
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        comm = Comm.from_torch_distributed()
    finally:
        dist.destroy_process_group()
    assert comm.world == 1 and comm.rank == 0 and comm.rccl_version() > 0
    rng = np.random.default_rng(5)
    local = torch.from_numpy(rng.standard_normal((300, 512)).astype(np.float32)).cuda()
    out = torch.zeros_like(local)
    st = torch.cuda.current_stream().cuda_stream
    comm.all_gather_rows(local.data_ptr(), [300], 512, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(out, local)
    rows = knn_oracle.normalize_rows(rng.standard_normal((20000, 512)).astype(np.float32))     # fp16 scan path
    qs = knn_oracle.normalize_rows(rng.standard_normal((33, 512)).astype(np.float32))
    idx = _mk_index(rows)
    q_t = torch.from_numpy(qs).cuda()
    ids = torch.empty((33, 10), dtype=torch.int32, device="cuda")
    dd = torch.empty((33, 10), dtype=torch.float32, device="cuda")
    comm.search_sharded(idx, q_t.data_ptr(), 33, 10, 1_000_000, ids.data_ptr(), dd.data_ptr())
    idx.synchronize()
    oid, od = knn_oracle.topk(idx._export(), qs, 10)
    assert np.array_equal(ids.cpu().numpy(), oid + 1_000_000) and np.array_equal(dd.cpu().numpy(), od)
    comm.check()                                                           # nothing was voided

    # ---- a rank whose LOCAL scan fails still enters the exchange: here the shard refuses the fp16 mode
    # (rows stored un-normalised at 3x unit length).  The failing rank gets its error, the merge sees its status word:
    # every list comes back empty and the communicator is flagged — then it keeps working.
    from video_quierer_amd.indexes.hnsw import MODE_FP16, OptimizedHNSWIndex
    bad = OptimizedHNSWIndex(dimension=512)
    big = np.ascontiguousarray(rows[:2000] * np.float32(3.0))
    bad._append_stored(big, range(2000))
    ids.fill_(7); dd.fill_(7.0)
    with pytest.raises(ValueError, match="fp16 scan needs"):
        comm.search_sharded(bad, q_t.data_ptr(), 33, 10, 0, ids.data_ptr(), dd.data_ptr(), mode=MODE_FP16)
    bad.synchronize()
    assert bool((ids == -1).all()) and bool(torch.isinf(dd).all())        # visibly empty, not silently partial
    with pytest.raises(gpu_lib.VqError, match="voided.*rank 0"):
        comm.check()
    comm.check()                                                           # reported once
    comm.search_sharded(idx, q_t.data_ptr(), 33, 10, 0, ids.data_ptr(), dd.data_ptr())
    idx.synchronize()
    assert np.array_equal(ids.cpu().numpy(), oid) and np.array_equal(dd.cpu().numpy(), od)
    comm.check()
    bad.close()

    # ---- the ragged all-gather's compaction on a synthetic padded buffer (counts differ only BETWEEN ranks, so one rank never
    # reaches it through vq_allgather_rows): 4 "ranks", 9 rows of padding each, counts 9 / 0 / 4 / 1
    from ctypes import c_int64, c_void_p
    counts = [9, 0, 4, 1]
    padded = torch.from_numpy(rng.standard_normal((4, 9, 512)).astype(np.float32)).cuda()
    outc = torch.full((sum(counts), 512), float("nan"), device="cuda")
    gpu_lib.check(gpu_lib.load().vq_compact_gathered_rows(c_void_p(padded.data_ptr()), (c_int64 * 4)(*counts), 4, 9, 512,
                                                          c_void_p(outc.data_ptr()), c_void_p(st)))
    torch.cuda.synchronize()
    assert torch.equal(outc, torch.cat([padded[r, :c] for r, c in enumerate(counts)]))
    assert gpu_lib.load().vq_compact_gathered_rows(c_void_p(padded.data_ptr()), (c_int64 * 4)(9, 10, 0, 0), 4, 9, 512,
                                                   c_void_p(outc.data_ptr()), c_void_p(st)) < 0             # a count above the padding
    idx.close()
    comm.close()


@pytest.mark.timeout(180)
def test_native_comm_scratch_allocation_failure_is_agreed_before_the_collective(gpu_lib, monkeypatch):
    """A call that outgrows the exchange scratch allocates and then exchanges one status word per rank (agree()): with an
    allocation failure injected ($VQ_COMM_FAIL_ALLOC) the call returns an error BEFORE the data collective — on a real
    node every rank would, instead of the healthy ranks waiting in ncclAllGather for the one that left — and the next call
    (allocation succeeds) runs normally."""
    from video_quierer_amd.comm import Comm
    monkeypatch.setenv("VQ_COMM_FAIL_ALLOC", "1")
    comm = Comm.single()
    monkeypatch.delenv("VQ_COMM_FAIL_ALLOC")
    rng = np.random.default_rng(6)
    rows = knn_oracle.normalize_rows(rng.standard_normal((3000, 128)).astype(np.float32))
    qs = knn_oracle.normalize_rows(rng.standard_normal((5, 128)).astype(np.float32))
    idx = _mk_index(rows)
    q_t = torch.from_numpy(qs).cuda()
    ids = torch.empty((5, 4), dtype=torch.int32, device="cuda")
    dd = torch.empty((5, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(gpu_lib.VqError, match="scratch hipMalloc"):
        comm.search_sharded(idx, q_t.data_ptr(), 5, 4, 0, ids.data_ptr(), dd.data_ptr())
    comm.search_sharded(idx, q_t.data_ptr(), 5, 4, 0, ids.data_ptr(), dd.data_ptr())
    idx.synchronize()
    oid, od = knn_oracle.topk(idx._export(), qs, 4)
    assert np.array_equal(ids.cpu().numpy(), oid) and np.array_equal(dd.cpu().numpy(), od)
    comm.check()
    idx.close()
    comm.close()


# ------------------------------------------------------------------ the real-checkpoint door
def test_feature_extractor_from_a_local_checkpoint_directory(gpu_lib, tmp_path):
    """FeatureExtractor(model_name=<local HF directory>) (reference :76-81 from_pretrained): embeddings bit-identical
    to the seeded model carrying the same tensors; extract_text_features runs the checkpoint's own tokenizer
    (reference :218-234) and equals the ids path and the fp32 oracle."""
    from conftest import toy_text_config, write_checkpoint_dir
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    from video_quierer_amd.weights import seeded_text_weights
    d = write_checkpoint_dir(str(tmp_path / "clip-vit-base-patch32"))
    fx = FeatureExtractor(model_name=d, batch_size=8, device_batch=8)
    ref = FeatureExtractor(model_name="seed:1234", batch_size=8, device_batch=8)
    frames = list(synth_frames(8, seed=17))
    assert fx.output_dim == 512 and fx.model_name == d
    assert np.array_equal(fx.extract_batch(frames), ref.extract_batch(frames))
    t = fx.extract_text_features("the cat")
    assert t.shape == (512,) and t.dtype == np.float32 and abs(float(np.linalg.norm(t)) - 1.0) < 1e-5
    ids = np.array([[518, 517, 513, 519]])
    assert np.array_equal(t, fx.extract_text_features_from_ids(ids[0]))
    want = clip_vit_oracle.encode_token_ids(ids, seeded_text_weights(toy_text_config(), 1234), eos_token_id=519)[0]
    assert float(np.dot(t, want)) >= 1.0 - 1e-4
    assert float(np.dot(fx.extract_text_features("a dog sat"), t)) < 0.999        # a different prompt, a different vector
    fx.thread_pool.shutdown(); ref.thread_pool.shutdown()


# ------------------------------------------------------------------ threading / wrappers / odd sizes
def test_handles_are_thread_safe(gpu_lib, b32_weights):
    """extract_batch runs from asyncio executor threads and search from a 4-thread pool in the reference
    (feature_extractor.py:215-216, hnsw.py:291-294): concurrent calls on ONE handle must equal serial calls."""
    from concurrent.futures import ThreadPoolExecutor
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    fx = FeatureExtractor(model_name="seed:1234", batch_size=8, device_batch=16)
    frames = synth_frames(48, seed=5)
    serial = [fx.extract_batch(list(frames[i:i + 8])) for i in range(0, 48, 8)]
    with ThreadPoolExecutor(4) as pool:
        par = list(pool.map(lambda i: fx.extract_batch(list(frames[i:i + 8])), range(0, 48, 8)))
    for a, b in zip(serial, par):
        assert np.array_equal(a, b)
    vecs = np.random.default_rng(3).standard_normal((3000, 512)).astype(np.float32)
    idx = _mk_index(vecs)
    qs = list(np.concatenate(serial))
    want = idx.search_batch(qs, 7)
    with ThreadPoolExecutor(4) as pool:
        got = list(pool.map(lambda q: idx.search(q, 7), qs))
    assert [[r["id"] for r in rr] for rr in got] == [[r["id"] for r in rr] for rr in want]
    fx.thread_pool.shutdown(); idx.thread_pool.shutdown()


def test_async_wrappers_over_the_dropin(gpu_lib):
    import asyncio
    from video_quierer_amd.core.feature_extractor import BatchProcessor, CachedFeatureExtractor
    fx = CachedFeatureExtractor(model_name="seed:1234", batch_size=4, device_batch=8, cache_size=2)
    frames = synth_frames(6, seed=8)
    direct = fx.extract_batch(list(frames))

    async def run():
        bp = BatchProcessor(fx, timeout_ms=5)
        outs = await asyncio.gather(*[bp.process_request(f"r{i}", [frames[i]]) for i in range(6)])
        batch = await fx.extract_batch_async(list(frames[:3]))
        return outs, batch
    outs, batch = asyncio.run(run())
    for i, o in enumerate(outs):
        assert o.shape == (512,) and float(np.dot(o, direct[i])) > 1 - 1e-4
    assert np.allclose(batch, direct[:3], atol=2e-3)
    a = fx.extract_features(frames[0]); b = fx.extract_features(frames[0])
    assert np.array_equal(a, b) and fx.get_cache_stats()["cache_hits"] == 1
    fx.extract_features(frames[1]); fx.extract_features(frames[2])          # evicts (cache_size=2)
    assert fx.get_cache_stats()["cache_size"] == 2


def test_search_large_k_and_tiny_batches(gpu_lib, b32_weights):
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.indexes.hnsw import MODE_FP16
    from video_quierer_amd.weights import VIT_B_32
    rng = np.random.default_rng(41)
    vecs = rng.standard_normal((17000, 512)).astype(np.float32)
    idx = _mk_index(vecs)                                        # auto mode: > 16384 rows -> fp16 scan when k <= 100
    qs = rng.standard_normal((5, 512)).astype(np.float32)
    stored = idx._export()
    uq = np.stack([q / np.linalg.norm(q) for q in qs]).astype(np.float32)
    for k in (33, 64, 65, 100, 101, 150):                        # up to 100 (the API's k <= 50, doubled by the caller): the fp16 scans' wide pools; beyond -> exact scan
        res = idx.search_batch(list(qs), k)
        oid, od = knn_oracle.topk(stored, uq, k)
        assert np.array_equal(np.array([[r["id"] for r in rr] for rr in res]), oid)
        assert np.array_equal(np.array([[r["distance"] for r in rr] for rr in res], dtype=np.float32), od)
        st = idx.last_search_stats()
        assert k <= 100 or st["exact_fallback"] == 5, (k, st)     # beyond 100: the exact scan answers every query
    idx.search_mode = MODE_FP16
    assert len(idx.search(qs[0], 64)) == 64 and len(idx.search(qs[0], 100)) == 100
    with pytest.raises(ValueError):
        idx.search(qs[0], 101)
    enc = VitEncoder(VIT_B_32, b32_weights, max_batch=1)        # smallest workspace, one frame at a time
    f = synth_frames(3, seed=2)
    one_by_one = enc.encode(f)
    ref = clip_vit_oracle.encode_frames(f, b32_weights, batch_size=1)
    assert np.sum(one_by_one * ref, axis=1).min() >= 1 - COS_TOL
    enc.close()


def test_bench_config4_workload_on_one_gpu(gpu_lib):
    """`bench.py --workload config4` = configs[3] end to end (4 x 1000 frames -> encode -> [all-gather] -> index under string ids ->
    1,000 queries, k = 10) as the driver would type it for one GPU: one JSON line, every query finds its source frame first."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "config4", "--steps", "1", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["config"]["frames_per_rank"] == [4000] and out["config"]["queries_per_rank"] == 1000
    assert out["value"] > 0 and out["queries_per_s"] > 0 and out["last_job"]["top1_is_source_frame"] >= 0.99


# ------------------------------------------------------------------ other geometries (streaming attention, patch 14)
def test_encoder_small_patch14_geometry_vs_oracle(gpu_lib):
    """65 tokens (> one attention tile), patch 14 (generic patch extraction, K padded 588 -> 640), 2 blocks."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VitConfig, seeded_weights
    cfg = VitConfig(image_size=112, patch_size=14, hidden=768, mlp=3072, layers=2, heads=12, proj_dim=512)
    W = seeded_weights(cfg, 77)
    frames = np.random.default_rng(9).integers(0, 255, (5, 112, 112, 3), dtype=np.uint8)
    ref = clip_vit_oracle.encode_frames(frames, W, patch=14, heads=12, layers=2, batch_size=5)
    for dt, tol in (("bf16", 5e-3), ("fp16", 8e-4)):
        enc = VitEncoder(cfg, W, max_batch=8, compute_dtype=dt)
        emb = enc.encode(frames)
        enc.close()
        err = np.linalg.norm(emb - ref, axis=1).max()
        assert err <= tol, (dt, err)


def test_encoder_patch16_geometry_both_attention_forms(gpu_lib, monkeypatch):
    """197 tokens (224 / 16, squared, + CLS) = three full 64-key steps and one of five keys, seven 32-row query tiles (the last
    with five rows): the streaming attention's 32-rows-per-wave form (default; masking compiled into the peeled last key step,
    permlane-swap reductions) and the 64-row form ($VQ_AMD_ATTN=q64) against the fp32 oracle, and against each other."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VitConfig, seeded_weights
    cfg = VitConfig(image_size=224, patch_size=16, hidden=768, mlp=3072, layers=2, heads=12, proj_dim=512)
    W = seeded_weights(cfg, 78)
    frames = np.random.default_rng(10).integers(0, 255, (6, 224, 224, 3), dtype=np.uint8)
    ref = clip_vit_oracle.encode_frames(frames, W, patch=16, heads=12, layers=2, batch_size=6)
    out = {}
    for form in ("q32", "q64"):
        monkeypatch.setenv("VQ_AMD_ATTN", form)
        enc = VitEncoder(cfg, W, max_batch=8, compute_dtype="fp16")
        out[form] = enc.encode(frames)
        enc.close()
        assert np.linalg.norm(out[form] - ref, axis=1).max() <= 8e-4, form
    assert np.abs(out["q32"] - out["q64"]).max() <= 2e-4        # same arithmetic per row; only the online softmax's tile walk is shared


def test_encoder_vit_l14_336_matches_golden(gpu_lib):
    """BASELINE configs[4] model: ViT-L/14@336, fp16 operands as that config names (and bf16)."""
    from conftest import GOLDEN, FRAME_SEED
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_L_14_336, seeded_weights
    g = np.load(os.path.join(GOLDEN, "encoder_l14_336_seed1234.npz"))
    frames = np.random.default_rng(FRAME_SEED).integers(0, 255, (32, 336, 336, 3), dtype=np.uint8)      # one bench-sized batch (--model l14 --batch 32)
    W = seeded_weights(VIT_L_14_336, 1234)
    for dt, tol in (("fp16", 2e-3), ("bf16", 1.5e-2)):
        enc = VitEncoder(VIT_L_14_336, W, max_batch=32, compute_dtype=dt)
        emb = enc.encode(frames)
        enc.close()
        assert emb.shape == (32, 768)
        err = np.linalg.norm(emb - g["embeddings"], axis=1).max()
        cos = np.sum(emb * g["embeddings"], axis=1).min()
        print(f"ViT-L/14@336 {dt}: max L2 err {err:.2e}, min cos {cos:.7f}")
        assert err <= tol and cos >= 1 - COS_TOL


# ------------------------------------------------------------------ text tower ("next" #1)
def test_text_tower_matches_golden(gpu_lib):
    """16 synthetic prompts (token ids) vs transformers' get_text_features on the same seeded weights."""
    from video_quierer_amd.text_encoder import TextEncoder
    from video_quierer_amd.weights import TEXT_B_32, seeded_text_weights
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "text_b32_seed1234.npz"))
    W = seeded_text_weights(TEXT_B_32, 1234)
    for dt, tol in (("bf16", 8e-3), ("fp16", 1.2e-3)):
        enc = TextEncoder(TEXT_B_32, W, max_batch=8, compute_dtype=dt)      # 16 prompts -> two device passes
        emb = enc.encode_ids(g["input_ids"])
        short = enc.encode_ids(g["input_ids"][1:2, :3])                      # a 3-token prompt given un-padded
        enc.close()
        err = np.linalg.norm(emb - g["embeddings"], axis=1)
        print(f"text tower {dt}: max L2 err {err.max():.2e}, min cos {np.sum(emb * g['embeddings'], axis=1).min():.7f}")
        assert err.max() <= tol and np.sum(emb * g["embeddings"], axis=1).min() >= 1 - COS_TOL
        assert np.abs(short[0] - emb[1]).max() <= 1e-6                        # padding is invisible to the EOS position
    ref = clip_vit_oracle.encode_token_ids(g["input_ids"], W)
    assert np.abs(ref - g["embeddings"]).max() <= 1e-5


def test_text_tower_l14_matches_golden(gpu_lib):
    """configs[4]'s "mixed text+image queries": the ViT-L/14 text tower (768 wide, 12 heads, projection 768) on the 16 synthetic
    prompts against transformers' get_text_features on the same seeded weights (tests/golden/text_l14_seed1234.npz)."""
    from video_quierer_amd.text_encoder import TextEncoder
    from video_quierer_amd.weights import TEXT_L_14, seeded_text_weights
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "text_l14_seed1234.npz"))
    W = seeded_text_weights(TEXT_L_14, 1234)
    enc = TextEncoder(TEXT_L_14, W, max_batch=16, compute_dtype="fp16")
    emb = enc.encode_ids(g["input_ids"])
    enc.close()
    err = np.linalg.norm(emb - g["embeddings"], axis=1)
    print(f"ViT-L/14 text tower fp16: max L2 err {err.max():.2e}, min cos {np.sum(emb * g['embeddings'], axis=1).min():.7f}")
    assert emb.shape == (16, 768) and err.max() <= 1.5e-3 and np.sum(emb * g["embeddings"], axis=1).min() >= 1 - COS_TOL


def test_feature_extractor_text_ids(gpu_lib):
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    fx = FeatureExtractor(model_name="seed:1234", batch_size=8, device_batch=8)
    ids = np.array([49406, 320, 1125, 539, 320, 2368, 49407])               # "a photo of a cat"-shaped prompt
    v = fx.extract_text_features_from_ids(ids)
    assert v.shape == (512,) and v.dtype == np.float32 and abs(np.linalg.norm(v) - 1) < 1e-5
    both = fx.extract_text_features_from_ids(np.stack([ids, ids[::-1].copy()]))
    assert both.shape == (2, 512) and np.allclose(both[0], v, atol=1e-6)
    fx.thread_pool.shutdown()


# ------------------------------------------------------------------ BASELINE full sizes through size-independent properties
def test_config3_full_size_properties(gpu_lib):
    """configs[2]: 1,000,000 x 512 matrix.  (a) self-queries return their own row first at distance ~0, (b) lists are
    sorted by (distance, id), (c) the fp16-scan result is bit-identical to the independent exact fp32-master scan on a
    query subset, (d) every query is accounted for by the proof statistics, (e) 64 queries x k = 10 are bit-exact
    against the C oracle over the exported 1M rows on every scan path (one query, 33, 64, the 256-query MFMA tile)."""
    import torch
    from video_quierer_amd.indexes.hnsw import MODE_EXACT, MODE_FP16, OptimizedHNSWIndex
    n, d = 1_000_000, 512
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(123)
    idx = OptimizedHNSWIndex(dimension=d)
    for c0 in range(0, n, 250_000):
        blk = torch.randn((250_000, d), device=dev, generator=g)
        torch.cuda.synchronize()
        idx.add_device(blk.data_ptr(), 250_000, range(c0, c0 + 250_000), normalize=True)
        idx.synchronize()
    assert idx.size() == n
    probe = torch.randn((64, d), device=dev, generator=g)
    probe = probe / probe.norm(dim=1, keepdim=True)
    ids16 = torch.empty((64, 10), dtype=torch.int32, device=dev); d16 = torch.empty((64, 10), device=dev)
    idsx = torch.empty((64, 10), dtype=torch.int32, device=dev); dx = torch.empty((64, 10), device=dev)
    torch.cuda.synchronize()
    idx.search_device(probe.data_ptr(), 64, 10, ids16.data_ptr(), d16.data_ptr(), mode=MODE_FP16); idx.synchronize()
    st = idx.last_search_stats()
    idx.search_device(probe.data_ptr(), 64, 10, idsx.data_ptr(), dx.data_ptr(), mode=MODE_EXACT); idx.synchronize()
    assert torch.equal(ids16, idsx) and torch.equal(d16, dx)                  # (c) two independent code paths, same bits
    assert st["verified"] + st["rescanned"] + st["exact_fallback"] == 64      # (d)
    dd = d16.cpu().numpy(); ii = ids16.cpu().numpy()
    assert np.all(np.diff(dd, axis=1) >= 0) and np.all((ii >= 0) & (ii < n))  # (b)
    # (c) again on every scan path: one query (the reference's call pattern), 33 (two query groups per pass of the
    # streaming scan), 300 (the 256-query MFMA tile, ragged second tile)
    more = torch.randn((300, d), device=dev, generator=g)
    more = more / more.norm(dim=1, keepdim=True)
    for nq in (1, 33, 300):
        a_i = torch.empty((nq, 10), dtype=torch.int32, device=dev); a_d = torch.empty((nq, 10), device=dev)
        b_i = torch.empty((nq, 10), dtype=torch.int32, device=dev); b_d = torch.empty((nq, 10), device=dev)
        idx.search_device(more.data_ptr(), nq, 10, a_i.data_ptr(), a_d.data_ptr(), mode=MODE_FP16); idx.synchronize()
        st = idx.last_search_stats()
        idx.search_device(more.data_ptr(), nq, 10, b_i.data_ptr(), b_d.data_ptr(), mode=MODE_EXACT); idx.synchronize()
        assert torch.equal(a_i, b_i) and torch.equal(a_d, b_d), nq
        assert st["verified"] + st["rescanned"] + st["exact_fallback"] == nq and st["exact_fallback"] <= 1, (nq, st)
    # HIP vs the C oracle at FULL size (the comparisons above are between two HIP paths that share the row
    # normalisation, the fp32 master and the addressing): the matrix exported once, 64 queries x k = 10 through
    # oracle/knn_oracle.c (fp64-chain dot, seconds on the box's cores), bit-exact ids and distances on each scan path
    host_rows = idx._export()
    assert host_rows.shape == (n, d)
    more_h = more[:64].cpu().numpy()
    oid, od = knn_oracle.topk(host_rows, more_h, 10)
    for nq in (1, 33, 64):
        a_i = torch.empty((nq, 10), dtype=torch.int32, device=dev); a_d = torch.empty((nq, 10), device=dev)
        idx.search_device(more.data_ptr(), nq, 10, a_i.data_ptr(), a_d.data_ptr(), mode=MODE_FP16); idx.synchronize()
        assert np.array_equal(a_i.cpu().numpy(), oid[:nq]) and np.array_equal(a_d.cpu().numpy(), od[:nq]), nq
    a_i = torch.empty((300, 10), dtype=torch.int32, device=dev); a_d = torch.empty((300, 10), device=dev)
    idx.search_device(more.data_ptr(), 300, 10, a_i.data_ptr(), a_d.data_ptr(), mode=MODE_FP16); idx.synchronize()      # the MFMA-tile scan
    assert np.array_equal(a_i.cpu().numpy()[:64], oid) and np.array_equal(a_d.cpu().numpy()[:64], od)
    # ... and the rows the device normalised are the oracle's normalisation of the same raw rows (first block)
    g0 = torch.Generator(device=dev); g0.manual_seed(123)
    raw = torch.randn((250_000, d), device=dev, generator=g0)[:4096].cpu().numpy()
    assert np.array_equal(host_rows[:4096], knn_oracle.normalize_rows(raw))
    del host_rows
    # the caller's over-fetch (k * 2, video_search_system.py:297) for user k up to 32: k in (20, 64] stays on the fp16 scans
    # (80- / 128-candidate re-score pools up to k = 100: the API's k <= 50) and closes its proofs at this size
    for nq, k in ((1, 20), (1, 32), (1, 64), (33, 24), (300, 32), (300, 64), (1, 100), (300, 100)):
        a_i = torch.empty((nq, k), dtype=torch.int32, device=dev); a_d = torch.empty((nq, k), device=dev)
        b_i = torch.empty((nq, k), dtype=torch.int32, device=dev); b_d = torch.empty((nq, k), device=dev)
        idx.search_device(more.data_ptr(), nq, k, a_i.data_ptr(), a_d.data_ptr(), mode=MODE_FP16); idx.synchronize()
        st = idx.last_search_stats()
        idx.search_device(more.data_ptr(), nq, k, b_i.data_ptr(), b_d.data_ptr(), mode=MODE_EXACT); idx.synchronize()
        assert torch.equal(a_i, b_i) and torch.equal(a_d, b_d), (nq, k)
        assert st["verified"] + st["rescanned"] + st["exact_fallback"] == nq and st["exact_fallback"] <= max(1, nq // 100), (nq, k, st)
    # (a) self-queries.  The first rows of the big index are reproduced bit for bit in a small second index
    # (same generator seed -> identical first block, same device normalisation) and exported from there.
    small = OptimizedHNSWIndex(dimension=d)
    g2 = torch.Generator(device=dev); g2.manual_seed(123)
    blk = torch.randn((250_000, d), device=dev, generator=g2)               # same stream -> identical first block
    torch.cuda.synchronize()
    small.add_device(blk.data_ptr(), 4096, range(4096), normalize=True); small.synchronize()
    first = small._export()                                                   # rows 0..4095 of the big index, bit for bit
    res = idx.search_batch(list(first[:256]), 3)
    assert [r[0]["id"] for r in res] == list(range(256))
    assert max(abs(float(r[0]["distance"])) for r in res) <= 1e-6
    idx.close(); small.close()


def test_config2_batching_invariance(gpu_lib, b32_weights):
    """configs[1]: embeddings must not depend on how frames are grouped into device passes: 1,000 frames in
    passes of 256 vs passes of 100 give identical bits (each output row is the same MFMA/K sequence whatever
    tile it lands in), and the run is deterministic."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    frames = synth_frames(1000, seed=77)
    a = VitEncoder(VIT_B_32, b32_weights, max_batch=256)
    b = VitEncoder(VIT_B_32, b32_weights, max_batch=100)
    ea, eb = a.encode(frames), b.encode(frames)
    assert np.array_equal(ea, a.encode(frames))
    assert np.array_equal(ea, eb)
    assert np.allclose(np.linalg.norm(ea, axis=1), 1.0, atol=1e-5)
    a.close(); b.close()


def test_config2_full_size_50k_frames(gpu_lib, b32_weights):
    """configs[1] at its full size: 50,000 device-resident frames in 196 passes of 256 (the last one 80 frames).
    Too many for the CPU oracle, so: every embedding is finite and unit-norm, the whole run is reproducible bit for
    bit, the ragged last pass gives the bits a full pass gives for the same frames, and a sample of frames agrees
    with the fp32 oracle to the parity bar."""
    import torch
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.weights import VIT_B_32
    n, bsz = 50_000, 256
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(20250824)
    frames = torch.randint(0, 255, (n, 224, 224, 3), dtype=torch.uint8, device=dev, generator=g)    # 7.5 GB
    enc = VitEncoder(VIT_B_32, b32_weights, max_batch=bsz)

    def run():
        out = torch.empty((n, 512), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        passes = 0
        for lo in range(0, n, bsz):
            m = min(bsz, n - lo)
            enc.encode_device(frames[lo:lo + m].data_ptr(), m, out[lo:lo + m].data_ptr())
            passes += 1
        enc.synchronize()
        return out, passes

    e1, passes = run()
    assert passes == 196 and n - 195 * bsz == 80
    assert bool(torch.isfinite(e1).all()) and float((e1.norm(dim=1) - 1).abs().max()) <= 1e-5
    e2, _ = run()
    assert torch.equal(e1, e2)                                                  # reproducible, all 50,000 x 512
    tail = torch.empty((bsz, 512), dtype=torch.float32, device=dev)             # the last 80 frames inside a full pass
    mixed = torch.cat([frames[n - 80:], frames[:bsz - 80]])
    torch.cuda.synchronize()
    enc.encode_device(mixed.data_ptr(), bsz, tail.data_ptr()); enc.synchronize()
    assert torch.equal(tail[:80], e1[n - 80:]) and torch.equal(tail[80:], e1[:bsz - 80])
    pick = [0, 255, 256, 12_345, 33_333, 49_919, 49_920, 49_999]                # pass boundaries and the ragged pass
    ref = clip_vit_oracle.encode_frames(frames[pick].cpu().numpy(), b32_weights, batch_size=8)
    cos = np.sum(e1[pick].cpu().numpy() * ref, axis=1)
    assert cos.min() >= 1.0 - COS_TOL
    enc.close()


def test_config5_scale_index_8m_x_768(gpu_lib):
    """configs[4]'s index at full size on one GPU: 8,000,000 x 768 (6.1e9 elements: every row offset needs 64
    bits; fp32 master 24.6 GB + fp16 image 12.3 GB).  Properties: the fp16-scan result equals the independent exact
    fp32-master scan bit for bit, lists are sorted by (distance, id), ids are in range, every query is accounted
    for by the proof statistics, and rows queried against the index return themselves first."""
    import torch
    from video_quierer_amd.indexes.hnsw import MODE_EXACT, MODE_FP16, OptimizedHNSWIndex
    n, d, chunk = 8_000_000, 768, 1_000_000
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(555)
    idx = OptimizedHNSWIndex(dimension=d)
    keep = None
    for c0 in range(0, n, chunk):
        blk = torch.randn((chunk, d), device=dev, generator=g)
        if c0 == 7 * chunk:
            keep = (blk[-64:] / blk[-64:].norm(dim=1, keepdim=True)).clone()    # the last 64 rows (offsets > 2^32 elements)
        torch.cuda.synchronize()
        idx.add_device(blk.data_ptr(), chunk, range(c0, c0 + chunk), normalize=True)
        idx.synchronize()
        del blk
    assert idx.size() == n
    nq, k = 32, 10
    probe = torch.randn((nq, d), device=dev, generator=g)
    probe = torch.cat([probe / probe.norm(dim=1, keepdim=True), keep[:16]])   # 32 random directions + 16 stored rows
    nq = probe.shape[0]
    ids16 = torch.empty((nq, k), dtype=torch.int32, device=dev); d16 = torch.empty((nq, k), device=dev)
    idsx = torch.empty((nq, k), dtype=torch.int32, device=dev); dx = torch.empty((nq, k), device=dev)
    torch.cuda.synchronize()
    idx.search_device(probe.data_ptr(), nq, k, ids16.data_ptr(), d16.data_ptr(), mode=MODE_FP16); idx.synchronize()
    st = idx.last_search_stats()
    idx.search_device(probe.data_ptr(), nq, k, idsx.data_ptr(), dx.data_ptr(), mode=MODE_EXACT); idx.synchronize()
    assert torch.equal(ids16, idsx) and torch.equal(d16, dx)
    assert st["verified"] + st["rescanned"] + st["exact_fallback"] == nq
    dd, ii = d16.cpu().numpy(), ids16.cpu().numpy()
    assert np.all(np.diff(dd, axis=1) >= 0) and np.all((ii >= 0) & (ii < n))
    assert ii[32:, 0].tolist() == list(range(n - 64, n - 48)) and np.abs(dd[32:, 0]).max() <= 1e-5
    idx.close()


# ------------------------------------------------------------------ frame preprocessing in front of the encoder (§8f #3)
@pytest.fixture(scope="module")
def pre(gpu_lib):
    from video_quierer_amd.preprocess import FramePreprocessor
    p = FramePreprocessor()
    yield p
    p.close()


def test_resample_matches_pillow_golden(pre, golden_resample):
    """Bit-exact against Pillow / the CLIP image processor (captured in tests/golden/resample_pil.npz)."""
    import hashlib
    from conftest import RESAMPLE_CASES, resample_input
    for i, (name, h, w, kind, mode) in enumerate(RESAMPLE_CASES):
        img = resample_input(h, w, kind)
        out = (pre.stretch(img) if mode == "stretch" else pre.clip_processor(img))[0]
        assert out.shape == (224, 224, 3) and out.dtype == np.uint8
        assert hashlib.sha256(out.tobytes()).hexdigest() == str(golden_resample[f"sha256_{name}"]), name
        if i < 2:
            assert np.array_equal(out, golden_resample[f"out_{name}"])


def test_resample_ragged_sizes_filters_crops_vs_oracle(pre):
    from oracle import resample_oracle as ro
    from video_quierer_amd.preprocess import BICUBIC, BILINEAR
    # the cases, and which launch forms they reach between them: tests/test_preproc_plan_cpu.py
    from test_preproc_plan_cpu import MANY_FRAMES_CASE, RAGGED_CASES, ragged_frames, ragged_window
    rng = np.random.default_rng(8)
    for (h, w, ow, oh) in RAGGED_CASES:
        n = ragged_frames(h, w)
        frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        for filt in (BILINEAR, BICUBIC):
            ref = np.stack([ro.resize_u8(f, ow, oh, filt) for f in frames])
            assert np.array_equal(pre.resize(frames, oh, ow, filt), ref), (h, w, ow, oh, filt)
            ct, cl, ch, cw = ragged_window(ow, oh)            # a window of the resized frame = the same pixels of the full result
            got = pre.resize(frames, oh, ow, filt, crop=(ct, cl, ch, cw))
            assert np.array_equal(got, ref[:, ct:ct + ch, cl:cl + cw]), ("crop", h, w, ow, oh, filt)
    n, h, w, ow, oh = MANY_FRAMES_CASE                        # several segments per workgroup
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for filt in (BILINEAR, BICUBIC):
        ref = np.stack([ro.resize_u8(f, ow, oh, filt) for f in frames])
        assert np.array_equal(pre.resize(frames, oh, ow, filt), ref), ("many frames", filt)
    # list of separately allocated frames == stacked frames; empty list
    frames = [rng.integers(0, 256, (90, 160, 3), dtype=np.uint8) for _ in range(5)]
    assert np.array_equal(pre.resize_list(frames, 224, 224), pre.resize(np.stack(frames), 224, 224))
    assert pre.resize_list([], 224, 224).shape == (0, 224, 224, 3)
    # bad arguments raise, as the reference's wrappers do
    with pytest.raises(ValueError):
        pre.resize(frames[0], 224, 224, filter=1)              # LANCZOS is not on the path
    with pytest.raises(ValueError):
        pre.resize(frames[0], 224, 224, crop=(200, 0, 100, 10))
    with pytest.raises(TypeError):
        pre.resize(frames[0].astype(np.float32), 224, 224)


def test_resample_device_path_into_encoder(pre, encoder):
    """Device-resident frames: resize on the GPU, hand the device buffer to the encoder — same embeddings as
    encoding the Pillow-exact host result."""
    import torch
    from oracle import resample_oracle as ro
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (6, 270, 480, 3), dtype=np.uint8)
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ptr = pre.resize_device(d.data_ptr(), 6, 270, 480, 224, 224)
    pre.synchronize()
    out = torch.empty((6, 512), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    encoder.encode_device(ptr, 6, out.data_ptr(), swap_rb=True)
    encoder.synchronize()
    via_device = out.cpu().numpy()
    host = np.stack([ro.stretch_to_square(f) for f in frames])
    assert np.array_equal(via_device, encoder.encode(host, swap_rb=True))


def test_feature_extractor_resizes_on_gpu(gpu_lib, b32_weights):
    from oracle import resample_oracle as ro
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    rng = np.random.default_rng(13)
    big = [rng.integers(0, 256, (360, 640, 3), dtype=np.uint8) for _ in range(5)]
    tall = [rng.integers(0, 256, (300, 200, 3), dtype=np.uint8) for _ in range(2)]
    native = list(synth_frames(3, seed=4))
    mixed = [big[0], native[0], tall[0], big[1], native[1], big[2], tall[1], big[3], native[2], big[4]]
    fx = FeatureExtractor(model_name="seed:1234", batch_size=16, device_batch=16)
    got = fx.extract_batch(mixed)
    want = fx.extract_batch([f if f.shape[:2] == (224, 224) else ro.stretch_to_square(f) for f in mixed])
    assert np.array_equal(got, want)                            # Resize((224,224)) moved to the GPU, bit for bit
    emb = clip_vit_oracle.encode_frames(np.stack([ro.stretch_to_square(f) for f in mixed[:3]]), b32_weights)
    assert min(float(np.dot(a, b)) for a, b in zip(got[:3], emb)) >= 1.0 - COS_TOL
    from PIL import Image
    pil = fx.extract_features(Image.fromarray(np.ascontiguousarray(big[0][..., ::-1])))    # RGB PIL == BGR ndarray
    assert np.allclose(pil, got[0], atol=2e-3)
    fx2 = FeatureExtractor(model_name="seed:1234", batch_size=16, device_batch=16, resize_mode="clip_processor")
    got2 = fx2.extract_batch(big[:2])
    want2 = fx2.extract_batch([ro.clip_processor_u8(f) for f in big[:2]])
    assert np.array_equal(got2, want2) and not np.array_equal(got2, got[[0, 3]])
    fx.thread_pool.shutdown(); fx2.thread_pool.shutdown()


def test_cv_resize_vs_oracle(pre):
    """cv2.resize(frame, (w, h)) restated (INTER_LINEAR, parity unpinned vs OpenCV): the GPU kernel equals the numpy
    restatement bit for bit on down-scales, up-scales, the exact-2x shortcut, equal sizes and crop windows."""
    from oracle import cv_resize_oracle as cv
    rng = np.random.default_rng(15)
    for (h, w, ow, oh) in [(1080, 1920, 224, 224), (720, 1280, 224, 224), (448, 448, 224, 224), (100, 80, 224, 224),
                           (224, 224, 224, 224), (37, 53, 7, 5), (2, 3, 9, 4), (1, 1, 3, 3), (480, 640, 320, 240), (300, 400, 401, 299)]:
        n = 2 if h * w < 400000 else 1
        frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        ref = np.stack([cv.resize_linear_u8(f, ow, oh) for f in frames])
        assert np.array_equal(pre.cv_resize(frames, (ow, oh)), ref), (h, w, ow, oh)
        if ow >= 4 and oh >= 4:
            win = (oh // 4, ow // 4, oh // 2, ow // 2)
            got = pre.cv_resize(frames, (ow, oh), crop=win)
            assert np.array_equal(got, ref[:, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])
    # a Pillow resize after it on the same handle still uses its own tables
    f = rng.integers(0, 256, (1, 90, 160, 3), dtype=np.uint8)
    a = pre.stretch(f); pre.cv_resize(f, (224, 224)); assert np.array_equal(pre.stretch(f), a)


def test_table_cache_across_interleaved_filters(pre):
    """One handle, one geometry, the filters in turn: every call finds its own tables on the device, whatever the call
    before it left there (Pillow's and OpenCV's tables share one cache)."""
    from oracle import cv_resize_oracle as cv
    from oracle import resample_oracle as ro
    from video_quierer_amd.preprocess import BICUBIC, BILINEAR
    frames = np.random.default_rng(16).integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
    oh, ow = 24, 40
    pil = {f: np.stack([ro.resize_u8(x, ow, oh, f) for x in frames]) for f in (BILINEAR, BICUBIC)}
    lin = np.stack([cv.resize_linear_u8(x, ow, oh) for x in frames])
    assert np.array_equal(pre.resize(frames, oh, ow, BILINEAR), pil[BILINEAR])
    assert np.array_equal(pre.cv_resize(frames, (ow, oh)), lin)
    assert np.array_equal(pre.resize(frames, oh, ow, BICUBIC), pil[BICUBIC])
    out, keep, _ = pre.postprocess(frames, (ow, oh), quality_filter=False)       # the fused pass in its linear mode
    assert keep.all() and np.array_equal(out, lin)
    assert np.array_equal(pre.resize(frames, oh, ow, BILINEAR), pil[BILINEAR])


def test_frame_quality_vs_oracle(pre):
    """np.mean(frame) exactly; Laplacian variance from exact integer sums vs numpy's float64 two-pass (1e-12);
    the low-quality decision of reference frame_extractor.py:301-316 on dark / bright / flat / textured frames."""
    from oracle import quality_oracle as q
    rng = np.random.default_rng(14)
    for (h, w) in [(224, 224), (37, 53), (1, 9), (9, 1), (1, 1), (480, 640)]:
        frames = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
        frames[1] = (frames[1] // 16) + 100                      # low-contrast frame
        mean, var = pre.quality(frames)
        for i in range(3):
            m, v = q.quality(frames[i])
            assert mean[i] == m and abs(var[i] - v) <= 1e-12 * max(1.0, v), (h, w, i)
    yy, xx = np.mgrid[0:240, 0:320]
    smooth = np.stack([yy * 255 // 239, xx * 255 // 319, (yy + xx) // 3], -1).astype(np.uint8)
    batch = np.stack([np.full((240, 320, 3), 5, np.uint8), np.full((240, 320, 3), 250, np.uint8), smooth,
                      rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)])
    low = pre.is_low_quality(batch)
    assert low.tolist() == [q.is_low_quality(f) for f in batch] == [True, True, True, False]


def test_pipelined_ingest_matches_single_pass(gpu_lib):
    """stage_frames / submit_staged / wait_staged (two slots, two handles) return exactly what a plain encode of the
    same frames returns, in order, for full, ragged and mixed-size batches; misuse raises."""
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    fx = FeatureExtractor(model_name="seed:1234", batch_size=8, device_batch=16)      # 16-frame passes -> many passes
    frames = list(synth_frames(150, seed=31))
    fds = [{"frame": f, "frame_number": i} for i, f in enumerate(frames)]
    import time as _t
    t0 = _t.time()
    out = fx.extract_from_video_frames(fds)                                           # 10 passes: both ingest handles
    wall = _t.time() - t0
    assert [o["frame_number"] for o in out] == list(range(150))
    # get_stats (reference :236-258) multiplies the number of extraction_times entries by batch_size: one entry per
    # reference-sized batch, so the figure is frames / seconds (19 entries x 8 = 152 ~ 150 frames)
    st = fx.get_stats()
    assert len(fx.extraction_times) == 19 and 0.8 * 150 / wall <= st["throughput_images_per_sec"]
    ref = fx.model.encode(np.stack(frames[:150]))
    got = np.stack([o["features"] for o in out])
    assert np.abs(got - ref).max() <= 2e-6            # different tile shapes (160- vs 256-row GEMM tiles): fp32 summation order only
    few = fx.extract_from_video_frames(fds[:20])                                      # 2 passes: the single handle
    assert np.array_equal(np.stack([o["features"] for o in few]), ref[:20])
    odd = [dict(fd) for fd in fds[:40]]
    odd[3]["frame"] = np.ascontiguousarray(np.repeat(np.repeat(frames[3], 2, 0), 2, 1))   # 448x448: resized on the GPU
    mixed = fx.extract_from_video_frames(odd)
    assert np.abs(np.stack([o["features"] for i, o in enumerate(mixed) if i != 3]) - np.delete(ref[:40], 3, 0)).max() <= 2e-6
    m = fx.model
    m.stage_frames(0, frames[:4])
    m.submit_staged(0, 4)
    with pytest.raises(ValueError):
        m.submit_staged(0, 4)                          # slot busy
    with pytest.raises(ValueError):
        m.stage_frames(0, frames[:4])                  # would overwrite a batch in flight
    assert np.array_equal(m.wait_staged(0, 4), ref[:4])
    with pytest.raises(ValueError):
        m.wait_staged(0, 4)                            # nothing in flight
    fx.thread_pool.shutdown()


def test_ingest_recovers_after_a_bad_frame(gpu_lib):
    """An exception in the middle of a pipelined ingest (a frame of the wrong dtype) propagates, as the reference's
    extract_from_video_frames re-raises (:207-209), and leaves the extractor usable: in-flight slots are drained."""
    from video_quierer_amd.core.feature_extractor import FeatureExtractor
    fx = FeatureExtractor(model_name="seed:1234", batch_size=8, device_batch=16)
    frames = list(synth_frames(96, seed=41))
    fds = [{"frame": f, "frame_number": i} for i, f in enumerate(frames)]
    bad = [dict(fd) for fd in fds]
    bad[70]["frame"] = frames[70].astype(np.float32)
    with pytest.raises(TypeError):
        fx.extract_from_video_frames(bad)
    again = fx.extract_from_video_frames(fds)
    assert len(again) == 96 and np.abs(np.stack([o["features"] for o in again]) - fx.model.encode(np.stack(frames))).max() <= 2e-6
    fx.thread_pool.shutdown()


def test_index_zero_vectors_do_not_break_search(gpu_lib):
    """The reference divides by the norm without a guard (hnsw.py:157, :250/:499): a zero query yields NaN distances
    and no error [SURVEY.md §8a K6], a zero row is stored as NaNs.  Here: a zero query returns k entries with NaN
    distance/score and no exception on both scan paths; a zero row never displaces a finite result."""
    import warnings
    from video_quierer_amd.indexes.hnsw import OptimizedHNSWIndex
    rng = np.random.default_rng(17)
    for n in (100, 20000):                                   # exact path / fp16-scan path
        vecs = rng.standard_normal((n, 64)).astype(np.float32)
        idx = OptimizedHNSWIndex(dimension=64)
        idx.add_batch(list(vecs), list(range(n)))
        before = [(r["id"], r["distance"]) for r in idx.search(vecs[5], 5)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = idx.search(np.zeros(64, np.float32), 3)
            assert len(res) == 3 and all(np.isnan(r["distance"]) and np.isnan(r["score"]) for r in res)
            idx.add(np.zeros(64, np.float32), 10 * n)
        assert idx.size() == n + 1
        assert [(r["id"], r["distance"]) for r in idx.search(vecs[5], 5)] == before
        idx.close()
