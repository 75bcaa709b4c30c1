"""The per-case bodies of tests/test_encoder_stages.py, where the tests and a fresh child process can both call them.

run_f32_chain / run_split_chain are one case each of the two stage tests: the layer-limited passes, every buffer read back
and held to the fp64 references and derived bounds of encoder_stage_ref.py, then the product pass.  The caller has set the
environment the handle is to be created under ($VQ_AMD_GEMM, $VQ_AMD_RESID, $VQ_AMD_ATTN: read at handle creation).

assert_ln_plans is what makes a case about ONE kernel: it asks vq_debug_gemm_plan what q|k|v, fc1, out_proj and fc2 (and the
patch embedding) get in this process and fails if that is not the kernel and the tiles per workgroup the case was written for.

As a program (`python tests/encoder_stage_run.py tpw-child TPW`) this is the child of
test_multi_tile_tiles_per_workgroup_in_a_child: $VQ_AMD_GEMM_TPW is read once per process (gemm_options), so each forced
count needs a process of its own."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import encoder_stage_ref as R
from video_quierer_amd.weights import TextConfig, VitConfig

TILE128, RING160, AUTO_NO160, DEEP, MULTI_WHERE_WORTH, MULTI = 1, 5, 6, 8, 15, 16      # GemmKernel ids (csrc/gemm_dispatch.h)
REPEAT_BUFFERS = ("qkv", "att", "mlp", "x")


def record(tag, ratios, table=None):
    lines = [f"{tag:44s} {stage}{layer:<2d} {r:.4g}" for (stage, layer), r in ratios.items()]
    print("\n".join(lines))
    path = os.environ.get("VQ_STAGE_RATIOS_OUT")
    if path and table:                                      # a second table next to the first
        path = os.path.join(os.path.dirname(path), table)
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def read(enc, rows, names):
    return {nm: enc.debug_read(nm, rows) for nm in names}


def plan_resid_rows(lib, cfg, n, concurrent):
    """(out_proj rows, fc2 rows) of a handle with max_batch = n under this process's environment (vq_debug_encoder_plan)."""
    from video_quierer_amd import _lib
    out = _lib.EncoderPlanC()
    if isinstance(cfg, TextConfig):
        c = _lib.TextConfigC(cfg.vocab, cfg.max_positions, cfg.hidden, cfg.mlp, cfg.layers, cfg.heads, cfg.proj_dim, cfg.eos_token_id, cfg.ln_eps)
        args = (None, ctypes.byref(c))
    else:
        c = _lib.VitConfigC(cfg.image_size, cfg.patch_size, cfg.hidden, cfg.mlp, cfg.layers, cfg.heads, cfg.proj_dim, cfg.ln_eps)
        args = (ctypes.byref(c), None)
    assert lib.vq_debug_encoder_plan(*args, n, n, 1 | (2 if concurrent else 0), 0, -1, 0, ctypes.byref(out), None) == 0
    return out.rows_out, out.rows_fc2


def plan_kernels(lib, M, N, K, force, row_in=0):
    """[(kernel, rows, first row, tiles per workgroup), ...] of launch_gemm_auto for this shape in this process."""
    n = ctypes.c_int(0)
    k, r, r0, t = ((ctypes.c_int * 2)() for _ in range(4))
    assert lib.vq_debug_gemm_plan(M, N, K, K, K, row_in, force, ctypes.byref(n), k, r, r0, t) == 0
    return [(k[i], r[i], r0[i], t[i]) for i in range(n.value)]


def pad_rows(r):
    """enc_pad_rows (csrc/encoder_plan.h): to 256 where that adds less than 1/16 of the 128-row padding, else to 128."""
    r256, r128 = -(-r // 256) * 256, -(-r // 128) * 128
    return r256 if (r256 - r128) * 16 <= r128 else r128


def assert_ln_plans(lib, cfg, tokens, n, plan_force, ln, resid=None):
    """ln = {"qkv": (kernel, tiles per workgroup), "fc1": ..., optionally "patch": ...}: the single step each LayerNorm-consuming
    GEMM (row_in) must plan as on the padded rows of n inputs; resid = (rows, kernel) of out_proj and fc2.  Returns the plans
    as text for the table's tag."""
    rows = pad_rows(n * tokens)
    H = cfg.hidden
    for name, N in (("qkv", 3 * H), ("fc1", cfg.mlp)):
        kernel, tpw = ln[name]
        got = plan_kernels(lib, rows, N, H, plan_force, row_in=1)
        assert got == [(kernel, rows, 0, tpw)], f"{name} ({rows} x {N} x {H}, id {plan_force}) plans as {got}: this case was written for kernel " \
            f"{kernel} at {tpw} tiles per workgroup - move it to a shape that still gets that kernel"
    if "patch" in ln:
        prows, pk = pad_rows(n * (tokens - 1)), 3 * cfg.patch_size ** 2
        assert plan_kernels(lib, prows, H, pk, plan_force) == [(ln["patch"][0], prows, 0, ln["patch"][1])], ("patch", prows, pk)
    if resid is not None:
        for K in (H, cfg.mlp):
            assert plan_kernels(lib, resid[0], H, K, plan_force) == [(resid[1], resid[0], 0, 1)], (n, K)
    return f"qkv={ln['qkv'][0]}x{ln['qkv'][1]} fc1={ln['fc1'][0]}x{ln['fc1'][1]}"


def assert_repeats(run, reread, first, tag):
    """The pass just read, twice more: every buffer bit for bit what the first read gave.  A race between the operand DMA that
    runs under a GEMM epilogue and that epilogue's LDS strips need not leave a bound every time, but it rarely repeats."""
    for rep in (1, 2):
        run()
        again = reread()
        assert first and set(again) >= set(first), (tag, sorted(first), sorted(again))
        for nm in first:
            a, b = np.ascontiguousarray(first[nm]), np.ascontiguousarray(again[nm])
            bad = int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))
            assert bad == 0, f"{tag}: repeat {rep} of the same pass changed {bad} elements of {nm}"


def finish(tag, ratios, table=None):
    record(tag, ratios, table)
    amb = ratios.pop(("ambiguous", 0))
    print(f"{tag}: {amb} fc1 operand elements with an ambiguous 16-bit rounding (none excluded)")
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{tag}: stage {worst} is {ratios[worst]:.3g} x its bound"
    return ratios


def run_f32_chain(cfg, is_text, dt, kind, n, concurrent, tag):
    """One case of test_every_stage_against_fp64_on_the_device_inputs ($VQ_AMD_RESID=f32 is set by the caller)."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.text_encoder import TextEncoder
    tower = "text" if is_text else "image"
    W = R.make_weights(tower, cfg, kind)
    inp = R.make_input(tower, cfg, n)
    tw = R.Tower(tower, cfg, W, dt)
    enc = TextEncoder(cfg, W, max_batch=n, compute_dtype=dt) if is_text else \
        VitEncoder(cfg, W, max_batch=n, compute_dtype=dt, concurrent=concurrent)
    run = (lambda **kw: enc.encode_ids(inp)) if is_text else (lambda swap_rb=True: enc.encode(inp, swap_rb=swap_rb))
    rows = n * tw.T
    try:
        runs = []
        for k in range(cfg.layers + 1):
            enc.debug_set_layers(k)
            run()
            runs.append(read(enc, rows, ("x", "h") if k == 0 else ("x", "h", "qkv", "att", "mlp")))
        # (every attention form accumulates in a fixed order, no atomics: `att` is held to the same bits as the rest)
        assert_repeats(run, lambda: read(enc, rows, REPEAT_BUFFERS), {nm: runs[-1][nm] for nm in REPEAT_BUFFERS}, tag)
        ratios = R.check_chain(tw, n, inp, runs)
        if not is_text:                                     # the other channel order through patchify
            enc.debug_set_layers(0)
            run(swap_rb=False)
            ratios[("embed_rgb", 0)] = R.check_embed(tw, inp, enc.debug_read("x", rows), swap_rb=False)
        enc.debug_set_layers(-1)
        emb = run()
        if is_text:
            x = enc.debug_read("x", rows)
            assert np.array_equal(x.view(np.uint32), runs[-1]["x"].view(np.uint32)), "full pass and the pass limited to every block differ"
            ratios[("pool", cfg.layers - 1)] = R.check_pool(tw, x[R.eos_rows(inp, cfg)], emb)
        else:
            prod = {"x": enc.debug_read("x", rows), "att": enc.debug_read("att", rows), "h": enc.debug_read("h", n), "mlp": enc.debug_read("mlp", n)}
            ratios.update(R.check_product_image(tw, n, runs[-2], prod, emb))
    finally:
        enc.close()
    return finish(tag, ratios)


def run_split_chain(cfg, is_text, kind, n, concurrent, resid, full_pass, tag):
    """One case of test_every_stage_of_the_split_stream_against_fp64.  full_pass: the handle can run its last block (an image
    tower under a forced 256x256 id cannot: that id refuses the 128 rows of the CLS-only GEMMs)."""
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.text_encoder import TextEncoder
    tower = "text" if is_text else "image"
    tw = R.Tower(tower, cfg, R.make_weights(tower, cfg, kind), "fp16")
    inp = R.make_input(tower, cfg, n)
    rows = n * tw.T
    full_rows = cfg.layers if is_text else cfg.layers - 1   # blocks that run on every row
    want_forms = R.split_forms(tw) if resid is None else [False] * (cfg.layers + 1)
    enc = TextEncoder(cfg, tw.W, max_batch=n, compute_dtype="fp16") if is_text else \
        VitEncoder(cfg, tw.W, max_batch=n, compute_dtype="fp16", concurrent=concurrent)
    run = (lambda: enc.encode_ids(inp)) if is_text else (lambda: enc.encode(inp))
    names = ("x", "h", "xl", "qkv", "att", "mlp")
    try:
        enc.debug_keep_stream(True)
        runs, forms = [], []
        for k in range(cfg.layers + 1 if full_pass else full_rows + 1):
            enc.debug_set_layers(k)
            emb_k = run()
            forms.append(enc.debug_stream_is_split())
            r = read(enc, rows, ("x", "h", "xl") if k == 0 else names)
            r["split"] = forms[-1]
            runs.append(r)
        assert forms == want_forms[:len(forms)], f"{tag}: stream forms {forms}, the rule gives {want_forms}"
        # qkv, att, mlp, x as in the fp32-stream test; h and xl too: where the stream is left split they ARE the block's output
        assert_repeats(run, lambda: read(enc, rows, names), {nm: runs[-1][nm] for nm in names}, tag)
        ratios = R.check_chain(tw, n, inp, runs[:full_rows + 1], split=resid is None)
        if full_pass:
            enc.debug_set_layers(-1)
            emb = run()
            assert not enc.debug_stream_is_split()
            x = enc.debug_read("x", rows)
            assert np.array_equal(emb.view(np.uint32), emb_k.view(np.uint32)), "the pass limited to every block and the full pass differ"
            if is_text:
                assert np.array_equal(x.view(np.uint32), runs[full_rows]["x"].view(np.uint32)), "full pass and the pass limited to every block differ"
                ratios[("pool", cfg.layers - 1)] = R.check_pool(tw, x[R.eos_rows(inp, cfg)], emb)
            else:
                # (check_product_image holds the non-CLS rows to the x that block 1's fc2 wrote back from a split input)
                assert np.array_equal(x.view(np.uint32), runs[cfg.layers]["x"].view(np.uint32)), "full pass and the pass limited to every block differ"
                prod = {"x": x, "att": enc.debug_read("att", rows), "h": enc.debug_read("h", n), "mlp": enc.debug_read("mlp", n)}
                ratios.update(R.check_product_image(tw, n, runs[full_rows], prod, emb))
        enc.debug_keep_stream(False)                        # off: a layer-limited pass keeps the fp32 stream, as before
        enc.debug_set_layers(1)
        run()
        assert not enc.debug_stream_is_split()
    finally:
        enc.close()
    return finish(tag, ratios, table="ratios_split.txt")


# ---------------------------------------------------------------- the child: a forced number of tiles per multi-tile workgroup
# ViT-L's widths on the 50-token geometry: q|k|v is N = 3072 = 12 tiles across (ViT-L/14@336 at batch 32 runs it as 73 x 12 tiles,
# four per workgroup).  n = 56: 2,800 rows pad to 2,816 = 11 tile rows, 132 q|k|v tiles - under id 15 the multi-tile kernel.
TPW_CFG = VitConfig(image_size=224, patch_size=32, hidden=1024, mlp=4096, heads=16, proj_dim=768, layers=2)
TPW_N = 56
TPW_COUNTS = (4, 2, 1, 12)


def tpw_child(tpw):
    """Runs under $VQ_AMD_GEMM=15 and $VQ_AMD_GEMM_TPW=tpw (set by the parent): both chains on TPW_CFG, after the plan shows that
    the switch took effect."""
    from video_quierer_amd import _lib
    assert int(os.environ["VQ_AMD_GEMM_TPW"]) == tpw and int(os.environ["VQ_AMD_GEMM"]) == MULTI_WHERE_WORTH
    _lib.init(0)
    rows = pad_rows(TPW_N * TPW_CFG.tokens)
    assert rows == 2816
    # fc1: N = 4096 = 16 tiles across, not divisible by 3 -> the deep kernel with the row-stat prologue, whatever $VQ_AMD_GEMM_TPW says
    kernels = assert_ln_plans(_lib.load(), TPW_CFG, TPW_CFG.tokens, TPW_N, MULTI_WHERE_WORTH, {"qkv": (MULTI, tpw), "fc1": (DEEP, 1)},
                              resid=(rows, TILE128))
    assert plan_resid_rows(_lib.load(), TPW_CFG, TPW_N, False) == (rows, rows)
    base = f"t50w1024 stress rows={TPW_N * TPW_CFG.tokens} {kernels}"
    os.environ["VQ_AMD_RESID"] = "f32"
    run_f32_chain(TPW_CFG, False, "fp16", "stress", TPW_N, False, base + " f32")
    del os.environ["VQ_AMD_RESID"]
    run_split_chain(TPW_CFG, False, "stress", TPW_N, False, None, True, base + f" gemm={TILE128}")
    print(f"tpw-child {tpw}: ok")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "tpw-child", sys.argv
    tpw_child(int(sys.argv[2]))
