"""Every encoder stage against fp64 on the inputs the device itself had (GPU).

Per case: passes limited to 0, 1 and 2 blocks (debug_set_layers) on the same input, every intermediate buffer read back
(debug_read), and each stage compared with its fp64 reference inside the bound DERIVED in tests/encoder_stage_ref.py
(shown sound and non-vacuous without a GPU by tests/test_encoder_stages_cpu.py).  Then the product pass (fp32 residual
stream, default pruning): the CLS-only last block with its gather, split-K and reduce, and the pooling head.  Every
valid element of every buffer takes part.  Each check prints max(error / bound); profiles/encoder_stages/ratios.txt is
that table from one run.

The second test does the same for the DEFAULT pass, which holds the residual stream between its residual epilogues as
fp16 + one fp8 byte (debug_keep_stream: a layer-limited pass then runs its blocks exactly as the full pass does; the low
bytes are read back raw and decoded here).  profiles/encoder_stages/ratios_split.txt is its table."""
import ctypes
import os

import numpy as np
import pytest

import encoder_stage_ref as R
from video_quierer_amd.weights import TextConfig, VitConfig

pytestmark = pytest.mark.gpu

IMAGE_GEOMETRIES = {        # name -> (config, default batch)
    "t37": (VitConfig(image_size=192, patch_size=32, layers=2), 4),                 # run-time-T single tile
    "t50": (VitConfig(image_size=224, patch_size=32, layers=2), 5),                 # compile-time-T single tile; 250 rows
    "t65": (VitConfig(image_size=112, patch_size=14, layers=2), 3),                 # generic patchify, K 588 -> 640; one key past a tile
    "t197": (VitConfig(image_size=224, patch_size=16, layers=2), 2),
    "t257": (VitConfig(image_size=256, patch_size=16, layers=2), 2),                # four key steps + one key
    "t577": (VitConfig(image_size=336, patch_size=14, hidden=1024, mlp=4096, heads=16, proj_dim=768, layers=2), 1),
}
TEXT_GEOMETRIES = {
    "text512": (TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, layers=2), 4),
    "text768": (TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, hidden=768, mlp=3072, heads=12, proj_dim=768, layers=2), 3),
    "text512_p65": (TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, max_positions=65, layers=2), 4),
}


def _cases():
    out = []
    for geo, (cfg, n) in IMAGE_GEOMETRIES.items():
        forms = ["default"] + (["t64"] if cfg.tokens == 50 else []) + (["q64", "simple"] if cfg.tokens > 64 else [])
        for form in forms:
            for dt in ("fp16", "bf16"):
                out.append((geo, form, dt, "stress", n, False))
    for geo, dt, kind in (("t50", "fp16", "seeded"), ("t50", "bf16", "seeded"), ("t257", "fp16", "seeded"),
                          ("t50", "fp16", "lowvar"), ("t50", "bf16", "lowvar"), ("t197", "fp16", "lowvar")):
        out.append((geo, "default", dt, kind, IMAGE_GEOMETRIES[geo][1], False))
    for n in (1, 6, 128):                                   # 50 rows (128-row padding), 300 (160-row tiles / 256-row padding), 6400 = 25 x 256
        out.append(("t50", "default", "fp16", "stress", n, False))
    out.append(("t50", "default", "fp16", "stress", 5, True))
    for geo, (cfg, n) in TEXT_GEOMETRIES.items():
        for dt in ("fp16", "bf16"):
            out.append((geo, "default", dt, "stress", n, False))
    out += [("text512", "default", "fp16", "seeded", 4, False), ("text512", "default", "fp16", "lowvar", 4, False)]
    return out


def _record(tag, ratios, table=None):
    lines = [f"{tag:44s} {stage}{layer:<2d} {r:.4g}" for (stage, layer), r in ratios.items()]
    print("\n".join(lines))
    path = os.environ.get("VQ_STAGE_RATIOS_OUT")
    if path and table:                                      # a second table next to the first
        path = os.path.join(os.path.dirname(path), table)
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def _read(enc, rows, names):
    return {nm: enc.debug_read(nm, rows) for nm in names}


@pytest.mark.parametrize("geo,form,dt,kind,n,concurrent", _cases(), ids=lambda v: str(v))
def test_every_stage_against_fp64_on_the_device_inputs(gpu_lib, monkeypatch, geo, form, dt, kind, n, concurrent):
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.text_encoder import TextEncoder
    is_text = geo in TEXT_GEOMETRIES
    cfg = (TEXT_GEOMETRIES if is_text else IMAGE_GEOMETRIES)[geo][0]
    tower = "text" if is_text else "image"
    W = R.make_weights(tower, cfg, kind)
    inp = R.make_input(tower, cfg, n)
    tw = R.Tower(tower, cfg, W, dt)
    monkeypatch.setenv("VQ_AMD_RESID", "f32")              # the product pass below keeps the fp32 x (layer-limited passes always do)
    if form != "default":
        monkeypatch.setenv("VQ_AMD_ATTN", form)
    enc = TextEncoder(cfg, W, max_batch=n, compute_dtype=dt) if is_text else \
        VitEncoder(cfg, W, max_batch=n, compute_dtype=dt, concurrent=concurrent)
    run = (lambda **kw: enc.encode_ids(inp)) if is_text else (lambda swap_rb=True: enc.encode(inp, swap_rb=swap_rb))
    rows = n * tw.T
    tag = f"{geo} {form} {dt} {kind} rows={rows}" + (" concurrent" if concurrent else "")
    try:
        runs = []
        for k in range(cfg.layers + 1):
            enc.debug_set_layers(k)
            run()
            runs.append(_read(enc, rows, ("x", "h") if k == 0 else ("x", "h", "qkv", "att", "mlp")))
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
    _record(tag, ratios)
    amb = ratios.pop(("ambiguous", 0))
    print(f"{tag}: {amb} fc1 operand elements with an ambiguous 16-bit rounding (none excluded)")
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{tag}: stage {worst} is {ratios[worst]:.3g} x its bound"


# ---------------------------------------------------------------- the default pass: the split 16 + 8-bit residual stream
TILE128, RING160, DEEP = 1, 5, 8                            # GemmKernel ids (csrc/gemm_dispatch.h)
SPLIT_IMAGE = {             # three blocks: OUT_SPLIT, IN|OUT_SPLIT (block 0), IN|OUT_SPLIT, IN_SPLIT|OUT_F32 (block 1), CLS-only (block 2)
    "t50": VitConfig(image_size=224, patch_size=32, layers=3),
    "t65": VitConfig(image_size=112, patch_size=14, layers=3),
    "t197": VitConfig(image_size=224, patch_size=16, layers=3),
}
SPLIT_TEXT = {"text512": TEXT_GEOMETRIES["text512"][0]}     # two blocks reach all four modes; pools from the rewritten fp32 x


def _split_cases():
    """(geometry, kind, batch, concurrent, $VQ_AMD_GEMM, $VQ_AMD_RESID, GEMM rows of out_proj / fc2, their kernel).

    The rows are the encoder's padding rule (plan_forward: 160-row tiles where prefer_tn160 holds for a lone handle, else 128 or
    256), pinned here and compared with vq_debug_encoder_plan's out_proj and fc2 rows in the test; the kernel for them is asked
    of vq_debug_gemm_plan.  t50: 50 and 250 rows -> 128 and 256 rows of the 128x128
    kernel; 300 rows pad to 384 of the same kernel (two 160-row tiles would be no more workgroups than two 256-row tiles), so
    350 rows (n = 7: three 160-row tiles, the odd-MI tail) are the smallest batch on the ring; 6400 rows are on the ring too.
    The deep 256x256 kernel comes by $VQ_AMD_GEMM=8 at 256 rows: the text tower at n = 3 (231 rows) start to end, the image
    tower at n = 5 in the full-row blocks only - its CLS-only GEMMs have 128 rows, which that id refuses."""
    out = []
    for kind in ("passthrough", "stress"):
        out += [("t50", kind, 1, False, None, None, 128, TILE128), ("t50", kind, 5, False, None, None, 256, TILE128),
                ("t50", kind, 6, False, None, None, 384, TILE128), ("t50", kind, 7, False, None, None, 480, RING160),
                ("t50", kind, 5, False, DEEP, None, 256, DEEP), ("text512", kind, 3, False, DEEP, None, 256, DEEP),
                ("t197", kind, 2, False, None, None, 480, RING160), ("t65", kind, 3, False, None, None, 256, TILE128),
                ("text512", kind, 4, False, None, None, 384, TILE128)]
    out += [("t50", "stress", 5, True, None, None, 256, TILE128), ("t50", "stress", 128, False, None, None, 6400, RING160),
            ("t50", "seeded", 5, False, None, None, 256, TILE128),
            ("t50", "passthrough", 5, False, None, "f32", 256, TILE128), ("text512", "passthrough", 4, False, None, "f32", 384, TILE128)]
    return out


def _plan_resid_rows(lib, cfg, n, concurrent):
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


def _plan_kernels(lib, M, N, K, force):
    n = ctypes.c_int(0)
    k, r, r0, t = ((ctypes.c_int * 2)() for _ in range(4))
    assert lib.vq_debug_gemm_plan(M, N, K, K, K, 0, force, ctypes.byref(n), k, r, r0, t) == 0
    return [(k[i], r[i]) for i in range(n.value)]


@pytest.mark.parametrize("geo,kind,n,concurrent,force,resid,gemm_rows,kernel", _split_cases(), ids=lambda v: str(v))
def test_every_stage_of_the_split_stream_against_fp64(gpu_lib, monkeypatch, geo, kind, n, concurrent, force, resid, gemm_rows, kernel):
    from video_quierer_amd import _lib
    from video_quierer_amd.encoder import VitEncoder
    from video_quierer_amd.text_encoder import TextEncoder
    is_text = geo in SPLIT_TEXT
    cfg = (SPLIT_TEXT if is_text else SPLIT_IMAGE)[geo]
    tower = "text" if is_text else "image"
    tw = R.Tower(tower, cfg, R.make_weights(tower, cfg, kind), "fp16")
    inp = R.make_input(tower, cfg, n)
    monkeypatch.delenv("VQ_AMD_RESID", raising=False)
    monkeypatch.delenv("VQ_AMD_GEMM", raising=False)
    if resid:
        monkeypatch.setenv("VQ_AMD_RESID", resid)
    if force:
        monkeypatch.setenv("VQ_AMD_GEMM", str(force))
    rows = n * tw.T
    assert gemm_rows >= rows
    assert _plan_resid_rows(_lib.load(), cfg, n, concurrent) == (gemm_rows, gemm_rows), (geo, n)
    plan_force = force or (6 if concurrent else 0)          # a concurrent handle plans as GK_AUTO_NO160
    for K in (cfg.hidden, cfg.mlp):                         # out_proj, fc2: the GEMMs that carry the wide residual epilogue
        assert _plan_kernels(_lib.load(), gemm_rows, cfg.hidden, K, plan_force) == [(kernel, gemm_rows)], (geo, n, K)
    full_pass = not (force and not is_text)                 # (see _split_cases: the forced id refuses the CLS-only GEMMs)
    full_rows = cfg.layers if is_text else cfg.layers - 1   # blocks that run on every row
    want_forms = R.split_forms(tw) if resid is None else [False] * (cfg.layers + 1)
    enc = TextEncoder(cfg, tw.W, max_batch=n, compute_dtype="fp16") if is_text else \
        VitEncoder(cfg, tw.W, max_batch=n, compute_dtype="fp16", concurrent=concurrent)
    run = (lambda: enc.encode_ids(inp)) if is_text else (lambda: enc.encode(inp))
    tag = f"{geo} {kind} rows={rows} gemm={kernel}" + (" concurrent" if concurrent else "") + (" resid=f32" if resid else "")
    try:
        enc.debug_keep_stream(True)
        runs, forms = [], []
        for k in range(cfg.layers + 1 if full_pass else full_rows + 1):
            enc.debug_set_layers(k)
            emb_k = run()
            forms.append(enc.debug_stream_is_split())
            r = _read(enc, rows, ("x", "h", "xl") if k == 0 else ("x", "h", "xl", "qkv", "att", "mlp"))
            r["split"] = forms[-1]
            runs.append(r)
        assert forms == want_forms[:len(forms)], f"{tag}: stream forms {forms}, the rule gives {want_forms}"
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
    _record(tag, ratios, table="ratios_split.txt")
    amb = ratios.pop(("ambiguous", 0))
    print(f"{tag}: {amb} fc1 operand elements with an ambiguous 16-bit rounding (none excluded)")
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"{tag}: stage {worst} is {ratios[worst]:.3g} x its bound"
