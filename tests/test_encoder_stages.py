"""Every encoder stage against fp64 on the inputs the device itself had (GPU).

Per case: passes limited to 0, 1 and 2 blocks (debug_set_layers) on the same input, every intermediate buffer read back
(debug_read), and each stage compared with its fp64 reference inside the bound DERIVED in tests/encoder_stage_ref.py
(shown sound and non-vacuous without a GPU by tests/test_encoder_stages_cpu.py).  Then the product pass (fp32 residual
stream, default pruning): the CLS-only last block with its gather, split-K and reduce, and the pooling head.  Every
valid element of every buffer takes part.  Each check prints max(error / bound); profiles/encoder_stages/ratios.txt is
that table from one run."""
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


def _record(tag, ratios):
    lines = [f"{tag:44s} {stage}{layer:<2d} {r:.4g}" for (stage, layer), r in ratios.items()]
    print("\n".join(lines))
    path = os.environ.get("VQ_STAGE_RATIOS_OUT")
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
