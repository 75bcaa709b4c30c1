"""Every encoder stage against fp64 on the inputs the device itself had (GPU).

Per case: passes limited to 0, 1 and 2 blocks (debug_set_layers) on the same input, every intermediate buffer read back
(debug_read), and each stage compared with its fp64 reference inside the bound DERIVED in tests/encoder_stage_ref.py
(shown sound and non-vacuous without a GPU by tests/test_encoder_stages_cpu.py).  Then the product pass (fp32 residual
stream, default pruning): the CLS-only last block with its gather, split-K and reduce, and the pooling head.  Every
valid element of every buffer takes part.  Each check prints max(error / bound); profiles/encoder_stages/ratios.txt is
that table from one run.

The second test does the same for the DEFAULT pass, which holds the residual stream between its residual epilogues as
fp16 + one fp8 byte (debug_keep_stream: a layer-limited pass then runs its blocks exactly as the full pass does; the low
bytes are read back raw and decoded here).  profiles/encoder_stages/ratios_split.txt is its table.

The bodies of both live in tests/encoder_stage_run.py.  Every case also repeats its last layer-limited pass twice and wants
the same bits.  Cases that name a GEMM kernel for q|k|v and fc1 (_multi_cases, _split_multi_cases: the multi-tile 256x256
kernel gemm_tn256dm under the LayerNorm-consuming epilogues, the deep kernel under the split residual epilogue on many tile
rows, the benchmark's own dispatch at n = 220) first ask vq_debug_gemm_plan and fail if the dispatch gives them another;
tests/test_gemm_plan_cpu.py pins the same plans without a GPU.  The third test forces the tiles per multi-tile workgroup,
which takes a fresh process per count."""
import os

import pytest

import encoder_stage_run as S
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


def _old(case, n_new):
    """A case from before the trailing parameters existed: they are None, and the id is the one `ids=str` gave it."""
    return pytest.param(*case, *(None,) * n_new, id="-".join(str(v) for v in case))


def _multi_cases():
    """(geometry, form, type, fixture, batch, concurrent, $VQ_AMD_GEMM, {GEMM: (kernel, tiles per workgroup)}): the LayerNorm-consuming
    GEMMs on gemm_tn256dm.  Id 15 gives them that kernel once the shape tiles by 256 with tiles_n % 3 == 0 and >= 128 tiles.
    t50: hidden 768, q|k|v 9 tiles across -> 15 tile rows (135 tiles; fc1 180): n = 72, whose 3,600 rows pad to 3,840, is the
    smallest batch that has them (n = 71 pads to 3,584: 126 tiles, the 128x128 kernel).  text512: q|k|v 6 tiles across (two
    workgroups of three on a tile row, K = 512) -> 22 tile rows = 5,632 rows, from n = 70 (5,390 rows) on; fc1 is 8 tiles across,
    not divisible by 3: the deep kernel with the row-stat prologue on 22 tile rows.  out_proj and fc2 (45 / 44 tiles) stay on the
    128x128 kernel, like the patch embedding and the CLS-only GEMMs."""
    m3 = {"qkv": (S.MULTI, 3), "fc1": (S.MULTI, 3)}
    return [pytest.param("t50", "default", "fp16", "stress", 72, False, 15, m3, id="t50-default-fp16-stress-72-False-gemm15-qkv16x3+fc116x3"),
            pytest.param("t50", "default", "bf16", "stress", 72, False, 15, m3, id="t50-default-bf16-stress-72-False-gemm15-qkv16x3+fc116x3"),
            pytest.param("text512", "default", "fp16", "stress", 70, False, 15, {"qkv": (S.MULTI, 3), "fc1": (S.DEEP, 1)},
                         id="text512-default-fp16-stress-70-False-gemm15-qkv16x3+fc18x1")]


@pytest.mark.parametrize("geo,form,dt,kind,n,concurrent,force,ln", [_old(c, 2) for c in _cases()] + _multi_cases())
def test_every_stage_against_fp64_on_the_device_inputs(gpu_lib, monkeypatch, geo, form, dt, kind, n, concurrent, force, ln):
    from video_quierer_amd import _lib
    is_text = geo in TEXT_GEOMETRIES
    cfg = (TEXT_GEOMETRIES if is_text else IMAGE_GEOMETRIES)[geo][0]
    T = cfg.max_positions if is_text else cfg.tokens
    monkeypatch.setenv("VQ_AMD_RESID", "f32")              # the product pass below keeps the fp32 x (layer-limited passes always do)
    if form != "default":
        monkeypatch.setenv("VQ_AMD_ATTN", form)
    tag = f"{geo} {form} {dt} {kind} rows={n * T}" + (" concurrent" if concurrent else "")
    if force:
        monkeypatch.setenv("VQ_AMD_GEMM", str(force))
        rows = S.pad_rows(n * T)
        assert S.plan_resid_rows(_lib.load(), cfg, n, concurrent) == (rows, rows), (geo, n)
        tag += " " + S.assert_ln_plans(_lib.load(), cfg, T, n, force, ln, resid=(rows, TILE128))
    S.run_f32_chain(cfg, is_text, dt, kind, n, concurrent, tag)


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


def _split_multi_cases():
    """The cases of _split_cases + {GEMM: (kernel, tiles per workgroup)} of q|k|v and fc1 (and the patch embedding): see _multi_cases
    for the batches under $VQ_AMD_GEMM=15.  Two more here:
      * the benchmark's own dispatch, no $VQ_AMD_GEMM: a concurrent handle (it plans as id 6) at n = 220.  11,000 rows pad to
        11,008 = 43 tile rows, the fewest at which the unforced dispatch picks the multi-tile kernel (its `worth` rule wants
        tiles / 3 >= 128: q|k|v 387 tiles = 129 workgroups of three, fc1 516 = 172; 42 tile rows give 126), and batches 216 .. 220
        are the ones that pad to exactly that.  out_proj and fc2 have 129 tiles: the deep kernel under the split residual
        epilogue across 43 tile rows, no tail split; the patch embedding (10,780 -> 11,008 rows) is on the deep kernel too.
      * $VQ_AMD_GEMM=8 at n = 77 (3,850 rows pad to 4,096): the deep kernel under every tower epilogue on 16 tile rows (the
        CLS-only block is refused by that id, as at n = 5)."""
    m3 = {"qkv": (S.MULTI, 3), "fc1": (S.MULTI, 3)}
    d1 = {"qkv": (DEEP, 1), "fc1": (DEEP, 1)}
    return [pytest.param("t50", "stress", 72, False, 15, None, 3840, TILE128, m3, id="t50-stress-72-False-15-None-3840-1-qkv16x3+fc116x3"),
            pytest.param("text512", "stress", 70, False, 15, None, 5632, TILE128, {"qkv": (S.MULTI, 3), "fc1": (DEEP, 1)},
                         id="text512-stress-70-False-15-None-5632-1-qkv16x3+fc18x1"),
            pytest.param("t50", "stress", 220, True, None, None, 11008, DEEP, dict(m3, patch=(DEEP, 1)),
                         id="t50-stress-220-True-None-None-11008-8-qkv16x3+fc116x3+patch8x1"),
            pytest.param("t50", "stress", 77, False, DEEP, None, 4096, DEEP, d1, id="t50-stress-77-False-8-None-4096-8-qkv8x1+fc18x1")]


@pytest.mark.parametrize("geo,kind,n,concurrent,force,resid,gemm_rows,kernel,ln", [_old(c, 1) for c in _split_cases()] + _split_multi_cases())
def test_every_stage_of_the_split_stream_against_fp64(gpu_lib, monkeypatch, geo, kind, n, concurrent, force, resid, gemm_rows, kernel, ln):
    from video_quierer_amd import _lib
    is_text = geo in SPLIT_TEXT
    cfg = (SPLIT_TEXT if is_text else SPLIT_IMAGE)[geo]
    T = cfg.max_positions if is_text else cfg.tokens
    monkeypatch.delenv("VQ_AMD_RESID", raising=False)
    monkeypatch.delenv("VQ_AMD_GEMM", raising=False)
    if resid:
        monkeypatch.setenv("VQ_AMD_RESID", resid)
    if force:
        monkeypatch.setenv("VQ_AMD_GEMM", str(force))
    rows = n * T
    assert gemm_rows >= rows
    assert S.plan_resid_rows(_lib.load(), cfg, n, concurrent) == (gemm_rows, gemm_rows), (geo, n)
    plan_force = force or (6 if concurrent else 0)          # a concurrent handle plans as GK_AUTO_NO160
    for K in (cfg.hidden, cfg.mlp):                         # out_proj, fc2: the GEMMs that carry the wide residual epilogue
        assert S.plan_kernels(_lib.load(), gemm_rows, cfg.hidden, K, plan_force) == [(kernel, gemm_rows, 0, 1)], (geo, n, K)
    tag = f"{geo} {kind} rows={rows} gemm={kernel}" + (" concurrent" if concurrent else "") + (" resid=f32" if resid else "")
    if ln:
        assert gemm_rows == S.pad_rows(rows)
        tag += " " + S.assert_ln_plans(_lib.load(), cfg, T, n, plan_force, ln)
    full_pass = not (force == DEEP and not is_text)         # (see _split_cases: that forced id refuses the CLS-only GEMMs)
    S.run_split_chain(cfg, is_text, kind, n, concurrent, resid, full_pass, tag)


_CHILD_STATUS = []          # the first child that did not end with status 0: no child is started after it


@pytest.mark.parametrize("tpw", S.TPW_COUNTS)
def test_multi_tile_tiles_per_workgroup_in_a_child(gpu_lib, tpw):
    """Four, two, one and twelve tiles per multi-tile workgroup under the LayerNorm-consuming q|k|v epilogue: both chains above on
    ViT-L's widths (S.TPW_CFG; q|k|v 11 x 12 tiles).  $VQ_AMD_GEMM_TPW is read once per process, so each count runs in a fresh
    child (one at a time next to this process); the child first shows through vq_debug_gemm_plan that the switch took effect.
    After a child that failed, died or ran into its time limit nothing more is started: the remaining counts fail without touching the GPU."""
    import subprocess
    import sys
    assert not _CHILD_STATUS, f"not started: the child for {_CHILD_STATUS[0][0]} tiles per workgroup ended with status {_CHILD_STATUS[0][1]}"
    env = dict(os.environ, VQ_AMD_GEMM="15", VQ_AMD_GEMM_TPW=str(tpw))
    for name in ("VQ_AMD_RESID", "VQ_AMD_ATTN"):
        env.pop(name, None)
    try:
        child = subprocess.run([sys.executable, S.__file__, "tpw-child", str(tpw)], env=env, timeout=240,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:                  # run() has killed the child; a hang stops the remaining counts too
        _CHILD_STATUS.append((tpw, "timeout"))
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(out)
        pytest.fail(f"child for {tpw} tiles per workgroup did not end within {e.timeout:.0f} s:\n{out[-4000:]}")
    print(child.stdout)
    if child.returncode != 0:
        _CHILD_STATUS.append((tpw, child.returncode))
    assert child.returncode == 0, f"child for {tpw} tiles per workgroup ended with status {child.returncode}:\n{child.stdout[-4000:]}"
