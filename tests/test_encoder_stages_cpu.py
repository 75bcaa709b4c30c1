"""The stage bounds of tests/encoder_stage_ref.py are neither wrong nor vacuous (no GPU needed).

For every stage, geometry class and operand type: the float32 emulation of the kernel's stated arithmetic stays within
the derived bound of the fp64 reference, on seeded and on stress inputs, and every mutant of the emulation that applies
to the stage leaves the bound on at least one element.  The stress fixture's promised properties are asserted too.
tests/test_encoder_stages.py then holds the real kernels to the same bounds."""
import functools

import numpy as np
import pytest

import encoder_stage_ref as R
from video_quierer_amd.weights import TextConfig, VitConfig

GEOMETRIES = {      # name -> (tower, config, batch)
    "tile_t50": ("image", VitConfig(image_size=224, patch_size=32, layers=2), 3),
    "stream_t65_patch14": ("image", VitConfig(image_size=112, patch_size=14, layers=2), 2),
    "stream_t257": ("image", VitConfig(image_size=256, patch_size=16, layers=2), 1),
    "text_t77": ("text", TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, layers=2), 4),
}
KINDS = ("seeded", "stress", "lowvar")
DTYPES = ("fp16", "bf16")


@functools.lru_cache(maxsize=None)
def chain(geo, kind, dt):
    tower, cfg, n = GEOMETRIES[geo]
    tw = R.Tower(tower, cfg, R.make_weights(tower, cfg, kind), dt)
    inp = R.make_input(tower, cfg, n)
    return tw, n, inp, R.emu_chain(tw, n, inp)


def attention_mutants(tw):
    """Under the causal mask a key past the sequence end is past every query as well: `padded_key` cannot be told from the
    kernel there (the two conditions are one `if`), so the text tower has the two off-by-one masks instead."""
    return tuple(m for m in R.ATT_MUTANTS if m != "padded_key") + R.CAUSAL_MUTANTS if tw.is_text else R.ATT_MUTANTS


def show(tag, ratios):
    print(tag, "  ".join(f"{s}{l}={r:.3g}" for (s, l), r in ratios.items()))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_emulation_stays_within_every_bound(geo, kind, dt):
    tw, n, inp, runs = chain(geo, kind, dt)
    ratios = R.check_chain(tw, n, inp, runs)
    amb = ratios.pop(("ambiguous", 0))
    if tw.is_text:
        ratios[("pool", tw.layers - 1)] = R.check_pool(tw, runs[-1]["x"][R.eos_rows(inp, tw.cfg)], R.emu_pool(tw, runs[-1]["x"][R.eos_rows(inp, tw.cfg)]))
    else:
        prod, emb = R.emu_product_image(tw, n, runs[-2])
        ratios.update(R.check_product_image(tw, n, runs[-2], prod, emb))
    show(f"{geo} {kind} {dt} (ambiguous fc1 operand elements: {amb})", ratios)
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"emulation leaves the bound at {worst}: {ratios[worst]}"


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_stress_fixture_has_the_promised_properties(geo):
    tw, n, inp, runs = chain(geo, "stress", "fp16")
    pr = R.stress_properties(tw, n, runs)
    print(geo, pr)
    assert pr["spread_hot"] > 200, pr                      # a row whose softmax overflows fp32 without the max subtraction (e^200)
    assert 15 < pr["spread_warm"] < 80, pr
    assert pr["spread_zero_q"] == 0.0, pr                  # q = 0 exactly: uniform softmax
    assert pr["argmax_first_tile"] > 0 and pr["argmax_last_tile"] > 0 and pr["argmax_last_key"] > 0, pr
    assert 1.0 < pr["mean_over_std_median"] < 3.0, pr
    assert pr["preact_max"] > 60 and pr["preact_min"] < -60, pr
    lv = chain(geo, "lowvar", "fp16")
    var = float(np.median(np.asarray(lv[3][0]["x"], np.float64).var(1)))
    assert var < 1e-2, var                                 # eps = 1e-5 is > 0.1 % of such a variance


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_attention_mutants_leave_the_bound(geo, dt):
    tw, n, inp, runs = chain(geo, "stress", dt)
    qkv = runs[1]["qkv"]
    assert R.check_att(tw, n, qkv, runs[1]["att"]) <= 1.0
    for mutant in attention_mutants(tw):
        r = R.check_att(tw, n, qkv, R.emu_attention(qkv, n, tw.T, tw.heads, dt, tw.is_text, mutant))
        print(f"{geo} {dt} attention mutant {mutant}: {r:.3g}")
        assert r > 1.0, f"mutant {mutant} stays within the bound ({r})"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_attention_mutants_on_seeded_inputs(geo, dt):
    """On the easy inputs too, with two exceptions that need the stress fixture.  `no_max`: with logits of a few units exp()
    does not overflow, and without the max subtraction it is the same function.  `padded_key`: the padded key has k = v = 0,
    so it only adds e^(0 - max s) to the denominator: at most 1 / (T + 1) of the output when every logit is near 0, i.e.
    3.9e-3 at T = 257, which IS u16 of bf16 (2^-8); the uniform head of the stress fixture (q = 0, |output| = |mean of V|,
    a bound of u16 times far less than sum p |v|) is where it shows at every T."""
    tw, n, inp, runs = chain(geo, "seeded", dt)
    qkv = runs[1]["qkv"]
    for mutant in attention_mutants(tw):
        if mutant in ("no_max", "padded_key"):
            continue
        r = R.check_att(tw, n, qkv, R.emu_attention(qkv, n, tw.T, tw.heads, dt, tw.is_text, mutant))
        print(f"{geo} {dt} seeded attention mutant {mutant}: {r:.3g}")
        assert r > 1.0, f"mutant {mutant} stays within the bound ({r})"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_folded_gemm_mutants_leave_the_bound(geo, dt):
    """q not pre-scaled, LayerNorm eps x 10 and / 10, GELU constant 1.70.

    eps needs the low-variance fixture: rstd moves by d_eps / (2 (var + eps)); at var = 1 that is 4.5e-5 (x 10) or 4.5e-6
    (/ 10) of the value, under the half ulp of either 16-bit type (2^-12 ... 2^-11 relative in fp16); at var = 2.5e-3 it is
    1.8e-2 and 1.8e-3.

    The GELU constant and LayerNorm-2's eps are shown where the operand xh is OBSERVED (as in the CLS-only last block, whose
    compact h can be read): in the full-row chain the device's 16-bit rounding of x_mid is not observable, and the term
    for ambiguous roundings, rstd sum_k ulp16(x_k) |W'_k| over about 2 e_mid / ulp16 of the K elements, is about
    2 e_mid sqrt(K) rstd ~ 1e-2 of a typical output against the constant's 1.702 / 1.70 - 1 = 1.2e-3."""
    for kind in ("stress", "lowvar"):
        tw, n, inp, runs = chain(geo, kind, dt)
        A, o = runs[0], tw.ops(0)
        ref, bound = R.ln_gemm_ref_bound(A["x"], A["h"], o["w_qkv"], o["c2_qkv"], tw.eps, False, dt)
        om = tw.ops(0, q_prescale=False)
        r = R.max_ratio(R.emu_ln_gemm(A["x"], A["h"], om["w_qkv"], om["c2_qkv"], tw.eps, False, dt), ref, bound)
        print(f"{geo} {kind} {dt} q not pre-scaled: {r:.3g}")
        assert r > 1.0
        x_mid, h_mid = R.emu_residual(A["x"], runs[1]["att"], o["w_out"], o["b_out"], dt)
        ref2, bound2 = R.ln_gemm_ref_bound(x_mid, h_mid, o["w_fc1"], o["c2_fc1"], tw.eps, True, dt)
        assert R.max_ratio(R.emu_ln_gemm(x_mid, h_mid, o["w_fc1"], o["c2_fc1"], tw.eps, True, dt), ref2, bound2) <= 1.0
        og = tw.ops(0, gelu_a=1.70)
        r = R.max_ratio(R.emu_ln_gemm(x_mid, h_mid, og["w_fc1"], og["c2_fc1"], tw.eps, True, dt), ref2, bound2)
        print(f"{geo} {kind} {dt} GELU constant 1.70: {r:.3g}")
        assert r > 1.0
        if kind != "lowvar":
            continue
        for f in (10.0, 0.1):
            r1 = R.max_ratio(R.emu_ln_gemm(A["x"], A["h"], o["w_qkv"], o["c2_qkv"], tw.eps * f, False, dt), ref, bound)
            r2 = R.max_ratio(R.emu_ln_gemm(x_mid, h_mid, o["w_fc1"], o["c2_fc1"], tw.eps * f, True, dt), ref2, bound2)
            print(f"{geo} {dt} eps x {f}: LayerNorm-1 {r1:.3g}, LayerNorm-2 {r2:.3g}")
            assert r1 > 1.0, f"eps x {f} is invisible at LayerNorm 1"
            assert r2 > 1.0, f"eps x {f} is invisible at LayerNorm 2"


@pytest.mark.parametrize("dt", DTYPES)
def test_cls_row_from_the_wrong_image_leaves_the_bound(dt):
    """Caught twice: the compact h is no rounding of the right LayerNorm input, and the CLS rows of x leave the residual bound."""
    tw, n, inp, runs = chain("tile_t50", "stress", dt)
    prod, emb = R.emu_product_image(tw, n, runs[-2], wrong_image=True)
    with pytest.raises(AssertionError, match="compact h is not a 16-bit rounding"):
        R.check_product_image(tw, n, runs[-2], prod, emb)
    T, l = tw.T, tw.layers - 1
    cls = lambda a: np.asarray(a).reshape(n, T, -1)[:, 0]
    r = R.check_resid(tw, l, cls(runs[-2]["x"]), cls(prod["att"]), prod["mlp"], cls(prod["x"]), extra_adds=9)
    print(f"{dt} CLS residual row from the wrong image: {r:.3g}")
    assert r > 1.0


def test_rounding_helpers():
    a = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 2.0 ** -25, 3.0e-39], np.float32)
    assert np.array_equal(R.round16(a, "fp16")[:3], np.array([1.0, 1.0, 1.0 + 2.0 ** -9], np.float32))     # ties to even
    import torch
    t = torch.from_numpy(np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 100)
    assert np.array_equal(R.round16(t.numpy(), "bf16"), t.to(torch.bfloat16).float().numpy())
    assert R.half_ulp16(1.5, "fp16") == 2.0 ** -11 and R.half_ulp16(1.5, "bf16") == 2.0 ** -8
    assert R.half_ulp16(1e-7, "fp16") == 2.0 ** -25                      # subnormal spacing
