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


# ------------------------------------------------------------------- the split residual stream (fp16 + one fp8 byte)
SPLIT_GEOMETRIES = {      # the smallest depths at which the default pass uses all four epilogue modes
    "image_t50_3_blocks": ("image", VitConfig(image_size=224, patch_size=32, layers=3), 3),
    "text_t77_2_blocks": ("text", TextConfig(vocab=520, eos_token_id=519, bos_token_id=518, layers=2), 4),
}


@functools.lru_cache(maxsize=None)
def split_chain(geo, kind, mutant=None):
    tower, cfg, n = SPLIT_GEOMETRIES[geo]
    tw = R.Tower(tower, cfg, R.make_weights(tower, cfg, kind), "fp16")
    inp = R.make_input(tower, cfg, n)
    return tw, n, inp, R.emu_chain_split(tw, n, inp, mutant)


def test_fp8_codec_against_torch():
    import torch
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(want), np.isnan(R.FP8_VALUE)) and np.array_equal(want[~np.isnan(want)], R.FP8_VALUE[~np.isnan(want)])
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.uniform(-448, 448, 20000), rng.uniform(-2.0 ** -5, 2.0 ** -5, 20000), R.FP8_VALUE[:127],
                        (R.FP8_VALUE[:126] + R.FP8_VALUE[1:127]) / 2]).astype(np.float32)      # the last: every tie
    mine = R.fp8_encode(t)
    theirs = torch.from_numpy(t).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    zero = t == 0
    assert np.array_equal(mine[~zero], theirs[~zero]) and np.all((mine[zero] & 0x7F) == 0)
    assert np.array_equal(R.fp8_encode(np.array([449.0, -1e9, np.nan])) & 0x7F, [0x7F] * 3)


def test_pair_bound_is_met_and_attained_in_every_binade():
    """Sound: no fp32 x leaves pair_bound.  Not slack: in every fp16 binade from 2^-14 to 2^15 some x comes within 1 % of it.
    Per binade [2^e, 2^(e+1)) and sign: EVERY fp32 value of four fp16 steps in the middle of the binade, of the two steps at its
    top (where xh is 2^(e+1)) and of the two at its bottom, so every position of x between two fp16 values occurs, ties included."""
    worst = {}
    for e in range(-14, 16):
        step32 = 2.0 ** (e - 23)
        k = np.arange(4 * 8192 + 1, dtype=np.float64)
        x = np.concatenate([2.0 ** e * 1.5 + k * step32, 2.0 ** (e + 1) - k[:2 * 8192 + 1] * step32, 2.0 ** e + k[:2 * 8192 + 1] * step32])
        x = x[x <= 65504.0]
        x = np.concatenate([x, -x]).astype(np.float32)
        assert np.all(np.abs(x.astype(np.float64)) >= 2.0 ** e) and np.all(np.abs(x.astype(np.float64)) <= 2.0 ** (e + 1))
        h, code = R.split16_8(x)
        err = np.abs(R.pair_value(h, code) - x.astype(np.float64))
        inside = np.abs(x.astype(np.float64)) < 2.0 ** (e + 1)
        bound = R.pair_bound(x.astype(np.float64))
        assert np.all(err <= bound), (e, float((err / bound).max()))
        assert len(np.unique(bound[inside])) == 1
        worst[e] = float(err[inside].max() / bound[inside][0])
        assert worst[e] >= 0.99, (e, worst[e])
        # the exact properties the device is held to
        assert np.all(np.abs(R.fp8_decode(code)) / R.XL_SCALE <= R.half_ulp16(h, "fp16")) and not np.any((code & 0x7F) == 0x7F)
    print("max error / pair_bound per binade:", {e: round(r, 4) for e, r in worst.items()})
    # the statements of csrc/encoder_kernels.h: relative to |x|, and where the clamp begins
    assert R.pair_bound(2047.9) == 2.0 ** -6 and R.pair_bound(2048.0) == 0.125
    for e in range(-3, 11):
        assert R.pair_bound(2.0 ** e) == 2.0 ** (e - 16)
    assert all(R.pair_bound(2.0 ** e) == 2.0 ** -19 for e in range(-7, -3)) and R.pair_bound(2.0 ** -8) == 2.0 ** -19
    # fp16's own subnormals: the low byte is zero and the pair is xh
    x = np.linspace(-2.0 ** -14, 2.0 ** -14, 40001).astype(np.float32)
    h, code = R.split16_8(x)
    assert np.all(np.abs(R.pair_value(h, code) - x.astype(np.float64)) <= R.pair_bound(x.astype(np.float64)))


@pytest.mark.parametrize("geo", list(SPLIT_GEOMETRIES))
def test_passthrough_fixture_has_the_promised_properties(geo):
    tw, n, inp, runs = split_chain(geo, "passthrough")
    assert [r["split"] for r in runs] == R.split_forms(tw)[:len(runs)]
    for l in range(tw.layers):                             # zero accumulators: the residual bound is the pair's error + four adds
        o = tw.ops(l)
        assert not o["w_out"].any() and not o["w_fc2"].any()
    pr = R.passthrough_properties(runs)
    print(geo, pr)
    assert min(pr.values()) >= 100, pr
    y = np.abs(np.asarray(runs[1]["y_mid"], np.float64))
    for lo in (2048.0, 8192.0):
        for sign in (1, -1):
            sel = (y >= lo) & (y < 2 * lo) & (np.sign(runs[1]["y_mid"]) == sign)
            assert np.count_nonzero(sel) >= 100, (lo, sign)


@pytest.mark.parametrize("kind", ("passthrough", "stress", "seeded"))
@pytest.mark.parametrize("geo", list(SPLIT_GEOMETRIES))
def test_split_emulation_stays_within_every_bound(geo, kind):
    tw, n, inp, runs = split_chain(geo, kind)
    ratios = R.check_chain(tw, n, inp, runs, split=True)
    amb = ratios.pop(("ambiguous", 0))
    if tw.is_text:
        rows = runs[-1]["x"][R.eos_rows(inp, tw.cfg)]
        ratios[("pool", tw.layers - 1)] = R.check_pool(tw, rows, R.emu_pool(tw, rows))
    else:
        prod, emb = R.emu_product_image(tw, n, runs[-1])
        ratios.update(R.check_product_image(tw, n, runs[-1], prod, emb))
    show(f"split {geo} {kind} (ambiguous fc1 operand elements: {amb})", ratios)
    worst = max(ratios, key=ratios.get)
    assert ratios[worst] <= 1.0, f"emulation leaves the bound at {worst}: {ratios[worst]}"
    if kind == "passthrough":                              # the pair leads the bound, and the emulation comes close to it
        assert max(r for (s, l), r in ratios.items() if s == "resid") > 0.5, ratios


@pytest.mark.parametrize("mutant", R.SPLIT_MUTANTS)
@pytest.mark.parametrize("geo", list(SPLIT_GEOMETRIES))
def test_low_half_mutants_leave_the_residual_bound(geo, mutant):
    tw, n, inp, runs = split_chain(geo, "passthrough", mutant)
    ratios = R.check_chain(tw, n, inp, runs, split=True, exact=False)
    resid = {k: r for k, r in ratios.items() if k[0] == "resid"}
    print(f"{geo} {mutant}:", "  ".join(f"resid{l}={r:.3g}" for (s, l), r in resid.items()))
    assert max(resid.values()) > 1.0, f"mutant {mutant} stays within the residual bound ({resid})"
    if mutant == "no_clamp":                               # the exact properties see this one as well
        with pytest.raises(AssertionError, match="NaN code"):
            R.check_chain(tw, n, inp, runs, split=True)


@pytest.mark.parametrize("kind", ("passthrough", "stress"))
@pytest.mark.parametrize("geo", list(SPLIT_GEOMETRIES))
def test_row_partials_missing_an_8_column_piece_leave_the_bound(geo, kind):
    tw, n, inp, runs = split_chain(geo, kind, R.STATS_MUTANT)
    ratios = R.check_chain(tw, n, inp, runs, split=True, exact=False)
    seen = {k: r for k, r in ratios.items() if k[0] in ("qkv", "mlp")}
    print(f"{geo} {kind} {R.STATS_MUTANT}:", "  ".join(f"{s}{l}={r:.3g}" for (s, l), r in seen.items()))
    assert ratios[("qkv", 0)] <= 1.0                       # block 0's q|k|v has the embedding kernel's partials
    assert ratios[("mlp", 0)] > 1.0 and ratios[("qkv", 1)] > 1.0, seen


def test_rounding_helpers():
    a = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 2.0 ** -25, 3.0e-39], np.float32)
    assert np.array_equal(R.round16(a, "fp16")[:3], np.array([1.0, 1.0, 1.0 + 2.0 ** -9], np.float32))     # ties to even
    import torch
    t = torch.from_numpy(np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 100)
    assert np.array_equal(R.round16(t.numpy(), "bf16"), t.to(torch.bfloat16).float().numpy())
    assert R.half_ulp16(1.5, "fp16") == 2.0 ** -11 and R.half_ulp16(1.5, "bf16") == 2.0 ** -8
    assert R.half_ulp16(1e-7, "fp16") == 2.0 ** -25                      # subnormal spacing
