"""Stage-by-stage parity helpers for the two encoder towers (tests/test_encoder_stages*.py).

For every stage of a transformer block this module has three things:

* a numpy fp64 REFERENCE written from the mathematical definition, evaluated on the inputs the device
  itself had (the activations are the device buffers as read; the 16-bit weights are rebuilt from the fp32
  tensors the way the host upload defines them: W * scale * gamma in fp32, round to nearest even);
* a per-element BOUND on |device - reference|, a sum of named terms, each the worst case of one rounding
  the kernel is documented to make.  Nothing in a bound was fitted to what a kernel returns;
* an EMULATION of the kernel's stated arithmetic in numpy float32 with the same 16-bit roundings, and
  MUTANTS of it (a dropped key, a wrong constant ...).  tests/test_encoder_stages_cpu.py shows that the
  emulation stays inside every bound and that every mutant leaves it: the bounds are neither wrong nor
  vacuous.

The default pass holds the residual stream between its residual epilogues as a PAIR: xh = fp16(x) and one fp8 byte
xl = e4m3((x - xh) 512).  pair_value / pair_bound, the split-aware check_chain (runs that carry "split" and "xl"),
emu_chain_split with its mutants and the `passthrough` fixture are about that form.

Notation of the bounds: u32 = 2^-24 is the unit roundoff of fp32, u16 that of the 16-bit operand type
(2^-11 fp16, 2^-8 bf16).  A sum of K terms accumulated in fp32 in ANY order is within (K - 1) u32 sum|a||w|
of the exact sum; C0 covers the handful of further roundings around it.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
U16 = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
MANT = {"fp16": 10, "bf16": 7}                   # explicit mantissa bits
EMIN = {"fp16": -14, "bf16": -126}               # exponent of the smallest normal number
# half of the smallest value the probability format holds apart from zero: fp16 has subnormals down to 2^-24; bf16 has
# fp32's exponent range, where the hardware exponential flushes below 2^-126
PSUB = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -126}
C0 = 4
LOG2E = float(np.log2(np.e))
GELU_A = 1.702                                   # quick_gelu(z) = z * sigmoid(1.702 z)
SILU_LIP = 1.1                                   # sup |d/dt (t sigmoid(t))| = 1.0998...
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)  # CLIPImageProcessor image_mean / image_std
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
KEY_TILE = 64                                    # key step of the streaming attention kernels

f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------------- number formats
def round16(a, dt):
    """fp32 -> fp16 / bf16 by round to nearest even -> fp32."""
    a = np.ascontiguousarray(a, dtype=f32)
    if dt == "fp16":
        with np.errstate(over="ignore"):
            return a.astype(np.float16).astype(f32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(f32)


def half_ulp16(mag, dt):
    """Half the spacing of the 16-bit format at magnitude `mag` (the error of one rounding to nearest)."""
    mag = np.maximum(np.abs(np.asarray(mag, f64)), 2.0 ** -200)
    e = np.frexp(mag)[1] - 1                      # floor(log2 mag)
    return np.ldexp(1.0, np.maximum(e, EMIN[dt]) - MANT[dt] - 1)


def with_output_rounding(ref, pre, dt):
    """pre = bound on the value before its rounding to 16 bits; the rounding adds half an ulp where that value may lie."""
    return pre + half_ulp16(np.abs(ref) + pre, dt)


def max_ratio(dev, ref, bound):
    """max |dev - ref| / bound over EVERY element; a NaN or infinity anywhere counts as infinitely far."""
    err = np.abs(np.asarray(dev, f64) - ref)
    r = err / bound
    r[~np.isfinite(err)] = np.inf
    return float(r.max())


# ------------------------------------------------------------------------- the split residual stream: fp16 + one fp8 byte
XL_SCALE, FP8_MAX = 512.0, 448.0


def _fp8_table():
    """The 256 values of OCP e4m3 ("fn": no infinities, S.1111.111 is NaN) from the definition: 4 exponent bits with bias 7,
    3 mantissa bits, subnormals m 2^-9 below 2^-6."""
    code = np.arange(256)
    e, m = (code >> 3) & 15, code & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2(e - 7.0))
    v = np.where((code & 0x7F) == 0x7F, np.nan, v)
    return np.where(code >= 128, -v, v)


FP8_VALUE = _fp8_table()
_FP8_POS = FP8_VALUE[:127]                       # 0 ... 448, ascending


def fp8_encode(t):
    """float -> e4m3 code by round to nearest, ties to the even code; beyond +-448 (and NaN) -> the NaN code 0x7F | sign."""
    t = np.asarray(t, f64)
    a = np.abs(t)
    hi = np.clip(np.searchsorted(_FP8_POS, a), 1, 126)
    lo = hi - 1
    dl, dh = a - _FP8_POS[lo], _FP8_POS[hi] - a
    code = np.where((dl < dh) | ((dl == dh) & (lo % 2 == 0)), lo, hi)
    code = np.where((a > FP8_MAX) | np.isnan(a), 0x7F, code)
    return (code + np.where(np.signbit(t), 128, 0)).astype(np.uint8)


def fp8_decode(code):
    """Codes 0..255 (any numeric array, as debug_read returns them) -> fp64 values."""
    return FP8_VALUE[np.asarray(code).astype(np.int64)]


def pair_value(h, xl_bytes):
    """What a residual epilogue reads from the split stream: the fp16 value + the decoded byte / 512, in fp64.  (The device adds the
    two in fp32, which is exact: the sum spans fewer than 24 bits.)"""
    return np.asarray(h, f64) + fp8_decode(xl_bytes) / XL_SCALE


def pair_bound(x):
    """Bound on |pair_value - x| for an fp32 x stored as xh = fp16(x), xl = e4m3(clamp((x - xh) 512, +-448)).

    r = x - xh is exact in fp32 and |r| <= hu = half_ulp16(x) = 2^(e-11) in the binade [2^e, 2^(e+1)) of x (at the top of a
    binade xh may be 2^(e+1), still within hu).  t = 512 r is exact and |t| <= T = 2^(e-2).  The error is that of e4m3 on t, / 512:
      normal     |t| in [2^k, 2^(k+1)), k >= -6, has step 2^(k-3): half a step is 2^(k-4).  The largest binade t reaches below
                 T is k = e - 3 (t = T itself is a power of two, exact), so the error of t is <= 2^(e-7) = 2^-5 (512 hu): 2^-5 hu;
      subnormal  below 2^-6 the step is 2^-9 whatever t is: half a step / 512 = 2^-19.  This is the larger of the two for e <= -4,
                 where T <= 2^-6;
      flush      for e <= -8, T <= 2^-10 is itself no more than half the subnormal step: t rounds to 0 and the error is |r| <= hu
                 (< 2^-19), which also covers fp16's own subnormals;
      clamp      |t| > 448 is stored as 448: the error is |r| - 448 / 512 <= hu - 0.875, positive from e = 11 (|x| >= 2048,
                 hu = 1) on; half an ulp in [1024, 2048) is 0.5 < 0.875.
    The binade sweep of tests/test_encoder_stages_cpu.py shows each binade attains it."""
    hu = half_ulp16(x, "fp16")
    return np.maximum(np.minimum(np.maximum(2.0 ** -5 * hu, 2.0 ** -19), hu), hu - FP8_MAX / XL_SCALE)


def split16_8(y, scale=XL_SCALE, clamp=True):
    """fp32 y -> (xh as fp32, xl codes) the way the residual epilogue states it: xh = fp16(y), r = y - xh,
    xl = e4m3(med3(r * 512, -448, 448))."""
    y = np.ascontiguousarray(y, f32)
    h = round16(y, "fp16")
    with np.errstate(invalid="ignore"):
        t = (y - h) * f32(scale)
    if clamp:
        t = np.clip(t, f32(-FP8_MAX), f32(FP8_MAX))
    return h, fp8_encode(t)


# ------------------------------------------------------------------------------------- weights as the host uploads them
def fold_ln(Wt, gamma, beta, bias, scale, dt):
    """LayerNorm folded into the GEMM that consumes it: W' = 16-bit(W * scale * gamma) (fp32 products), and
    c2 = scale (sum_k beta_k W_nk + bias_n) in fp64 (the upload rounds it to fp32: `c2` is bounded with one u32)."""
    w16 = round16((Wt.astype(f32) * f32(scale)) * gamma.astype(f32)[None, :], dt)
    c2 = ((beta.astype(f64)[None, :] * Wt.astype(f64)).sum(1) + bias.astype(f64)) * float(f32(scale))
    return w16, c2


def layer_operands(W, prefix, l, hidden, heads, dt, gelu_a=GELU_A, q_prescale=True):
    """The 16-bit GEMM operands and fp64 constants of block l.  gelu_a / q_prescale exist for the mutants."""
    p = f"{prefix}.encoder.layers.{l}."
    g1, b1 = W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"]
    g2, b2 = W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"]
    qscale = float(hidden // heads) ** -0.5 if q_prescale else 1.0
    parts = [fold_ln(W[p + f"self_attn.{n}_proj.weight"], g1, b1, W[p + f"self_attn.{n}_proj.bias"], s, dt)
             for n, s in (("q", qscale), ("k", 1.0), ("v", 1.0))]
    c = f32(gelu_a * LOG2E)
    w_fc1, c2_fc1 = fold_ln(W[p + "mlp.fc1.weight"], g2, b2, W[p + "mlp.fc1.bias"], c, dt)
    return {
        "w_qkv": np.concatenate([w for w, _ in parts]), "c2_qkv": np.concatenate([c2 for _, c2 in parts]),
        "w_out": round16(W[p + "self_attn.out_proj.weight"], dt), "b_out": W[p + "self_attn.out_proj.bias"].astype(f64),
        "w_fc1": w_fc1, "c2_fc1": c2_fc1,
        "w_fc2": round16(W[p + "mlp.fc2.weight"].astype(f32) * (f32(1.0) / c), dt), "b_fc2": W[p + "mlp.fc2.bias"].astype(f64),
    }


def patch_operands(W, cfg, dt):
    """Patch weights with ToTensor (/255) and Normalize ((x - mean) / std) folded in, for pixels stored as (p - 128):
    W' = W / (255 std_c), bias = sum W (128/255 - mean_c) / std_c.  fp16 weights carry the power of two 2^s, s =
    floor(log2(16000 / max|W'|)) clamped to [0, 24], that lifts them out of fp16's subnormal range; the epilogue
    multiplies by 2^-s (exact), so the effective weight is 16-bit(W' 2^s) 2^-s."""
    P, H = cfg.patch_size, cfg.hidden
    wp = W["vision_model.embeddings.patch_embedding.weight"].astype(f64).reshape(H, 3, P * P)
    std = np.array(CLIP_STD)[None, :, None]
    mean = np.array(CLIP_MEAN)[None, :, None]
    shift = 0
    if dt == "fp16":
        amax = np.abs(wp / (255.0 * std)).max()
        if amax > 0 and np.isfinite(amax):
            shift = int(min(24, max(0, np.floor(np.log2(16000.0 / amax)))))
    w16 = round16((wp * 2.0 ** shift / (255.0 * std)).astype(f32), dt).astype(f64) * 2.0 ** -shift
    bias = (wp * (128.0 / 255.0 - mean) / std).sum((1, 2))
    return w16.reshape(H, 3 * P * P), bias


# ---------------------------------------------------------------------------------------------- references + bounds
def layernorm_ref_bound(e, de, g, b, eps):
    """y = (e - mu) rstd g + b in fp64, and the bound for a two-pass fp32 LayerNorm whose input is within `de` of e.
    Terms: d_mu (input error + fp32 sum of H terms), d_var (centred sum of squares), the relative error of rstd
    (exact expression in d_var, + 3 u32 for the add of eps and the reciprocal square root), 4 roundings of the affine tail."""
    e = np.asarray(e, f64)
    g, b = g.astype(f64)[None, :], b.astype(f64)[None, :]
    H = e.shape[1]
    mu = e.mean(1, keepdims=True)
    cen = e - mu
    var = (cen * cen).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = cen * rstd * g + b
    de = np.broadcast_to(np.asarray(de, f64), e.shape)
    d_mu = de.mean(1, keepdims=True) + (H + 2) * U32 * np.abs(e).mean(1, keepdims=True)
    d_var = 2.0 * (np.abs(cen) * (de + d_mu + U32 * np.abs(cen))).mean(1, keepdims=True) + (H + 4) * U32 * var
    rel = 1.0 / np.sqrt(np.maximum(1.0 - d_var / (var + eps), 1e-300)) - 1.0 + 3 * U32
    dy = np.abs(g) * rstd * (de + d_mu + U32 * np.abs(cen)) + np.abs(y - b) * rel + 4 * U32 * (np.abs(y - b) + np.abs(b))
    return y, dy


def patches_of(frames, cfg, swap_rb):
    """uint8 [n,S,S,3] -> (pixel - 128) patch rows [n * patches, 3 P P], K ordered (c, ky, kx) like Conv2d's weight."""
    n, P, G = frames.shape[0], cfg.patch_size, cfg.grid
    px = frames.astype(f64) - 128.0
    if swap_rb:
        px = px[..., ::-1]
    return px.reshape(n, G, P, G, P, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n * G * G, 3 * P * P)


def embed_image_ref_bound(frames, W, cfg, dt, swap_rb):
    """x after the embedding stage: patchify, patch GEMM + folded bias + position embedding, CLS row, pre-LayerNorm.
    Input-side terms: fp32 accumulation over K = 3 P^2 of exact 16-bit products, 3 roundings of the epilogue
    (unscale is exact); the CLS row is one fp32 add."""
    H, T, n = cfg.hidden, cfg.tokens, frames.shape[0]
    w16, bias = patch_operands(W, cfg, dt)
    pt = patches_of(frames, cfg, swap_rb)
    pos = W["vision_model.embeddings.position_embedding.weight"].astype(f64)
    S = pt @ w16.T
    bias32 = bias.astype(f32).astype(f64)
    e = np.empty((n, T, H))
    de = np.empty((n, T, H))
    e[:, 1:] = (S + bias32[None, :]).reshape(n, T - 1, H) + pos[None, 1:]
    acc = (pt.shape[1] + C0) * U32 * (np.abs(pt) @ np.abs(w16).T) + U32 * np.abs(bias)[None, :]
    de[:, 1:] = acc.reshape(n, T - 1, H) + 3 * U32 * ((np.abs(S) + np.abs(bias)[None, :]).reshape(n, T - 1, H) + np.abs(pos[None, 1:]))
    cls = W["vision_model.embeddings.class_embedding"].astype(f64) + pos[0]
    e[:, 0] = cls
    de[:, 0] = U32 * np.abs(cls)
    y, dy = layernorm_ref_bound(e.reshape(n * T, H), de.reshape(n * T, H), W["vision_model.pre_layrnorm.weight"],
                                W["vision_model.pre_layrnorm.bias"], cfg.ln_eps)
    return y, dy + U32 * np.abs(y)


def embed_text_ref_bound(ids, W, cfg):
    """x = token_embedding[id] + position_embedding[t]: one fp32 add."""
    ids = np.asarray(ids)
    n, L = ids.shape
    T = cfg.max_positions
    full = np.full((n, T), cfg.eos_token_id, dtype=np.int64)      # the host pads every sequence with eos to max_positions
    full[:, :L] = ids
    x = W["text_model.embeddings.token_embedding.weight"].astype(f64)[full] + \
        W["text_model.embeddings.position_embedding.weight"].astype(f64)[None, :T]
    x = x.reshape(n * T, cfg.hidden)
    return x, U32 * np.abs(x) + 2.0 ** -150


def ln_gemm_ref_bound(x, xh, w16, c2, eps, gelu, dt_out, x_err=None, amb_ulp=None):
    """The GEMM with the LayerNorm in front of it folded in (q|k|v and fc1):
        y = rstd sum_k (xh_k - mean) W'_nk + c2_n,   [g = y / (1 + 2^-y) for fc1: y already carries c = 1.702 log2 e]
    mean and rstd from the fp32 x in fp64, xh the 16-bit operand.  The device evaluates rstd (acc - mean c1) + c2 with
    mean = s1 / H, var = s2 / H - mean^2 from fp32 partial sums.  Named terms:
      t_acc   fp32 accumulation of sum_k xh W'                       (H + C0) u32 rstd sum|xh||W'|
      t_mean  error of mean (fp32 sum of H terms; x_err if x itself is only known to x_err) times rstd |c1|;
              + 2 u32 |mean| for c1 rounded to fp32 and the product mean c1
      t_rstd  |y - c2| times the relative error of rstd, from d_var = d(E x^2) + 2|mean| d_mean + roundings of
              mean^2 and of the subtraction: this is where E[x^2] - E[x]^2 loses digits once |mean| >> std
      t_epi   3 roundings of the epilogue at the magnitudes it handles;  t_c2  c2 rounded to fp32
      t_amb   per ambiguous operand element (its 16-bit rounding not determined by the fp64 x): ulp16 |W'| rstd
    GELU: |dg| <= 1.1 |dy| (Lipschitz constant of t sigmoid(t)) + 6 u32 |g| (v_exp_f32 and v_rcp_f32 at 1 ulp = 2 u32
    each, the add and the multiply).  Then half an ulp of the 16-bit output."""
    x, xh, w, c2 = np.asarray(x, f64), np.asarray(xh, f64), np.asarray(w16, f64), np.asarray(c2, f64)[None, :]
    H = x.shape[1]
    mean = x.mean(1, keepdims=True)
    ex2 = (x * x).mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    c1 = w.sum(1)[None, :]
    S = xh @ w.T
    y = rstd * (S - mean * c1) + c2
    t_acc = (H + C0) * U32 * rstd * (np.abs(xh) @ np.abs(w).T)
    d_mean = (H + 2) * U32 * np.abs(x).mean(1, keepdims=True)
    d_ex2 = (H + 2) * U32 * ex2
    if x_err is not None:
        d_mean = d_mean + x_err.mean(1, keepdims=True)
        d_ex2 = d_ex2 + 2.0 * (np.abs(x) * x_err).mean(1, keepdims=True)
    d_var = d_ex2 + 2.0 * np.abs(mean) * d_mean + U32 * mean ** 2 + U32 * (ex2 + mean ** 2)
    rel = 1.0 / np.sqrt(np.maximum(1.0 - d_var / (var + eps), 1e-300)) - 1.0 + 3 * U32
    t_mean = rstd * np.abs(c1) * (d_mean + 2 * U32 * np.abs(mean))
    t_rstd = np.abs(y - c2) * rel
    t_epi = 3 * U32 * (rstd * (np.abs(S) + np.abs(mean) * np.abs(c1)) + np.abs(c2))
    t_c2 = U32 * np.abs(c2)
    by = t_acc + t_mean + t_rstd + t_epi + t_c2
    if amb_ulp is not None:
        by = by + rstd * (amb_ulp @ np.abs(w).T)
    if not gelu:
        return y, with_output_rounding(y, by, dt_out)
    with np.errstate(over="ignore"):
        g = y / (1.0 + np.exp2(-y))
    return g, with_output_rounding(g, SILU_LIP * by + 6 * U32 * np.abs(g), dt_out)


def split_heads(qkv, n, T, heads):
    a = np.asarray(qkv).reshape(n, T, 3, heads, 64).transpose(2, 0, 3, 1, 4)      # [3][n][heads][T][64]
    return a[0], a[1], a[2]


def attention_ref_bound(qkv, n, T, heads, dt, causal):
    """Softmax attention per (image, head) in fp64 on the 16-bit q | k | v the device read (q arrives pre-scaled).
    With p_j = exp(s_j - max s), l = sum p, o = sum p_j v_j / l and M = sum p_j |v_j| / l, the terms are
      t_s    score error ds_j = (64 + C0) u32 sum_d |q_d||k_jd|  (fp32 accumulation over the head dimension)
             + 4 u32 (|s_j| + |max s|)  (the scaling by log2 e and the subtraction of the max, in fp32);
             it moves o by at most sum_j p_j ds_j |v_j| / l + |o| sum_j p_j ds_j / l  (numerator and denominator)
      t_exp  8 u32 (M + |o|): v_exp_f32 at 1 ulp on p, the rescale factors, v_rcp_f32 / the division, the final product
      t_p16  ONE rounding of each probability to the 16-bit operand type: u16 M in the numerator, and u16 |o| because the
             single-tile and the workgroup streaming kernels take the denominator from the ROUNDED probabilities
      t_sub  fp16 probabilities below 2^-14 of the running maximum are subnormal: absolute error 2^-25 each
             (bf16: the exponential's flush at 2^-126) -> PSUB sum_j |v_j| / l
      t_acc  fp32 accumulation of P V over the keys (and one rescale per key step): (T + C0) u32 M
    then half an ulp of the 16-bit output."""
    q, k, v = (a.astype(f64) for a in split_heads(qkv, n, T, heads))
    s = q @ k.transpose(0, 1, 3, 2)
    sabs = np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)
    valid = np.tril(np.ones((T, T), bool)) if causal else np.ones((T, T), bool)
    s = np.where(valid, s, -np.inf)
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    o = (p @ v) / l
    av = np.abs(v)
    M = (p @ av) / l
    ds = np.where(valid, (64 + C0) * U32 * sabs + 4 * U32 * (np.abs(np.where(valid, s, 0.0)) + np.abs(m)), 0.0)
    pd = p * ds
    t_s = (pd @ av) / l + np.abs(o) * pd.sum(-1, keepdims=True) / l
    t_exp = 8 * U32 * (M + np.abs(o))
    t_p16 = U16[dt] * (M + np.abs(o))
    vsum = np.cumsum(av, axis=2) if causal else np.broadcast_to(av.sum(2, keepdims=True), av.shape)
    t_sub = PSUB[dt] * vsum / l
    t_acc = (T + C0) * U32 * M
    pre = t_s + t_exp + t_p16 + t_sub + t_acc
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(n * T, heads * 64)
    o, pre = back(o), back(pre)
    return o, with_output_rounding(o, pre, dt), {"p": p, "s": s}


def residual_ref_bound(x, a1, w1, b1, a2=None, w2=None, b2=None, extra_adds=0):
    """x + a1 W1^T + b1 [+ a2 W2^T + b2] in fp64; both GEMM operands are 16-bit values known exactly.  Terms: fp32
    accumulation of each GEMM, (K + C0) u32 sum|a||w|, and one u32 of the running magnitude per fp32 add of the
    epilogues (2 per GEMM; `extra_adds` more for the split-K reduce)."""
    x, a1, w1 = np.asarray(x, f64), np.asarray(a1, f64), np.asarray(w1, f64)
    S1 = a1 @ w1.T
    ref = x + S1 + b1[None, :]
    mag = np.abs(x) + np.abs(S1) + np.abs(b1)[None, :]
    bound = (a1.shape[1] + C0) * U32 * (np.abs(a1) @ np.abs(w1).T)
    adds = 2 + extra_adds
    if a2 is not None:
        a2, w2 = np.asarray(a2, f64), np.asarray(w2, f64)
        S2 = a2 @ w2.T
        ref = ref + S2 + b2[None, :]
        mag = mag + np.abs(S2) + np.abs(b2)[None, :]
        bound = bound + (a2.shape[1] + C0) * U32 * (np.abs(a2) @ np.abs(w2).T)
        adds += 2
    return ref, bound + adds * U32 * mag


def ambiguous_rounding(x_ref, x_err, dt):
    """The device rounds ITS fp32 x (within x_err of x_ref) to 16 bits.  Returns (xh, amb): xh = 16-bit(x_ref), and amb =
    the distance between the 16-bit neighbours the device may have chosen instead, 0 where every value within x_err of
    x_ref rounds to the same number."""
    e = x_err * (1.0 + 2.0 ** -20) + 2.0 * U32 * np.abs(x_ref)        # + the fp64 -> fp32 conversions below
    lo, hi = round16((x_ref - e).astype(f32), dt), round16((x_ref + e).astype(f32), dt)
    return round16(x_ref.astype(f32), dt).astype(f64), (hi.astype(f64) - lo.astype(f64))


def pool_ref_bound(xrows, g, b, wproj, eps):
    """post-LayerNorm -> projection (fp32 weights) -> x / ||x||, all in fp32 on the device.  Terms: the LayerNorm bound,
    carried through |W|; fp32 accumulation over H; the norm's error (fp32 sum of D squares, square root) and the division."""
    xn, dxn = layernorm_ref_bound(xrows, 0.0, g, b, eps)
    w = wproj.astype(f64)
    H, D = w.shape[1], w.shape[0]
    f = xn @ w.T
    df = dxn @ np.abs(w).T + (H + C0) * U32 * (np.abs(xn) @ np.abs(w).T)
    nrm = np.sqrt((f * f).sum(1, keepdims=True))
    e = f / nrm
    dn = (df * np.abs(f)).sum(1, keepdims=True) / nrm + (D + 4) * U32 * nrm
    return e, df / nrm + np.abs(e) * dn / nrm + 3 * U32 * np.abs(e)


# ------------------------------------------------------------------------------------------------- stage checks
class Tower:
    """What the checks need to know about one tower: names, geometry, operands."""

    def __init__(self, kind, cfg, W, dt):
        self.kind, self.cfg, self.W, self.dt = kind, cfg, W, dt
        self.is_text = kind == "text"
        self.prefix = "text_model" if self.is_text else "vision_model"
        self.T = cfg.max_positions if self.is_text else cfg.tokens
        self.H, self.heads, self.eps, self.layers = cfg.hidden, cfg.heads, cfg.ln_eps, cfg.layers
        self._ops = {}

    def ops(self, l, **mut):
        key = (l, tuple(sorted(mut.items())))
        if key not in self._ops:
            self._ops[key] = layer_operands(self.W, self.prefix, l, self.H, self.heads, self.dt, **mut)
        return self._ops[key]

    def post(self):
        W = self.W
        if self.is_text:
            return W["text_model.final_layer_norm.weight"], W["text_model.final_layer_norm.bias"], W["text_projection.weight"]
        return W["vision_model.post_layernorm.weight"], W["vision_model.post_layernorm.bias"], W["visual_projection.weight"]


def check_embed(tw, inp, x, swap_rb=True):
    ref, bound = embed_text_ref_bound(inp, tw.W, tw.cfg) if tw.is_text else embed_image_ref_bound(inp, tw.W, tw.cfg, tw.dt, swap_rb)
    return max_ratio(x, ref, bound)


def check_h(tw, x, h):
    """h is the 16-bit rounding of x, bit for bit (returned as the number of elements that differ)."""
    return int(np.count_nonzero(round16(x, tw.dt).view(np.uint32) != np.ascontiguousarray(h, f32).view(np.uint32)))


def check_pair(r):
    """The exact properties of a stream stored split, over every element: h is fp16, |xl| <= half an fp16 ulp of h, no NaN code."""
    h, code = np.ascontiguousarray(r["h"], f32), np.asarray(r["xl"]).astype(np.int64)
    assert np.array_equal(round16(h, "fp16").view(np.uint32), h.view(np.uint32)), "xh of the split stream is not fp16"
    bad = int(np.count_nonzero((code & 0x7F) == 0x7F))
    assert bad == 0, f"{bad} bytes of xl are the fp8 NaN code (an unclamped conversion)"
    bad = int(np.count_nonzero(np.abs(fp8_decode(code)) / XL_SCALE > half_ulp16(h, "fp16")))
    assert bad == 0, f"|xl| exceeds half an fp16 ulp of xh in {bad} elements"


def stream_of(r):
    """(x, x_err) of a run: the value the next residual epilogue READS (exactly: the pair's sum where the stream is split, else the
    fp32 x), and how far the fp32 value the producer took its row statistics from may lie from it (None: not at all).  That value
    rounds to xh, so its binade is that of the larger of |pair| and |xh|."""
    if not r.get("split"):
        return np.asarray(r["x"], f64), None
    x = pair_value(r["h"], r["xl"])
    return x, pair_bound(np.maximum(np.abs(x), np.abs(np.asarray(r["h"], f64))))


def check_qkv(tw, l, x_a, h_a, qkv_b, x_err=None):
    o = tw.ops(l)
    ref, bound = ln_gemm_ref_bound(x_a, h_a, o["w_qkv"], o["c2_qkv"], tw.eps, False, tw.dt, x_err=x_err)
    return max_ratio(qkv_b, ref, bound)


def check_att(tw, n, qkv_b, att_b):
    ref, bound, _ = attention_ref_bound(qkv_b, n, tw.T, tw.heads, tw.dt, tw.is_text)
    return max_ratio(att_b, ref, bound)


def check_mlp(tw, l, x_a, att_b, mlp_b):
    """Returns (ratio, number of ambiguous operand elements)."""
    o = tw.ops(l)
    x_mid, e_mid = residual_ref_bound(x_a, att_b, o["w_out"], o["b_out"])
    xh, amb = ambiguous_rounding(x_mid, e_mid, tw.dt)
    ref, bound = ln_gemm_ref_bound(x_mid, xh, o["w_fc1"], o["c2_fc1"], tw.eps, True, tw.dt, x_err=e_mid, amb_ulp=amb)
    return max_ratio(mlp_b, ref, bound), int(np.count_nonzero(amb))


def check_resid(tw, l, x_a, att_b, mlp_b, x_b, extra_adds=0, split_mid=False, split_out=False):
    """split_mid: x_mid went from out_proj to fc2 as a pair, so fc2 read a value within pair_bound(x_mid) of what out_proj computed.
    split_out: x_b is the pair the block's output was stored as, within pair_bound of what fc2 computed.  Each is one named term,
    taken at the largest magnitude the value may have (pair_bound does not decrease with |x|)."""
    o = tw.ops(l)
    ref, bound = residual_ref_bound(x_a, att_b, o["w_out"], o["b_out"], mlp_b, o["w_fc2"], o["b_fc2"], extra_adds)
    if split_mid:
        x_mid, e_mid = residual_ref_bound(x_a, att_b, o["w_out"], o["b_out"])
        bound = bound + pair_bound(np.abs(x_mid) + e_mid)
    if split_out:
        bound = bound + pair_bound(np.abs(ref) + bound)
    return max_ratio(x_b, ref, bound)


def check_pool(tw, xrows, emb):
    g, b, wp = tw.post()
    ref, bound = pool_ref_bound(xrows, g, b, wp, tw.eps)
    return max_ratio(emb, ref, bound)


def eos_rows(ids, cfg):
    """Pooling row of every sequence: the first position holding eos_token_id (position 0 if none)."""
    ids = np.asarray(ids)
    hit = ids == cfg.eos_token_id
    pos = np.where(hit.any(1), hit.argmax(1), 0)
    return np.arange(ids.shape[0]) * cfg.max_positions + pos


def check_chain(tw, n, inp, runs, swap_rb=True, split=False, exact=True):
    """runs[k] = {"x", "h", "qkv", "att", "mlp"} read after a pass limited to k blocks (k = 0 .. layers; for k = 0 only x and
    h mean anything).  Returns {(stage, layer): ratio}; raises AssertionError for a broken bit-exact property.

    split: the passes held the stream as the default pass does.  A run then also has "split" (the form it left the stream in) and
    "xl"; where "split" is set the block input and output are the pair (x is stale there), and every x_mid crossed from out_proj
    to fc2 as a pair.  exact=False skips the bit-exact properties (for mutants that are to be caught by a bound)."""
    out = {("embed", 0): check_embed(tw, inp, runs[0]["x"], swap_rb)}
    amb_total = 0
    for l in range(len(runs) - 1):
        A, B = runs[l], runs[l + 1]
        for r, tag in ((A, "A"), (B, "B")):
            if not exact:
                continue
            if r.get("split"):
                check_pair(r)
                continue
            bad = check_h(tw, r["x"], r["h"])
            assert bad == 0, f"h is not the 16-bit rounding of x in {bad} elements (block {l}, run {tag})"
        xa, xa_err = stream_of(A)
        xb, _ = stream_of(B)
        out[("qkv", l)] = check_qkv(tw, l, xa, A["h"], B["qkv"], xa_err)
        out[("att", l)] = check_att(tw, n, B["qkv"], B["att"])
        out[("mlp", l)], amb = check_mlp(tw, l, xa, B["att"], B["mlp"])
        amb_total += amb
        out[("resid", l)] = check_resid(tw, l, xa, B["att"], B["mlp"], xb, split_mid=split, split_out=bool(B.get("split")))
    out[("ambiguous", 0)] = amb_total
    return out


def split_forms(tw, prune_last=True):
    """The form the default pass leaves the stream in after k = 0 .. layers blocks (True: the pair): fp32 from the embedding, the
    pair behind every full-row block except the last one in front of a reader of the fp32 x - the pooling head, or the CLS-only
    last block of the image tower, which itself keeps the fp32 x."""
    cls = prune_last and not tw.is_text
    last_full = tw.layers - 1 if cls else tw.layers          # blocks that run on every row
    return [0 < k < last_full for k in range(tw.layers + 1)]


def check_product_image(tw, n, prev, prod, emb):
    """The CLS-only last block.  prev = run limited to layers - 1 blocks; prod = buffers after a full pass with the fp32
    residual stream: x [n T rows], att [n T rows], h and mlp COMPACT [n rows].  The non-CLS rows of x must be untouched."""
    T, l = tw.T, tw.layers - 1
    xp, x = np.asarray(prev["x"]).reshape(n, T, -1), np.asarray(prod["x"]).reshape(n, T, -1)
    assert np.array_equal(xp[:, 1:].view(np.uint32), x[:, 1:].view(np.uint32)), "the CLS-only last block changed a non-CLS row of x"
    att_cls = np.asarray(prod["att"]).reshape(n, T, -1)[:, 0]
    o = tw.ops(l)
    out = {}
    # x_cls = x_prev_cls + att_cls W_out + b_out + mlp W_fc2' + b_fc2 (split-K: 8 partial planes summed in order, + the residual add)
    out[("cls_resid", l)] = check_resid(tw, l, xp[:, 0], att_cls, prod["mlp"], x[:, 0], extra_adds=9)
    # compact h = 16-bit(x_mid of the CLS rows): not observable in fp32, so checked through the ambiguity analysis
    x_mid, e_mid = residual_ref_bound(xp[:, 0], att_cls, o["w_out"], o["b_out"])
    xh, amb = ambiguous_rounding(x_mid, e_mid, tw.dt)
    h = np.asarray(prod["h"], f64)
    bad = int(np.count_nonzero(np.abs(h - xh) > amb))
    assert bad == 0, f"compact h is not a 16-bit rounding of the CLS rows' LayerNorm input in {bad} elements"
    ref, bound = ln_gemm_ref_bound(x_mid, h, o["w_fc1"], o["c2_fc1"], tw.eps, True, tw.dt, x_err=e_mid)
    out[("cls_mlp", l)] = max_ratio(prod["mlp"], ref, bound)
    out[("pool", l)] = check_pool(tw, x[:, 0], emb)
    return out


# ------------------------------------------------------------------------------- float32 emulation of the kernels
def emu_layernorm(e, g, b, eps):
    e = e.astype(f32)
    mu = e.mean(1, dtype=f32, keepdims=True)
    cen = e - mu
    var = (cen * cen).mean(1, dtype=f32, keepdims=True)
    return cen * (f32(1.0) / np.sqrt(var + f32(eps))) * g.astype(f32)[None, :] + b.astype(f32)[None, :]


def emu_embed(tw, inp, swap_rb=True):
    cfg, W = tw.cfg, tw.W
    if tw.is_text:
        ids = np.asarray(inp)                               # one fp32 add of fp32 values
        full = np.full((ids.shape[0], tw.T), cfg.eos_token_id, dtype=np.int64)
        full[:, :ids.shape[1]] = ids
        x = (W["text_model.embeddings.token_embedding.weight"][full] +
             W["text_model.embeddings.position_embedding.weight"][None, :tw.T]).astype(f32).reshape(-1, tw.H)
    else:
        n, T, H = inp.shape[0], tw.T, tw.H
        w16, bias = patch_operands(W, cfg, tw.dt)
        pos = W["vision_model.embeddings.position_embedding.weight"]
        e = np.empty((n, T, H), f32)
        e[:, 1:] = ((patches_of(inp, cfg, swap_rb).astype(f32) @ w16.astype(f32).T) + bias.astype(f32)[None, :]).reshape(n, T - 1, H) + pos[None, 1:]
        e[:, 0] = W["vision_model.embeddings.class_embedding"] + pos[0]
        x = emu_layernorm(e.reshape(n * T, H), W["vision_model.pre_layrnorm.weight"], W["vision_model.pre_layrnorm.bias"], cfg.ln_eps)
    return {"x": x, "h": round16(x, tw.dt)}


def emu_ln_gemm(x, xh, w16, c2, eps, gelu, dt_out):
    """rstd (acc - mean c1) + c2 with mean = s1 / H and var = s2 / H - mean^2 from fp32 sums, as EpiLnH16 states it."""
    x, H = x.astype(f32), x.shape[1]
    inv_h = f32(1.0 / H)
    mean = x.sum(1, dtype=f32, keepdims=True) * inv_h
    var = np.maximum((x * x).sum(1, dtype=f32, keepdims=True) * inv_h - mean * mean, f32(0))
    rstd = f32(1.0) / np.sqrt(var + f32(eps))
    c1 = w16.astype(f64).sum(1).astype(f32)[None, :]
    y = rstd * (xh.astype(f32) @ w16.astype(f32).T - mean * c1) + np.asarray(c2).astype(f32)[None, :]
    if gelu:
        with np.errstate(over="ignore"):
            y = y * (f32(1.0) / (f32(1.0) + np.exp2(-y)))
    return round16(y, dt_out)


ATT_MUTANTS = ("drop_last_key", "padded_key", "scale_099", "no_max", "neighbour_v", "last_query_from_previous")
CAUSAL_MUTANTS = ("causal_plus_one", "causal_minus_one")


def emu_attention(qkv, n, T, heads, dt, causal, mutant=None):
    """The streaming form: keys in steps of 64, running maximum in the log2 domain, p = exp2(s log2e - m) rounded to 16 bits,
    the denominator accumulated from the ROUNDED probabilities; T <= 64 is the single-tile form."""
    q, k, v = (np.ascontiguousarray(a, f32) for a in split_heads(qkv, n, T, heads))
    if mutant == "neighbour_v":
        v = np.roll(v, 1, axis=1)
    if mutant == "last_query_from_previous":
        q = q.copy(); q[:, :, T - 1] = q[:, :, T - 2]
    keys = T - 1 if mutant == "drop_last_key" else T
    Tp = -(-T // KEY_TILE) * KEY_TILE
    if mutant == "padded_key":
        keys, Tp = T + 1, -(-(T + 1) // KEY_TILE) * KEY_TILE
    pad = ((0, 0), (0, 0), (0, Tp - T), (0, 0))
    k, v = np.pad(k, pad), np.pad(v, pad)                  # rows past the sequence read as zeros
    L2E = f32(LOG2E)
    qi, kj = np.arange(T)[:, None], np.arange(Tp)[None, :]
    live = np.broadcast_to(kj < keys, (T, Tp))
    if causal:
        live = live & (kj <= qi + {"causal_plus_one": 1, "causal_minus_one": -1}.get(mutant, 0))
    m_run = np.full((n, heads, T, 1), -3.0e38, f32)
    osum = np.zeros((n, heads, T, 1), f32)
    o = np.zeros((n, heads, T, 64), f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k0 in range(0, Tp, KEY_TILE):
            lv = live[:, k0:k0 + KEY_TILE]
            if not lv.any():
                continue
            s = q @ k[:, :, k0:k0 + KEY_TILE].transpose(0, 1, 3, 2)
            if mutant == "scale_099":
                s = s * f32(0.99)
            s = np.where(lv, s, f32(-3.0e38))
            m_new = np.maximum(m_run, s.max(-1, keepdims=True) * L2E)
            if mutant == "no_max":
                m_new = np.zeros_like(m_new)
            alpha = np.exp2(m_run - m_new)
            p = round16(np.where(lv, np.exp2(s * L2E - m_new), f32(0)), dt)
            osum = osum * alpha + p.sum(-1, dtype=f32, keepdims=True)
            o = o * alpha + p @ v[:, :, k0:k0 + KEY_TILE]
            m_run = m_new
        out = o * (f32(1.0) / osum)
    return round16(out.transpose(0, 2, 1, 3).reshape(n * T, heads * 64), dt)


def emu_residual(x, a, w16, b, dt):
    y = (x.astype(f32) + a.astype(f32) @ w16.astype(f32).T) + np.asarray(b).astype(f32)[None, :]
    return y, round16(y, dt)


def emu_block(tw, l, n, A, ops=None, eps=None, att_mutant=None):
    """One block on the emulated buffers A = {"x", "h"} -> {"qkv", "att", "mlp", "x", "h"}."""
    o = ops or tw.ops(l)
    eps = tw.eps if eps is None else eps
    qkv = emu_ln_gemm(A["x"], A["h"], o["w_qkv"], o["c2_qkv"], eps, False, tw.dt)
    att = emu_attention(qkv, n, tw.T, tw.heads, tw.dt, tw.is_text, att_mutant)
    x_mid, h_mid = emu_residual(A["x"], att, o["w_out"], o["b_out"], tw.dt)
    mlp = emu_ln_gemm(x_mid, h_mid, o["w_fc1"], o["c2_fc1"], eps, True, tw.dt)
    x, h = emu_residual(x_mid, mlp, o["w_fc2"], o["b_fc2"], tw.dt)
    return {"qkv": qkv, "att": att, "mlp": mlp, "x": x, "h": h}


def emu_chain(tw, n, inp, swap_rb=True):
    runs = [emu_embed(tw, inp, swap_rb)]
    for l in range(tw.layers):
        runs.append(emu_block(tw, l, n, runs[-1]))
    return runs


SPLIT_MUTANTS = ("low_half_dropped", "low_half_scale_256", "low_half_bytes_reversed_in_4", "low_half_stale", "no_clamp")
STATS_MUTANT = "stats_miss_one_8col_segment"


def emu_residual_split(A, a, w16, b, out_f32, mutant=None, site=1):
    """One residual epilogue on the stream state A = {"x", "h", "xl", "split", "y"} ("y": the fp32 value the row statistics were
    taken from): r = the fp32 x, or xh + e4m3(xl) / 512 where the stream is split; y = (r + acc) + bias in fp32; xh = fp16(y); then
    the fp32 y is written (out_f32), or xl = e4m3(med3((y - xh) 512, -448, 448)).  Mutants of the low half:
      low_half_dropped              the writer stores zero bytes
      low_half_scale_256            the writer scales by 256, the reader by 1 / 512
      low_half_bytes_reversed_in_4  the writer packs each group of four bytes in the opposite order
      low_half_stale                out_proj (site 0) does not write xl: fc2 reads what was there before
      no_clamp                      no med3: beyond +-448 the conversion gives the NaN code"""
    with np.errstate(invalid="ignore"):
        r = (A["h"].astype(f32) + (fp8_decode(A["xl"]) / XL_SCALE).astype(f32)) if A["split"] else A["x"].astype(f32)
        y = (r + a.astype(f32) @ w16.astype(f32).T) + np.asarray(b).astype(f32)[None, :]
    h, xl = split16_8(y, scale=256.0 if mutant == "low_half_scale_256" else XL_SCALE, clamp=mutant != "no_clamp")
    if out_f32:
        return {"x": y, "h": h, "xl": A["xl"], "split": False, "y": y}
    if mutant == "low_half_dropped":
        xl = np.zeros_like(xl)
    elif mutant == "low_half_bytes_reversed_in_4":
        xl = np.ascontiguousarray(xl.reshape(xl.shape[0], -1, 4)[:, :, ::-1]).reshape(xl.shape)
    elif mutant == "low_half_stale" and site == 0:
        xl = A["xl"]
    return {"x": A["x"], "h": h, "xl": xl, "split": True, "y": y}


def emu_block_split(tw, l, n, A, out_f32, mutant=None):
    """One full-row block of the default (split) pass.  out_proj always leaves the pair; fc2 leaves the fp32 x if out_f32.
    stats_miss_one_8col_segment: the row partials of both producers lack columns 8 .. 15 (one lane's piece of the 8-column form)."""
    o = tw.ops(l)

    def stats_of(st):
        if mutant != STATS_MUTANT or st.get("embed"):
            return st["y"]
        y = st["y"].copy()
        y[:, 8:16] = 0
        return y
    with np.errstate(invalid="ignore", over="ignore"):
        qkv = emu_ln_gemm(stats_of(A), A["h"], o["w_qkv"], o["c2_qkv"], tw.eps, False, tw.dt)
        att = emu_attention(qkv, n, tw.T, tw.heads, tw.dt, tw.is_text)
        mid = emu_residual_split(A, att, o["w_out"], o["b_out"], False, mutant, site=0)
        mlp = emu_ln_gemm(stats_of(mid), mid["h"], o["w_fc1"], o["c2_fc1"], tw.eps, True, tw.dt)
        B = emu_residual_split(mid, mlp, o["w_fc2"], o["b_fc2"], out_f32, mutant, site=1)
    B.update(qkv=qkv, att=att, mlp=mlp, y_mid=mid["y"])
    return B


def emu_chain_split(tw, n, inp, mutant=None, prune_last=True, swap_rb=True):
    """The passes limited to 0 .. (last full-row block) of the default pass, on the emulated buffers."""
    forms = split_forms(tw, prune_last)
    full = tw.layers - 1 if prune_last and not tw.is_text else tw.layers
    e = emu_embed(tw, inp, swap_rb)
    runs = [{"x": e["x"], "h": e["h"], "xl": np.zeros(e["x"].shape, np.uint8), "split": False, "y": e["x"], "embed": True}]
    for l in range(full):
        runs.append(emu_block_split(tw, l, n, runs[-1], not forms[l + 1], mutant))
    return runs


def emu_product_image(tw, n, prev, wrong_image=False):
    """The CLS-only last block on the emulated buffers of the run limited to layers - 1 blocks, then the pooling head.
    wrong_image (mutant): the residual row of image i is taken from image i + 1."""
    T, l = tw.T, tw.layers - 1
    o = tw.ops(l)
    full = emu_block(tw, l, n, prev)                       # q | k | v and the attention cover every token
    x = prev["x"].reshape(n, T, -1).copy()
    res = np.roll(x[:, 0], -1, axis=0) if wrong_image else x[:, 0]
    att_cls = full["att"].reshape(n, T, -1)[:, 0]
    x_mid, h = emu_residual(res, att_cls, o["w_out"], o["b_out"], tw.dt)
    mlp = emu_ln_gemm(x_mid, h, o["w_fc1"], o["c2_fc1"], tw.eps, True, tw.dt)
    x[:, 0], _ = emu_residual(x_mid, mlp, o["w_fc2"], o["b_fc2"], tw.dt)
    return {"x": x.reshape(n * T, -1), "att": full["att"], "h": h, "mlp": mlp}, emu_pool(tw, x[:, 0])


def emu_pool(tw, xrows):
    g, b, wp = tw.post()
    f = emu_layernorm(xrows, g, b, tw.eps) @ wp.astype(f32).T
    return f / np.maximum(np.sqrt((f * f).sum(1, dtype=f32, keepdims=True)), f32(1e-12))


# ---------------------------------------------------------------------------------------------------- hard inputs
def make_weights(tower, cfg, kind, seed=1234):
    """kind: 'seeded' | 'stress' | 'lowvar' (stress_weights with low_variance) | 'passthrough'."""
    from video_quierer_amd.weights import seeded_text_weights, seeded_weights
    if kind == "seeded":
        return seeded_text_weights(cfg, seed) if tower == "text" else seeded_weights(cfg, seed)
    if kind == "passthrough":
        return passthrough_weights(cfg, seed, text=tower == "text")
    return stress_weights(cfg, seed, low_variance=kind == "lowvar", text=tower == "text")


def make_input(tower, cfg, n, seed=1234):
    """Image tower: n random uint8 frames.  Text tower: ids [n, max_positions], bos first, eos (then eos padding) at a
    different position per row; the first row uses every position."""
    rng = np.random.default_rng([seed, 5])
    if tower == "image":
        return rng.integers(0, 256, (n, cfg.image_size, cfg.image_size, 3), dtype=np.uint8)
    T = cfg.max_positions
    ids = rng.integers(0, cfg.bos_token_id, (n, T))
    ids[:, 0] = cfg.bos_token_id
    for i, eos in enumerate(np.linspace(T - 1, 3, n).astype(int)):
        ids[i, eos:] = cfg.eos_token_id
    return ids


HOT_HEAD, WARM_HEAD, ZERO_Q_HEAD, KBIAS_HEAD = 0, 1, 2, 3
HOT_SCALE, WARM_SCALE = 7.0, 2.2         # on q AND k: logits x 49 and x 4.8
FC1_HOT_ROWS, FC1_HOT_SCALE = 64, 24.0
OUT_BIAS_OFFSET = 2.0
EDGE_POS_SCALE, EDGE_KEY_GAIN = 40.0, 60.0


def stress_weights(cfg, seed, low_variance=False, text=False):
    """Seeded weights pushed to where kernels go wrong (every block alike):
      * head 0: q, k weights and biases x 7 (logit spread in the hundreds: softmax overflows without the max subtraction and the
        running max keeps moving along the key walk); head 1: x 2.2 (spread about 30);
      * head 2: q = 0 exactly -> uniform softmax, the output is the mean of V over exactly T keys (or the causal prefix);
      * head 3: k bias + 6 in every dimension: a per-query common offset of the logits, to which softmax is invariant;
      * position embeddings of token 0 and token T - 1 x 40, and block 0's hot head keyed to them (below): the edge keys
        carry the weight of many rows, so a dropped key T - 1 or a wrong first tile cannot hide;
      * out_proj bias + 2 in every channel: |row mean| / row std of the LayerNorm-2 input between 1 and 3;
      * the first 64 fc1 rows x 24: pre-activations beyond +-60, where 2^-y saturates either way;
      * low_variance: pre-LayerNorm gain and bias x 0.05 (text tower: both embeddings x 0.1), row variance about 2.5e-3,
        where eps = 1e-5 is no longer invisible; out_proj x 0.05 instead of its offset, so that LayerNorm 2 of block 0 sees
        such rows too."""
    from video_quierer_amd.weights import seeded_text_weights, seeded_weights
    W = {k: v.copy() for k, v in (seeded_text_weights(cfg, seed) if text else seeded_weights(cfg, seed)).items()}
    prefix = "text_model" if text else "vision_model"
    sl = lambda h: slice(64 * h, 64 * h + 64)
    for l in range(cfg.layers):
        p = f"{prefix}.encoder.layers.{l}.self_attn."
        for nm in ("q_proj", "k_proj"):
            for head, s in ((HOT_HEAD, HOT_SCALE), (WARM_HEAD, WARM_SCALE)):
                W[p + nm + ".weight"][sl(head)] *= s
                W[p + nm + ".bias"][sl(head)] *= s
        W[p + "q_proj.weight"][sl(ZERO_Q_HEAD)] = 0.0
        W[p + "q_proj.bias"][sl(ZERO_Q_HEAD)] = 0.0
        W[p + "k_proj.bias"][sl(KBIAS_HEAD)] += 6.0
        if low_variance:                                   # the attention branch must not lift the variance of LayerNorm 2's input
            W[p + "out_proj.weight"] *= 0.05
            W[p + "out_proj.bias"] *= 0.05
        else:
            W[p + "out_proj.bias"] += OUT_BIAS_OFFSET
        W[f"{prefix}.encoder.layers.{l}.mlp.fc1.weight"][:FC1_HOT_ROWS] *= FC1_HOT_SCALE
    pos = W[f"{prefix}.embeddings.position_embedding.weight"]
    pos[0] *= EDGE_POS_SCALE
    pos[-1] *= EDGE_POS_SCALE
    # With such position embeddings the rows of tokens 0 and T - 1 are (nearly) the same in every image, so block 0's
    # LayerNorm-1 output z_t of either is known from the weights alone.  The hot head's k weights get a rank-one term
    # that adds EDGE_KEY_GAIN * u_t to the key of token t only (w = z_t / |z_t|^2 picks it out; other tokens see ~ H^-1/2 of
    # it), u_t = the unit direction of token t's own query: every query on u_t's side has its argmax on that edge key.
    std_row = lambda v: (v - v.mean()) / np.sqrt(v.var() + cfg.ln_eps)
    p0 = f"{prefix}.encoder.layers.0."
    if text:
        tok = W["text_model.embeddings.token_embedding.weight"]
        edge_x = [tok[cfg.bos_token_id].astype(f64) + pos[0], tok[cfg.eos_token_id].astype(f64) + pos[-1]]
    else:
        g, b = W["vision_model.pre_layrnorm.weight"].astype(f64), W["vision_model.pre_layrnorm.bias"].astype(f64)
        edge_x = [std_row(W["vision_model.embeddings.class_embedding"].astype(f64) + pos[0]) * g + b, std_row(pos[-1].astype(f64)) * g + b]
    for xt in edge_x:
        z = std_row(xt) * W[p0 + "layer_norm1.weight"] + W[p0 + "layer_norm1.bias"]
        qt = W[p0 + "self_attn.q_proj.weight"][sl(HOT_HEAD)].astype(f64) @ z + W[p0 + "self_attn.q_proj.bias"][sl(HOT_HEAD)]
        W[p0 + "self_attn.k_proj.weight"][sl(HOT_HEAD)] += (EDGE_KEY_GAIN * np.outer(qt / np.linalg.norm(qt), z / (z @ z))).astype(f32)
    if low_variance:
        if text:
            pos *= 0.1
            W["text_model.embeddings.token_embedding.weight"] *= 0.1
        else:
            W["vision_model.pre_layrnorm.weight"] *= 0.05
            W["vision_model.pre_layrnorm.bias"] *= 0.05
    return W


def stress_properties(tw, n, runs):
    """What the stress fixture promises, measured on the fp64 references of block 0 (from the buffers in `runs`)."""
    T = tw.T
    _, _, info = attention_ref_bound(runs[1]["qkv"], n, T, tw.heads, tw.dt, tw.is_text)
    s, p = info["s"], info["p"]
    fin = np.where(np.isfinite(s), s, np.nan)
    spread = np.nanmax(fin, -1) - np.nanmin(fin, -1)                        # [n][heads][T]
    arg = s.argmax(-1)
    pmax = (p / p.sum(-1, keepdims=True)).max(-1)
    hot = arg[:, [HOT_HEAD, WARM_HEAD]][pmax[:, [HOT_HEAD, WARM_HEAD]] > 0.5]   # the rows whose argmax key carries most of the weight
    o = tw.ops(0)
    x_mid, _ = residual_ref_bound(runs[0]["x"], runs[1]["att"], o["w_out"], o["b_out"])
    ratio = np.abs(x_mid.mean(1)) / x_mid.std(1)
    cz, _ = ln_gemm_ref_bound(x_mid, x_mid, o["w_fc1"], o["c2_fc1"], tw.eps, False, tw.dt)    # c * (fc1 pre-activation)
    pre = cz / (GELU_A * LOG2E)
    return {
        "spread_hot": float(spread[:, HOT_HEAD].max()), "spread_warm": float(np.median(spread[:, WARM_HEAD].max(-1))),
        "spread_zero_q": float(spread[:, ZERO_Q_HEAD].max()),
        "argmax_first_tile": int(np.count_nonzero(hot < KEY_TILE)), "argmax_last_tile": int(np.count_nonzero(hot >= (T - 1) // KEY_TILE * KEY_TILE)),
        "argmax_last_key": int(np.count_nonzero(hot == T - 1)),
        "mean_over_std_median": float(np.median(ratio)), "row_var_median": float(np.median(np.asarray(runs[0]["x"], f64).var(1))),
        "preact_min": float(pre.min()), "preact_max": float(pre.max()),
    }


# planted channels of the passthrough fixture: spread over the 8-column pieces and the 4-byte groups of a row
CLAMP_CHANNELS = tuple(3 + 5 * j for j in range(16))                 # 3 .. 78
CLAMP_VALUES = (3000.0, -3000.0, 12000.0, -12000.0)                  # |x| in [2048, 4096) and in [8192, 16384), both signs
TINY_CHANNELS = tuple(101 + 7 * j for j in range(24))                # 101 .. 262
TINY_SCALES = tuple(2.0 ** -(8 + j % 8) for j in range(24))          # |x| from about 2^-8 down to fp16's subnormals


def passthrough_weights(cfg, seed, text=False):
    """Seeded weights whose residual GEMMs add exactly nothing: out_proj.weight = fc2.weight = 0 in every block, so x_mid = x +
    b_out and x_out = x_mid + b_fc2 with zero accumulators, and the `resid` bound is the pair's own error plus four fp32 adds.
    The biases stay small (0.02 sigma), except:
      * block 0's out_proj bias puts CLAMP_CHANNELS at +-3000 and +-12000: half an fp16 ulp is 1 and 4 there, beyond the 448 / 512
        the low byte can hold - the clamp (and, without it, the NaN code);
      * TINY_CHANNELS are scaled by 2^-8 ... 2^-15 where they enter the stream (image tower: pre-LayerNorm gain and bias; text
        tower: the token- and position-embedding columns) and in every residual bias: |x| < 2^-6, where the low byte is an fp8
        subnormal or flushes to zero.
    q|k|v, the attention and the MLP still run on this stream and are held to their own bounds."""
    from video_quierer_amd.weights import seeded_text_weights, seeded_weights
    W = {k: v.copy() for k, v in (seeded_text_weights(cfg, seed) if text else seeded_weights(cfg, seed)).items()}
    prefix = "text_model" if text else "vision_model"
    ch, sc = np.array(TINY_CHANNELS), np.array(TINY_SCALES, f32)
    for l in range(cfg.layers):
        p = f"{prefix}.encoder.layers.{l}."
        W[p + "self_attn.out_proj.weight"][:] = 0.0
        W[p + "mlp.fc2.weight"][:] = 0.0
        for nm in ("self_attn.out_proj.bias", "mlp.fc2.bias"):
            W[p + nm][ch] *= sc
    b0 = W[f"{prefix}.encoder.layers.0.self_attn.out_proj.bias"]
    for j, c in enumerate(CLAMP_CHANNELS):
        b0[c] = CLAMP_VALUES[j % 4]
    if text:
        W["text_model.embeddings.token_embedding.weight"][:, ch] *= sc[None, :]
        W["text_model.embeddings.position_embedding.weight"][:, ch] *= sc[None, :]
    else:
        W["vision_model.pre_layrnorm.weight"][ch] *= sc
        W["vision_model.pre_layrnorm.bias"][ch] *= sc
    return W


def passthrough_properties(runs):
    """How many of the values a split pass STORED as a pair (every x_mid, and each block output left split; taken from the
    emulation, which has the fp32 y) lie where the low byte clamps, is an fp8 subnormal, belongs to an |x| < 2^-6, or is ordinary."""
    ys = [r["y_mid"] for r in runs[1:]] + [r["y"] for r in runs[1:] if r["split"]]
    y = np.concatenate([np.asarray(v, f64).ravel() for v in ys])
    t = np.abs(y - round16(y.astype(f32), "fp16").astype(f64)) * XL_SCALE
    return {"clamped": int(np.count_nonzero(t > FP8_MAX)), "fp8_subnormal": int(np.count_nonzero((t >= 2.0 ** -10) & (t < 2.0 ** -6))),
            "below_2^-6": int(np.count_nonzero(np.abs(y) < 2.0 ** -6)),
            "ordinary": int(np.count_nonzero((t >= 2.0 ** -6) & (t <= FP8_MAX) & (np.abs(y) >= 2.0 ** -6)))}
