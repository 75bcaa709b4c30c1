// The encoder's host decisions, each written once and none of them a HIP call:
//   place_weights / place_workspace   the only places that name a buffer's size.  Each runs twice per handle: on an Arena with a null
//                                     base to measure (a buffer's "pointer" is then its offset), and on the allocated one to carve.
//   plan_forward(...)                 (geometry, options, n) -> the scalars run_forward launches by: GEMM row counts and kernel ids, the
//                                     patchify and attention forms, the CLS-only last block and its split-K, the form of the residual
//                                     stream.  resid_mode(plan, layer, fc2) is the mode of one residual epilogue.
// vq_debug_encoder_plan returns all of it on a machine without a GPU (tests/test_encoder_plan_cpu.py).
#pragma once
#include "gemm_dispatch.h"
#include "encoder_kernels.h"
#include <algorithm>
#include <vector>

namespace vq {

// Operand type per GEMM group (bit set = fp16, clear = bf16; fp32 accumulation either way, same MFMA rate).
// A group = every 16-bit tensor that meets in one MFMA: the weights and the activations that multiply them.
//   DT_PATCH  patch pixels (exact in both types) x W_patch
//   DT_QKV    LN1 output h x W_qkv
//   DT_ATTN   q | k | v, softmax probabilities, attention output x W_out
//   DT_FC1    LN2 output h x W_fc1
//   DT_FC2    quick-GELU output x W_fc2
enum : int { DT_PATCH = 1, DT_QKV = 2, DT_ATTN = 4, DT_FC1 = 8, DT_FC2 = 16, DT_ALL = 31 };

struct EncGeometry {      // what a handle fixes at creation
    vq_vit_config cfg{};  // the text tower: image_size = patch_size = 0
    int tokens = 0, patches = 0, patch_k = 0, max_batch = 0;
    int64_t rows_pad = 0, prow_pad = 0;
    bool is_text = false;       // CLIP text tower (vq_text_encoder_*): token embedding, causal attention, EOS pooling
    int vocab = 0, eos_id = 0;
    size_t frame_bytes() const { return (size_t)cfg.image_size * cfg.image_size * 3; }
};

// $VQ_AMD_ATTN: simple = per-wave streaming attention (reference implementation of the wg one); q64 = 64 query rows per wave (the
// round-2 form) instead of 32; t64 = the run-time-T single-tile kernel where attention_tile_kernel<T> would run (A/B switches)
enum AttnSwitch : int { ATTN_DEFAULT = 0, ATTN_SIMPLE, ATTN_Q64, ATTN_T64 };

struct EncOptions {       // what the create flags, the environment (create_options) and the two debug setters decide
    int f16_mask = 0;           // per-GEMM-group operand type, DT_* bits: create flags / $VQ_AMD_DTYPE
    int gemm_force = GK_AUTO;   // $VQ_AMD_GEMM: a GemmKernel id (gemm_dispatch.h); concurrent handles: GK_AUTO_NO160
    int gemm24_mask = 0;        // $VQ_AMD_GEMM24: which full-batch GEMMs run the hand-scheduled four-wave kernel (gemm_asm256.h): 1 qkv, 2 out_proj, 4 fc1, 8 fc2,
                                // 16 patch embedding.  Default none: 16 % fewer cycles per K-tile, and the chip answers with a 14 % lower clock - frames/s equal
                                // within 1 % with three batches in flight, +1.3 % for fc2 on a lone handle, -1 % on ViT-L/14 (DESIGN.md §4 "Round 3" (5))
    bool split_resid = true;    // $VQ_AMD_RESID=f32: every residual epilogue reads and writes the fp32 x (rounds 1-3; the A/B switch)
    bool prune_last = true;     // last block on CLS rows only (outputs unchanged); $VQ_AMD_FULL_LAST_LAYER=1 turns it off
    AttnSwitch attn = ATTN_DEFAULT;
    int run_layers = -1;        // vq_encoder_debug_set_layers
    bool keep_stream = false;   // debug: a layer-limited pass keeps the residual stream in the form the full pass holds it in (vq_encoder_debug_keep_stream)
};

// ---- layout ---------------------------------------------------------------------------------------------------------
struct Arena {            // one hipMalloc, 256-B aligned bump allocation
    uintptr_t base = 0; size_t size = 0, used = 0;
    template <class T> T* take(size_t count) {
        used = (used + 255) & ~(size_t)255;
        T* p = (T*)(base + used);
        used += count * sizeof(T);
        return p;
    }
};

// LayerNorm 1 / 2 are folded into the qkv / fc1 GEMMs (encoder_kernels.h "LayerNorm folded into the GEMMs"):
// w_qkv = g1 (.) W_qkv, c1_qkv[n] = sum_k w_qkv[n][k] (of the rounded 16-bit values), c2_qkv[n] = sum_k b1[k] W_qkv[n][k] + bias
struct LayerW {
    float *c1_qkv, *c2_qkv, *b_out, *c1_fc1, *c2_fc1, *b_fc2;
    uint16_t *w_qkv, *w_out, *w_fc1, *w_fc2;
};
struct EncWeights {
    uint16_t* w_patch = nullptr; float *b_patch = nullptr, *cls = nullptr, *pos = nullptr, *tok_emb = nullptr;
    float *pre_g = nullptr, *pre_b = nullptr, *post_g = nullptr, *post_b = nullptr, *w_proj = nullptr;
    std::vector<LayerW> layers;
};
struct EncWorkspace {
    uint8_t* d_frames = nullptr; int *d_ids = nullptr, *d_rowidx = nullptr;
    float2* ps = nullptr;                      // LayerNorm row partials [LN_MAX_GRANULES][rows_pad]
    float *x = nullptr, *d_out = nullptr;
    uint16_t *h = nullptr, *qkv = nullptr, *att = nullptr, *mlp = nullptr;      // h = xh: the residual stream rounded to 16 bits
    uint16_t* xl = nullptr;                    // [r04] the low half of the split residual stream, one fp8 byte per element (EpiBiasResidualLnF32 modes)
};

static inline void place_weights(Arena& A, const EncGeometry& g, EncWeights& w) {
    const size_t H = g.cfg.hidden, M = g.cfg.mlp;
    if (g.is_text) w.tok_emb = A.take<float>((size_t)g.vocab * H);
    else { w.cls = A.take<float>(H); w.w_patch = A.take<uint16_t>(H * g.patch_k); w.b_patch = A.take<float>(H); }
    w.pos = A.take<float>((size_t)g.tokens * H);
    if (!g.is_text) { w.pre_g = A.take<float>(H); w.pre_b = A.take<float>(H); }
    w.layers.resize(g.cfg.layers);
    for (LayerW& L : w.layers) {
        L.w_qkv = A.take<uint16_t>(3 * H * H); L.c1_qkv = A.take<float>(3 * H); L.c2_qkv = A.take<float>(3 * H);
        L.w_out = A.take<uint16_t>(H * H);     L.b_out = A.take<float>(H);
        L.w_fc1 = A.take<uint16_t>(M * H);     L.c1_fc1 = A.take<float>(M);     L.c2_fc1 = A.take<float>(M);
        L.w_fc2 = A.take<uint16_t>(H * M);     L.b_fc2 = A.take<float>(H);
    }
    w.post_g = A.take<float>(H); w.post_b = A.take<float>(H);
    w.w_proj = A.take<float>((size_t)g.cfg.proj_dim * H);     // stored transposed [hidden][proj_dim]
}

static inline size_t xl_elems(const EncGeometry& g) {         // uint16 elements that hold xl: one byte per element of x (fp8 low half)
    const size_t n = (size_t)g.rows_pad * g.cfg.hidden;
    return VQ_RESID_XL8 ? (n + 1) / 2 : n;
}

static inline void place_workspace(Arena& A, const EncGeometry& g, EncWorkspace& w) {
    const size_t H = g.cfg.hidden, R = g.rows_pad;
    if (g.is_text) { w.d_ids = A.take<int>((size_t)g.max_batch * g.tokens); w.d_rowidx = A.take<int>(g.max_batch); }
    else w.d_frames = A.take<uint8_t>(g.max_batch * g.frame_bytes());
    w.ps = A.take<float2>((size_t)LN_MAX_GRANULES * R);
    w.x = A.take<float>(R * H);
    w.d_out = A.take<float>((size_t)g.max_batch * g.cfg.proj_dim);
    w.h = A.take<uint16_t>(R * H);
    w.xl = A.take<uint16_t>(xl_elems(g));
    w.qkv = A.take<uint16_t>(R * 3 * H);
    w.att = A.take<uint16_t>(R * H);
    w.mlp = A.take<uint16_t>(std::max(R * (size_t)g.cfg.mlp, (size_t)g.prow_pad * g.patch_k));     // also the patch rows of the patch-embedding GEMM
}

// What is allocated behind `mlp`, the last buffer: 4096 bytes, and the bytes by which the sum that sized the arena before
// the layout was measured counted xl (two bytes per element where one is carved).  No kernel is known to need them; the
// allocation keeps its size until somebody shows that none reads past mlp.
static inline size_t arena_tail_bytes(const EncGeometry& g) {
    return 4096 + ((size_t)g.rows_pad * g.cfg.hidden - xl_elems(g)) * 2;
}

// Bytes of a handle's arena: weights (unless they are another handle's) + workspace + tail.
static inline size_t arena_bytes(const EncGeometry& g, bool with_weights, EncWorkspace* offsets = nullptr) {
    Arena A;
    EncWeights w;
    EncWorkspace ws;
    if (with_weights) place_weights(A, g, w);
    place_workspace(A, g, offsets ? *offsets : ws);
    return A.used + arena_tail_bytes(g);
}

// ---- forward plan ---------------------------------------------------------------------------------------------------
enum PatchifyKernel : int { PATCHIFY_NONE = 0, PATCHIFY_U8, PATCHIFY_GENERIC };      // none: the text tower embeds tokens
enum AttnKernel : int {
    AK_TEXT_WG = 0,      // attention_stream_wg_kernel<F16, true>: causal
    AK_TILE50,           // attention_tile_kernel<F16, 50>: ViT-B/32 at 224^2, the compile-time-T form
    AK_T64,              // attention_t64_kernel: T <= 64 at run time
    AK_STREAM,           // attention_stream_kernel ($VQ_AMD_ATTN=simple)
    AK_WG32,             // attention_stream_wg_kernel<F16, false, 2>: 32 query rows per wave, three waves per SIMD
    AK_WG64,             // attention_stream_wg_kernel<F16, false> ($VQ_AMD_ATTN=q64)
};

struct EncPlan {
    int rows, rows_gemm, rows_out, rows_fc2;      // live rows n * T; GEMM rows of qkv and fc1, of out_proj, of fc2 (160-row tiles or not)
    int prows, prows_gemm, rows_cls;              // patch rows live / GEMM; GEMM rows of the CLS-only block
    int k_patch, k_qkv, k_out, k_fc1, k_fc2;      // the id launch_gemm_auto gets for each full-row GEMM (the CLS-only ones get gemm_force)
    int patchify, attention;                      // a PatchifyKernel, an AttnKernel
    int layers_run;
    bool cls_only_last;                           // the last block run is the CLS-only one
    int fc2_splits;                               // split-K slices of that block's fc2; 0: one launch_gemm_auto
    bool split;                                   // the residual stream is held as xh + xl between the residual epilogues
    int first_f32_layer;                          // ... and the fc2 of this block writes the fp32 x again (its reader comes next)
    bool stream_left_split;                       // the form the pass leaves the stream in
};

// GEMM row counts are padded (the buffers are): to 256 when that adds < 6 % work, so the phased
// 256x256 kernel applies; small batches keep 128-row granularity
static inline int enc_pad_rows(int r) {
    const int r256 = (int)round_up(r, G2_BM), r128 = (int)round_up(r, GEMM_BM);
    return (r256 - r128) * 16 <= r128 ? r256 : r128;
}

static inline EncPlan plan_forward(const EncGeometry& g, const EncOptions& o, int n) {
    const vq_vit_config& c = g.cfg;
    const int H = c.hidden, T = g.tokens;
    EncPlan p{};
    p.rows = n * T;
    p.rows_gemm = enc_pad_rows(p.rows);
    p.prows = n * g.patches;
    p.prows_gemm = enc_pad_rows(p.prows);
    p.rows_cls = enc_pad_rows(n);
    // the hand-scheduled four-wave kernel (gemm_asm256.h) for the GEMMs $VQ_AMD_GEMM24 names, where 256-row tiles fill half the chip
    auto use24 = [&](int bit, int M, int N, int K) {
        return (o.gemm24_mask & bit) && (o.gemm_force == GK_AUTO || o.gemm_force == GK_AUTO_NO160) && M % G2_BM == 0 && N % G2_BN == 0 && K % (2 * G2_BK) == 0 &&
               (int64_t)(M / G2_BM) * (N / G2_BN) >= 128;
    };
    auto kernel = [&](int bit, int M, int N, int K) { return use24(bit, M, N, K) ? (int)GK_ASM256 : o.gemm_force; };
    // per-GEMM row count: 160-row tiles where they occupy more CUs than 256-row tiles (gemm_mfma160.h)
    auto rows160 = [&](int bit, int N, int K) {
        if (use24(bit, p.rows_gemm, N, K)) return p.rows_gemm;
        const int r160 = (int)round_up(p.rows, G5_BM);
        return (o.gemm_force == GK_AUTO && gemm_use160() && r160 <= g.rows_pad && prefer_tn160(r160, N, K)) ? r160 : p.rows_gemm;
    };
    p.rows_out = rows160(2, H, H);
    p.rows_fc2 = rows160(8, H, c.mlp);
    p.k_patch = kernel(16, p.prows_gemm, H, g.patch_k);
    p.k_qkv = kernel(1, p.rows_gemm, 3 * H, H);
    p.k_out = kernel(2, p.rows_gemm, H, H);
    p.k_fc1 = kernel(4, p.rows_gemm, c.mlp, H);
    p.k_fc2 = kernel(8, p.rows_gemm, H, c.mlp);
    p.patchify = g.is_text ? PATCHIFY_NONE : (c.patch_size % 8 == 0 && g.patch_k == 3 * c.patch_size * c.patch_size) ? PATCHIFY_U8 : PATCHIFY_GENERIC;
    p.attention = g.is_text ? AK_TEXT_WG : (T == 50 && c.heads % 4 == 0 && o.attn != ATTN_T64) ? AK_TILE50 : (T <= 64 && c.heads % 4 == 0) ? AK_T64 :
                  o.attn == ATTN_SIMPLE ? AK_STREAM : o.attn != ATTN_Q64 ? AK_WG32 : AK_WG64;
    // [r04] the residual stream at 16 + 8 bits between the residual epilogues (encoder_kernels.h): fp16 operands in every group
    // that writes xh, and not in layer-limited debug runs (vq_encoder_debug_read reads the fp32 x).  The first residual epilogue
    // reads the embedding kernel's fp32 x; the last one in front of a reader of x (pooling head / the CLS-only last block) writes it.
    // With keep_stream a layer-limited run is the full pass cut short: every block it runs has the full pass's form and modes
    // (decided by cfg.layers and prune_last, not by the limit), and x, xh, xl stay as that block left them.
    p.layers_run = o.run_layers < 0 ? c.layers : std::min(o.run_layers, c.layers);
    const bool as_full = o.run_layers < 0 || o.keep_stream;
    // Only the CLS token of the last block is consumed (E8): its out_proj / LN2 / MLP run on the n CLS rows instead of n*T rows
    // (292.8 MMAC of 4408.8 per frame).  K/V and the attention itself still cover every token.
    const bool cls_last = !g.is_text && o.prune_last && as_full;      // layer-limited runs keep every row (unless they keep the full pass's stream)
    p.cls_only_last = cls_last && p.layers_run == c.layers;
    // 2 x 6 output tiles over K = mlp: split-K so that ~100 workgroups share the long K loop; the partial planes live in the q|k|v buffer
    const bool planes_fit = c.mlp % (8 * GEMM_BK) == 0 && (size_t)8 * p.rows_cls * H * 2 <= (size_t)g.rows_pad * 3 * H;
    p.fc2_splits = (planes_fit && p.rows_cls % GEMM_BM == 0 && o.gemm_force != GK_PHASE4 && o.gemm_force != GK_DEEP) ? 8 : 0;
    p.split = o.split_resid && (o.f16_mask & DT_QKV) && (o.f16_mask & DT_FC1) && as_full;
    p.first_f32_layer = cls_last ? c.layers - 2 : (as_full ? c.layers : p.layers_run) - 1;
    const int full_blocks = p.layers_run - (p.cls_only_last ? 1 : 0);
    p.stream_left_split = p.split && full_blocks > 0 && full_blocks - 1 != p.first_f32_layer;
    return p;
}

// The mode of the residual epilogue of block `layer` (its out_proj, or its fc2): a function of the plan alone.
static inline int resid_mode(const EncPlan& p, int layer, bool fc2) {
    if (!p.split) return RS_F32;
    return (layer == 0 && !fc2 ? 0 : RS_IN_SPLIT) | (fc2 && layer == p.first_f32_layer ? RS_OUT_F32 : RS_OUT_SPLIT);
}

}  // namespace vq
