// vq_encoder: CLIP ViT image-encoder forward pass on one MI355X.
// Replaces FeatureExtractor._load_model / extract_batch
// (reference src/core/feature_extractor.py:70-103, 137-177) and the
// transformers CLIP vision tower it calls.
// Buffer layout and the forward pass's decisions: encoder_plan.h; here the uploads, the launches and the C entry points.
#include "../../include/vq_amd.h"
#include "vq_common.h"
#include "encoder_plan.h"

#include <cmath>
#include <cstring>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <type_traits>
#include <thread>

namespace vq {
int require_init();

enum EncClass { C_PATCHIFY = 0, C_GEMM_PATCH, C_EMBED_FINISH, C_LAYERNORM, C_GEMM_QKV, C_ATTENTION,
                C_GEMM_OUT, C_GEMM_FC1, C_GEMM_FC2, C_POOL, C_LAST_CLS };
static const char* kEncClassNames[VQ_ENC_NCLASS] = {
    "patchify_u8", "gemm_patch_embed", "embed_finish_ln", "layernorm_bf16", "gemm_qkv",
    "attention", "gemm_out_proj_residual", "gemm_fc1_quickgelu", "gemm_fc2_residual", "pool_project",
    "last_block_cls_rows"};      // the last block's out_proj / fc1 / fc2 on the n CLS rows: a class of its own, so that the per-launch
                                 // averages of the three GEMM classes above are those of full-size launches only
}  // namespace vq

using namespace vq;

struct vq_encoder : EncGeometry, EncWeights, EncWorkspace {
    EncOptions opt;
    hipStream_t stream = nullptr;       // stream in use
    hipStream_t own_stream = nullptr;   // created by the handle
    std::mutex mu;
    Arena arena;
    std::shared_ptr<void> arena_owner;     // frees arena.base when the last handle using it goes
    std::shared_ptr<void> weights_owner;   // vq_encoder_create_shared: the parent's arena, where this handle's weights live
    uint8_t* h_stage[2] = {nullptr, nullptr};   // pinned staging slots (lazy)
    float* h_out_stage = nullptr;               // pinned result buffer
    // pipelined ingest (vq_encoder_submit_staged / wait_staged): per-slot device frames + pinned results, a copy
    // stream for the uploads, events ordering upload -> forward -> download per slot
    uint8_t* d_slot_frames[2] = {nullptr, nullptr};
    float* h_slot_out[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_fwd[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    int slot_n[2] = {0, 0};                     // frames in flight per slot (0 = idle)
    bool stream_split = false;                 // what the last pass left: the pair xh + xl (true) or the fp32 x
    float patch_unscale = 1.0f;   // 2^-s: undoes the power-of-two scale on fp16 patch weights (EpiPatchEmbedF32)
    bool h_is_f16 = false;   // type of what `h` holds right now (debug_read)
    // profiling
    bool profiling = false;
    struct Ev { int cls; hipEvent_t a, b; };
    std::vector<Ev> events;
    std::vector<hipEvent_t> pool;
};

namespace {

struct Prof {             // brackets one launch with events when profiling
    vq_encoder* e; int cls; hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t get(vq_encoder* e) {
        if (!e->pool.empty()) { hipEvent_t ev = e->pool.back(); e->pool.pop_back(); return ev; }
        hipEvent_t ev; (void)hipEventCreate(&ev); return ev;
    }
    Prof(vq_encoder* enc, int c) : e(enc), cls(c) {
        if (e->profiling) { a = get(e); b = get(e); (void)hipEventRecord(a, e->stream); }
    }
    ~Prof() {
        if (e->profiling) { (void)hipEventRecord(b, e->stream); e->events.push_back({cls, a, b}); }
    }
};

int upload_f32(float* dst, const float* src, size_t n) {
    VQ_HIP(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice));
    return 0;
}
int upload_h16(uint16_t* dst, const float* src, size_t n, bool f16, float scale = 1.0f) {
    std::vector<uint16_t> tmp(n);
    if (f16) for (size_t i = 0; i < n; ++i) tmp[i] = __builtin_bit_cast(uint16_t, (_Float16)(src[i] * scale));
    else     for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16_rne(src[i] * scale);
    VQ_HIP(hipMemcpy(dst, tmp.data(), n * 2, hipMemcpyHostToDevice));
    return 0;
}

// W' = gamma (.) W (scaled), rounded to the operand type; c1[n] = sum_k W'16[n][k]; c2[n] = scale (sum_k beta[k] W[n][k] + bias[n])
int upload_folded(uint16_t* dst, float* c1_dst, float* c2_dst, const float* W, const float* gamma, const float* beta,
                  const float* bias, size_t N, size_t K, bool f16, float scale = 1.0f) {
    std::vector<uint16_t> w16(N * K);
    std::vector<float> c1(N), c2(N);
    for (size_t n = 0; n < N; ++n) {
        double s1 = 0.0, s2 = 0.0;
        for (size_t k = 0; k < K; ++k) {
            const float wf = W[n * K + k] * scale * gamma[k];
            const uint16_t r = f16 ? __builtin_bit_cast(uint16_t, (_Float16)wf) : f32_to_bf16_rne(wf);
            w16[n * K + k] = r;
            s1 += f16 ? (double)(float)__builtin_bit_cast(_Float16, r) : (double)bf16_to_f32(r);
            s2 += (double)beta[k] * (double)W[n * K + k];
        }
        c1[n] = (float)s1;
        c2[n] = (float)((s2 + (double)bias[n]) * (double)scale);
    }
    VQ_HIP(hipMemcpy(dst, w16.data(), w16.size() * 2, hipMemcpyHostToDevice));
    VQ_HIP(hipMemcpy(c1_dst, c1.data(), N * 4, hipMemcpyHostToDevice));
    VQ_HIP(hipMemcpy(c2_dst, c2.data(), N * 4, hipMemcpyHostToDevice));
    return 0;
}

// One transformer block's tensors (HF order: ln1.{w,b}, q.{w,b}, k.{w,b}, v.{w,b}, out.{w,b}, ln2.{w,b}, fc1.{w,b}, fc2.{w,b})
// -> device, with layer_norm1 folded into the fused q|k|v weights (q additionally pre-scaled by d_h^-0.5) and
// layer_norm2 into fc1.
int upload_layer(const LayerW& L, int f16_mask, const float* const* weights, int& wi, size_t H, size_t M, float qscale) {
    const float *g1 = weights[wi], *b1 = weights[wi + 1];
    wi += 2;
    for (int part = 0; part < 3; ++part) {        // q, k, v
        const float s = part == 0 ? qscale : 1.0f;
        VQ_TRY(upload_folded(L.w_qkv + part * H * H, L.c1_qkv + part * H, L.c2_qkv + part * H, weights[wi], g1, b1, weights[wi + 1],
                             H, H, f16_mask & DT_QKV, s));
        wi += 2;
    }
    VQ_TRY(upload_h16(L.w_out, weights[wi++], H * H, f16_mask & DT_ATTN));
    VQ_TRY(upload_f32(L.b_out, weights[wi++], H));
    const float *g2 = weights[wi], *b2 = weights[wi + 1];
    wi += 2;
    VQ_TRY(upload_folded(L.w_fc1, L.c1_fc1, L.c2_fc1, weights[wi], g2, b2, weights[wi + 1], M, H, f16_mask & DT_FC1, VQ_GELU_FOLD ? QUICK_GELU_C : 1.0f));
    wi += 2;
    VQ_TRY(upload_h16(L.w_fc2, weights[wi++], H * M, f16_mask & DT_FC2, VQ_GELU_FOLD ? 1.0f / QUICK_GELU_C : 1.0f));
    return upload_f32(L.b_fc2, weights[wi++], H);
}

// Patch weights absorb ToTensor (/255) and Normalize ((x-mean)/std): the patchify kernel stores (pixel-128), so
// W' = W/(255 std_c), bias = sum W (128/255-mean_c)/std_c.
int upload_patch_embedding(vq_encoder* e, const float* wp) {
    static const double mean[3] = {0.48145466, 0.4578275, 0.40821073};
    static const double stdv[3] = {0.26862954, 0.26130258, 0.27577711};
    const size_t H = e->cfg.hidden;
    const int pp = e->cfg.patch_size * e->cfg.patch_size, patch_k = e->patch_k;
    const bool f16 = e->opt.f16_mask & DT_PATCH;
    std::vector<uint16_t> w16(H * patch_k);
    std::vector<float> bias(H);
    // fp16 patch weights: W/(255 std) ~ 1e-4 for trained and seeded weights alike, i.e. inside fp16's subnormal range
    // (< 6.1e-5 loses mantissa bits).  Scale by the power of two that puts the largest |W'| just under 2^14; the GEMM
    // epilogue multiplies the fp32 accumulator by 2^-s (exact).  bf16 has fp32's exponent range: no scale.
    int pshift = 0;
    if (f16) {
        double amax = 0.0;
        for (size_t n = 0; n < H; ++n)
            for (int ch = 0; ch < 3; ++ch)
                for (int i = 0; i < pp; ++i) amax = std::max(amax, std::fabs((double)wp[(n * 3 + ch) * pp + i]) / (255.0 * stdv[ch]));
        if (amax > 0.0 && std::isfinite(amax)) pshift = std::min(24, std::max(0, (int)std::floor(std::log2(16000.0 / amax))));
    }
    e->patch_unscale = (float)std::ldexp(1.0, -pshift);
    const double pscale = std::ldexp(1.0, pshift);
    for (size_t n = 0; n < H; ++n) {
        double b = 0.0;
        for (int ch = 0; ch < 3; ++ch)
            for (int i = 0; i < pp; ++i) {
                const double w = wp[(n * 3 + ch) * pp + i];
                w16[n * patch_k + ch * pp + i] = f16 ? __builtin_bit_cast(uint16_t, (_Float16)(float)(w * pscale / (255.0 * stdv[ch])))
                                                     : f32_to_bf16_rne((float)(w / (255.0 * stdv[ch])));
                b += w * (128.0 / 255.0 - mean[ch]) / stdv[ch];
            }
        bias[n] = (float)b;
    }
    hipError_t he = hipMemcpy(e->w_patch, w16.data(), w16.size() * 2, hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(VQ_ERR_HIP, "weight upload failed: %s", hipGetErrorString(he));
    return upload_f32(e->b_patch, bias.data(), H);
}

// Every weight tensor, in the order of weights.py (weight_shapes / text_weight_shapes), into the buffers place_weights carved.
int upload_weights(vq_encoder* e, const float* const* weights) {
    const vq_vit_config& c = e->cfg;
    const size_t H = c.hidden;
    int wi = 0;
    if (e->is_text) {
        VQ_TRY(upload_f32(e->tok_emb, weights[wi++], (size_t)e->vocab * H));
    } else {
        VQ_TRY(upload_f32(e->cls, weights[wi++], H));
        VQ_TRY(upload_patch_embedding(e, weights[wi++]));
    }
    VQ_TRY(upload_f32(e->pos, weights[wi++], (size_t)e->tokens * H));
    if (!e->is_text) {
        VQ_TRY(upload_f32(e->pre_g, weights[wi++], H));
        VQ_TRY(upload_f32(e->pre_b, weights[wi++], H));
    }
    const float qscale = 1.0f / std::sqrt((float)(c.hidden / c.heads));   // 0.125: exact in bf16
    for (const LayerW& L : e->layers) VQ_TRY(upload_layer(L, e->opt.f16_mask, weights, wi, H, c.mlp, qscale));
    VQ_TRY(upload_f32(e->post_g, weights[wi++], H));     // text: final_layer_norm
    VQ_TRY(upload_f32(e->post_b, weights[wi++], H));
    // the projection, stored transposed [hidden][proj_dim]: coalesced reads in pool_project_kernel
    const float* wp = weights[wi++];
    std::vector<float> wt((size_t)c.proj_dim * H);
    for (int o = 0; o < c.proj_dim; ++o)
        for (size_t k = 0; k < H; ++k) wt[k * c.proj_dim + o] = wp[(size_t)o * H + k];
    return upload_f32(e->w_proj, wt.data(), wt.size());
}

template <class Fn> static inline int by_f16(bool f16, Fn&& fn) {
    return f16 ? fn(std::true_type{}) : fn(std::false_type{});
}
template <class Fn> static inline int by_f16(bool in_f16, bool out_f16, Fn&& fn) {      // operand type F, epilogue output type FO
    return by_f16(in_f16, [&](auto F) { return by_f16(out_f16, [&](auto FO) { return fn(F, FO); }); });
}
#define VQ_F16(tag) (decltype(tag)::value)

// The epilogue of a full-row residual GEMM (SITE 0: out_proj, 1: fc2) for a residual mode.  The split forms exist with fp16
// outputs only, and per site only those a pass asks for: out_proj is never the one that writes the fp32 x again, fc2 never the first.
template <int SITE, bool F16, class Go>
int with_residual_epi(int mode, float* x, int H, const float* bias, uint16_t* xh, const LnPartials& part, uint16_t* xl, Go&& go) {
    if constexpr (F16) {
        constexpr int BOTH = RS_IN_SPLIT | RS_OUT_SPLIT, EDGE = SITE == 0 ? (int)RS_OUT_SPLIT : (RS_IN_SPLIT | RS_OUT_F32);
        if (mode == BOTH) return go(EpiBiasResidualLnF32<SITE, true, BOTH>{x, H, bias, xh, part, xl});
        if (mode == EDGE) return go(EpiBiasResidualLnF32<SITE, true, EDGE>{x, H, bias, xh, part, xl});
    }
    return go(EpiBiasResidualLnF32<SITE, F16>{x, H, bias, xh, part});
}

// plan_forward decides; what follows launches.
template <int NV>
int run_forward(vq_encoder* e, const uint8_t* d_frames, int n, int swap_rb, float* d_out_f32, uint16_t* d_out_f16, const int* d_ids) {
    const vq_vit_config& c = e->cfg;
    const EncPlan p = plan_forward(*e, e->opt, n);
    hipStream_t st = e->stream;
    const int H = c.hidden, T = e->tokens, rows = p.rows, mask = e->opt.f16_mask;
    const bool fP = mask & DT_PATCH, fQ = mask & DT_QKV, fA = mask & DT_ATTN, f1 = mask & DT_FC1, f2 = mask & DT_FC2;
    const LnPartials part{e->ps, e->rows_pad};
    const int granules = H / 64;
    const float inv_h = 1.0f / (float)H;
    // a tower GEMM C[M][N] = A[M][K] W[N][K]^T with operand type F, epilogue `epi` and the plan's kernel id
    auto gemm = [&](auto F, const uint16_t* A, const uint16_t* W, int M, int N, int K, const auto& epi, int id) {
        return launch_gemm_auto<VQ_F16(F)>(st, A, K, W, K, M, N, K, epi, id);
    };
    // out_proj (site 0) / fc2 (site 1) + residual; writes xh and the row partials for the LayerNorm folded into the next GEMM
    auto residual = [&](auto site, bool f_in, bool f_out, const uint16_t* A, const uint16_t* W, const float* bias, int M, int K, int mode, int id) {
        Prof pr(e, decltype(site)::value == 0 ? C_GEMM_OUT : C_GEMM_FC2);
        return by_f16(f_in, f_out, [&](auto F, auto FO) {
            return with_residual_epi<decltype(site)::value, VQ_F16(FO)>(mode, e->x, H, bias, e->h, part, e->xl, [&](auto epi) { return gemm(F, A, W, M, H, K, epi, id); });
        });
    };
    auto fc1 = [&](int cls, const LayerW& L, int M, int id) {      // E7: LN2 (folded) + fc1 + quick_gelu on xh
        Prof pr(e, cls);
        return by_f16(f1, f2, [&](auto F, auto FO) {
            return gemm(F, e->h, L.w_fc1, M, c.mlp, H, EpiLnH16<VQ_F16(FO), true>{e->mlp, c.mlp, L.c2_fc1, L.c1_fc1, part, granules, inv_h, c.ln_eps}, id);
        });
    };
    if (e->is_text) {
        Prof pr(e, C_EMBED_FINISH);
        by_f16(fQ, [&](auto F) {
            hipLaunchKernelGGL((embed_tokens_kernel<NV, VQ_F16(F)>), dim3(cdiv(rows, 4)), dim3(256), 0, st, d_ids, e->tok_emb, e->pos, e->x, e->h, part, rows, T, e->vocab);
            return 0;
        });
        hipLaunchKernelGGL(eos_rows_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, d_ids, e->d_rowidx, n, T, e->eos_id);
    } else {
        {   // E1/E2 + im2col: uint8 frames -> 16-bit patch rows (aliases the MLP buffer)
            Prof pr(e, C_PATCHIFY);
            by_f16(fP, [&](auto F) {
                const int64_t total = p.patchify == PATCHIFY_U8 ? (int64_t)n * c.image_size * (c.image_size / 8) : (int64_t)n * e->patches * 3 * c.patch_size;
                const int blocks = (int)std::min<int64_t>((total + 255) / 256, 256 * 16);
                if (p.patchify == PATCHIFY_U8)
                    hipLaunchKernelGGL(patchify_u8_kernel<VQ_F16(F)>, dim3(blocks), dim3(256), 0, st, d_frames, e->mlp, n, c.image_size, c.patch_size, swap_rb);
                else
                    hipLaunchKernelGGL(patchify_generic_kernel<VQ_F16(F)>, dim3(blocks), dim3(256), 0, st, d_frames, e->mlp, n, c.image_size, c.patch_size, e->patch_k, swap_rb);
                return 0;
            });
        }
        {   // E3: patch-embedding conv as a GEMM, epilogue scatters into token rows + position embedding
            Prof pr(e, C_GEMM_PATCH);
            VQ_TRY(by_f16(fP, [&](auto F) {
                return gemm(F, e->mlp, e->w_patch, p.prows_gemm, H, e->patch_k, EpiPatchEmbedF32{e->x, H, e->b_patch, e->pos, e->patches, T, p.prows, e->patch_unscale}, p.k_patch);
            }));
        }
        {   // CLS row, pre_layrnorm (in place); xh + row partials for the LN1 folded into layer 0's qkv GEMM
            Prof pr(e, C_EMBED_FINISH);
            by_f16(fQ, [&](auto F) {
                hipLaunchKernelGGL((embed_finish_kernel<NV, VQ_F16(F)>), dim3(cdiv(rows, 4)), dim3(256), 0, st, e->x, e->h, e->cls, e->pos, e->pre_g, e->pre_b, part, rows, T, c.ln_eps);
                return 0;
            });
        }
    }
    e->h_is_f16 = fQ;
    for (int l = 0; l < p.layers_run; ++l) {
        const LayerW& L = e->layers[l];
        {   // E5/E6: LN1 (folded) + fused q|k|v projection (q pre-scaled by d_h^-0.5 through its weights) on xh
            Prof pr(e, C_GEMM_QKV);
            VQ_TRY(by_f16(fQ, fA, [&](auto F, auto FO) {
                return gemm(F, e->h, L.w_qkv, p.rows_gemm, 3 * H, H, EpiLnH16<VQ_F16(FO), false>{e->qkv, 3 * H, L.c2_qkv, L.c1_qkv, part, granules, inv_h, c.ln_eps}, p.k_qkv);
            }));
        }
        {
            Prof pr(e, C_ATTENTION);
            by_f16(fA, [&](auto F) {
                constexpr bool F16 = VQ_F16(F);
                const int q_tiles = cdiv(T, 64), q_groups = cdiv(q_tiles, 4), q_tiles32 = cdiv(T, 32), q_groups32 = cdiv(q_tiles32, 4);
                const int units = n * c.heads * q_tiles;
                const dim3 tile_grid(n * (c.heads / 4)), wg_grid(n * c.heads * q_groups), wg32_grid(n * c.heads * q_groups32), wg(256);
                if (p.attention == AK_TEXT_WG)
                    hipLaunchKernelGGL((attention_stream_wg_kernel<F16, true>), wg_grid, wg, 0, st, e->qkv, e->att, T, H, c.heads, q_tiles, q_groups);
                else if (p.attention == AK_TILE50)
                    hipLaunchKernelGGL((attention_tile_kernel<F16, 50>), tile_grid, wg, 0, st, e->qkv, e->att, H, c.heads);
                else if (p.attention == AK_T64)
                    hipLaunchKernelGGL(attention_t64_kernel<F16>, tile_grid, wg, 0, st, e->qkv, e->att, T, H, c.heads);
                else if (p.attention == AK_STREAM)
                    hipLaunchKernelGGL((attention_stream_kernel<F16, false>), dim3(cdiv(units, 4)), wg, 0, st, e->qkv, e->att, T, H, c.heads, q_tiles, units);
                else if (p.attention == AK_WG32)      // 32 query rows per wave, three waves per SIMD (encoder_kernels.h)
                    hipLaunchKernelGGL((attention_stream_wg_kernel<F16, false, 2>), wg32_grid, wg, 0, st, e->qkv, e->att, T, H, c.heads, q_tiles32, q_groups32);
                else
                    hipLaunchKernelGGL((attention_stream_wg_kernel<F16, false>), wg_grid, wg, 0, st, e->qkv, e->att, T, H, c.heads, q_tiles, q_groups);
                return 0;
            });
        }
        if (p.cls_only_last && l == p.layers_run - 1) {      // the last block on the n CLS rows (plan_forward)
            {   // attention rows of the CLS tokens -> compact operand (the q|k|v buffer is free now); x, xh (compact) out
                Prof pr(e, C_LAST_CLS);
                hipLaunchKernelGGL(gather_rows_h16_kernel, dim3(cdiv(n * (H / 8), 256)), dim3(256), 0, st, e->att, e->qkv, n, H, T);
                VQ_TRY(by_f16(fA, f1, [&](auto F, auto FO) {
                    return gemm(F, e->qkv, L.w_out, p.rows_cls, H, H, EpiBiasResidualClsLnF32<VQ_F16(FO)>{e->x, H, T, L.b_out, n, e->h, part}, e->opt.gemm_force);
                }));
                e->h_is_f16 = f1;
            }
            VQ_TRY(fc1(C_LAST_CLS, L, p.rows_cls, e->opt.gemm_force));
            Prof pr(e, C_LAST_CLS);
            if (p.fc2_splits) {   // partial planes live in the (now free) q|k|v buffer, summed in slice order by the reduce kernel
                float* planes = (float*)e->qkv;
                const int64_t plane = (int64_t)p.rows_cls * H;
                VQ_TRY(by_f16(f2, [&](auto F) {
                    return launch_gemm_tn_splitk<VQ_F16(F)>(st, e->mlp, c.mlp, L.w_fc2, c.mlp, p.rows_cls, H, c.mlp, p.fc2_splits, EpiSplitKPartialF32{planes, H, plane});
                }));
                hipLaunchKernelGGL(splitk_reduce_residual_cls_kernel, dim3(cdiv((int64_t)n * (H / 4), 256)), dim3(256), 0, st, planes, plane, p.fc2_splits, e->x, L.b_fc2, H, T, n);
            } else {
                VQ_TRY(by_f16(f2, [&](auto F) {
                    return gemm(F, e->mlp, L.w_fc2, p.rows_cls, H, c.mlp, EpiBiasResidualClsF32{e->x, H, T, L.b_fc2, n}, e->opt.gemm_force);
                }));
            }
            break;
        }
        VQ_TRY(residual(std::integral_constant<int, 0>{}, fA, f1, e->att, L.w_out, L.b_out, p.rows_out, H, resid_mode(p, l, false), p.k_out));
        e->h_is_f16 = f1;
        VQ_TRY(fc1(C_GEMM_FC1, L, p.rows_gemm, p.k_fc1));
        VQ_TRY(residual(std::integral_constant<int, 1>{}, f2, fQ, e->mlp, L.w_fc2, L.b_fc2, p.rows_fc2, c.mlp, resid_mode(p, l, true), p.k_fc2));
        e->h_is_f16 = fQ;
    }
    {   // E8-E10
        Prof pr(e, C_POOL);
        hipLaunchKernelGGL((pool_project_kernel<NV>), dim3(cdiv(n, POOL_IMGS), cdiv(c.proj_dim, POOL_CHUNK)), dim3(256), 0, st, e->x, e->post_g, e->post_b,
                           e->w_proj, d_out_f32, n, T, c.proj_dim, c.ln_eps, e->d_rowidx);      // d_rowidx: the EOS rows of the text tower, null for images
        hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, d_out_f32, d_out_f16, n, c.proj_dim);
    }
    VQ_HIP(hipGetLastError());
    e->stream_split = p.stream_left_split;
    return 0;
}

int forward(vq_encoder* e, const uint8_t* d_frames, int n, int swap_rb, float* d_out_f32, uint16_t* d_out_f16, const int* d_ids = nullptr) {
    switch (e->cfg.hidden / 256) {
        case 2: return run_forward<2>(e, d_frames, n, swap_rb, d_out_f32, d_out_f16, d_ids);
        case 3: return run_forward<3>(e, d_frames, n, swap_rb, d_out_f32, d_out_f16, d_ids);
        case 4: return run_forward<4>(e, d_frames, n, swap_rb, d_out_f32, d_out_f16, d_ids);
        default: return fail(VQ_ERR_INVALID, "unsupported hidden size %d", e->cfg.hidden);
    }
}

// One device pass per max_batch slice of n inputs: upload(done, cur) enqueues the slice's input on the handle's stream, then
// forward -> download to out -> synchronise.
template <class Upload>
int encode_slices(vq_encoder* e, int n, int swap_rb, float* out, Upload&& upload) {
    const size_t dim = e->cfg.proj_dim;
    for (int done = 0; done < n; done += e->max_batch) {
        const int cur = std::min(e->max_batch, n - done);
        VQ_TRY(upload(done, cur));
        VQ_TRY(forward(e, e->d_frames, cur, swap_rb, e->d_out, nullptr, e->d_ids));
        VQ_HIP(hipMemcpyAsync(out + done * dim, e->d_out, cur * dim * 4, hipMemcpyDeviceToHost, e->stream));
        VQ_HIP(hipStreamSynchronize(e->stream));
    }
    return 0;
}

// create flags / $VQ_AMD_DTYPE -> DT_* mask.  VQ_ENC_FP16: every group; VQ_ENC_F16_* bits: that group.
// $VQ_AMD_DTYPE = bf16 | fp16 | mixed | mask:<int> overrides the flags (experiments, bench.py --dtype).
int dtype_mask_from(int flags) {
    int mask = (flags & VQ_ENC_FP16) ? DT_ALL : ((flags >> 8) & DT_ALL);
    if (const char* dt = getenv("VQ_AMD_DTYPE")) {
        if (!strcmp(dt, "fp16") || !strcmp(dt, "f16")) mask = DT_ALL;
        else if (!strcmp(dt, "bf16")) mask = 0;
        else if (!strcmp(dt, "mixed")) mask = (VQ_ENC_MIXED >> 8) & DT_ALL;
        else if (!strncmp(dt, "mask:", 5)) mask = atoi(dt + 5) & DT_ALL;
    }
    return mask;
}

// What a new handle takes from its create flags and the environment.  A shared handle (`parent`) takes the attention
// and prune switches and the operand types from the handle whose weights it uses (they are already stored in those
// types); the text tower has no concurrent mode and no attention or prune switches.
EncOptions create_options(bool is_text, int flags, const EncOptions* parent) {
    EncOptions o;
    if (!is_text && (flags & VQ_ENC_CONCURRENT)) o.gemm_force = GK_AUTO_NO160;
    if (const char* gf = getenv("VQ_AMD_GEMM")) o.gemm_force = atoi(gf);
    if (const char* rs = getenv("VQ_AMD_RESID")) o.split_resid = strcmp(rs, "f32") != 0;
#ifdef VQ_DIAG
    if (const char* gm = getenv("VQ_AMD_GEMM24")) o.gemm24_mask = atoi(gm);
#endif
    if (parent) {
        o.attn = parent->attn; o.prune_last = parent->prune_last; o.f16_mask = parent->f16_mask;
        return o;
    }
    if (!is_text) {
        if (const char* at = getenv("VQ_AMD_ATTN")) o.attn = !strcmp(at, "simple") ? ATTN_SIMPLE : !strcmp(at, "q64") ? ATTN_Q64 : !strcmp(at, "t64") ? ATTN_T64 : ATTN_DEFAULT;
        if (const char* fl = getenv("VQ_AMD_FULL_LAST_LAYER")) o.prune_last = atoi(fl) == 0;
    }
    o.f16_mask = dtype_mask_from(flags);
    return o;
}

// The argument checks of both towers, and the geometry that follows from them.  g arrives with cfg, is_text and max_batch set
// (the text tower: tokens, vocab and eos_id too); n_weights < 0: no weights to count.
int tower_geometry(const char* who, EncGeometry& g, int n_weights) {
    const vq_vit_config& c = g.cfg;
    const int n_expected = (g.is_text ? 2 : 5) + 16 * c.layers + 3;
    VQ_CHECK(c.layers > 0 && (n_weights < 0 || n_weights == n_expected), "%s: expected %d weight tensors, got %d", who, n_expected, n_weights);
    VQ_CHECK(g.max_batch > 0 && g.max_batch <= 8192, "%s: max_batch %d out of range", who, g.max_batch);
    if (!g.is_text) {
        VQ_CHECK(c.image_size > 0 && c.patch_size > 0 && c.image_size % c.patch_size == 0,
                 "%s: image %d is not a multiple of patch %d", who, c.image_size, c.patch_size);
        const int grid = c.image_size / c.patch_size;
        g.patches = grid * grid; g.tokens = g.patches + 1;
        VQ_CHECK(g.tokens <= 4096, "%s: %d tokens is beyond what this build sizes for", who, g.tokens);
        g.patch_k = (int)round_up(3 * c.patch_size * c.patch_size, 2 * G2_BK);     // zero-padded K (ViT-L/14: 588 -> 640)
    }
    VQ_CHECK(c.hidden % c.heads == 0 && c.hidden / c.heads == 64, "%s: head_dim must be 64", who);
    VQ_CHECK(((g.is_text && c.hidden == 512) || c.hidden == 768 || c.hidden == 1024) && c.mlp % (g.is_text ? 256 : 128) == 0,
             "%s: hidden %d / mlp %d unsupported", who, c.hidden, c.mlp);
    if (g.is_text) VQ_CHECK(g.tokens > 0 && g.tokens <= 4096 && g.vocab > 0, "%s: bad vocabulary/positions", who);
    VQ_CHECK(c.proj_dim > 0 && c.proj_dim <= 4096, "%s: proj_dim %d out of range", who, c.proj_dim);
    g.rows_pad = round_up((int64_t)g.max_batch * g.tokens + (G5_BM - 1), 256);     // room for 256- and 160-row padding
    g.prow_pad = round_up((int64_t)g.max_batch * g.patches, 256);
    return 0;
}

EncGeometry text_geometry_in(const vq_text_config& t, int max_batch) {
    EncGeometry g;
    g.is_text = true;
    g.cfg = vq_vit_config{0, 0, t.hidden, t.mlp, t.layers, t.heads, t.proj_dim, t.ln_eps};
    g.tokens = t.max_positions; g.vocab = t.vocab; g.eos_id = t.eos_token_id; g.max_batch = max_batch;
    return g;
}

// The arena (sized by the layout that then carves it), the stream, and the weights unless they are another handle's.
int open_handle(vq_encoder* e, const char* who, const float* const* weights) {
    const size_t bytes = arena_bytes(*e, weights != nullptr);
    void* base = nullptr;
    hipError_t he = hipMalloc(&base, bytes);
    if (he != hipSuccess) return fail(VQ_ERR_OOM, "%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(he));
    e->arena.base = (uintptr_t)base; e->arena.size = bytes;
    e->arena_owner = std::shared_ptr<void>(base, [](void* p) { (void)hipFree(p); });
    he = hipMemset(base, 0, bytes);
    if (he != hipSuccess) return fail(VQ_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(he));
    he = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking);
    if (he != hipSuccess) return fail(VQ_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(he));
    e->stream = e->own_stream;
    if (weights) place_weights(e->arena, *e, *e);
    place_workspace(e->arena, *e, *e);
    return weights ? upload_weights(e, weights) : 0;
}

// A new handle of geometry g: its arena and stream; on any failure what exists of it goes through vq_encoder_destroy.
int create_handle(const char* who, const EncGeometry& g, const EncOptions& opt, const float* const* weights, const vq_encoder* parent, vq_encoder** out) {
    vq_encoder* e = new vq_encoder();
    static_cast<EncGeometry&>(*e) = g;
    e->opt = opt;
    if (parent) {
        static_cast<EncWeights&>(*e) = *parent;
        e->patch_unscale = parent->patch_unscale;
        e->weights_owner = parent->weights_owner ? parent->weights_owner : parent->arena_owner;   // a clone of a clone still pins the original weights
    }
    const int rc = open_handle(e, who, weights);
    if (rc) { vq_encoder_destroy(e); return rc; }
    *out = e;
    return 0;
}

}  // namespace

extern "C" {

int vq_encoder_create(const vq_vit_config* cfg, const float* const* weights, int n_weights, int max_batch, vq_encoder** out) {
    return vq_encoder_create_ex(cfg, weights, n_weights, max_batch, 0, out);
}

int vq_encoder_create_ex(const vq_vit_config* cfg, const float* const* weights, int n_weights, int max_batch, int flags, vq_encoder** out) {
    VQ_TRY(require_init());
    VQ_CHECK(cfg && weights && out, "vq_encoder_create: null argument");
    EncGeometry g;
    g.cfg = *cfg; g.max_batch = max_batch;
    VQ_TRY(tower_geometry("vq_encoder_create", g, n_weights));
    return create_handle("vq_encoder_create", g, create_options(false, flags, nullptr), weights, nullptr, out);
}

// A second handle on the SAME weights: own stream, own workspace, own profiling state.  What a caller that keeps
// several batches in flight needs (bench.py --streams, the ingest loop's alternating handles) without copying the
// 176 MB of weights per handle.  The weights stay alive until the last handle that uses them is destroyed.
int vq_encoder_create_shared(vq_encoder* parent, int max_batch, int flags, vq_encoder** out) {
    VQ_TRY(require_init());
    VQ_CHECK(parent && out && !parent->is_text, "vq_encoder_create_shared: needs an image-encoder handle");
    EncGeometry g = *parent;
    g.max_batch = max_batch;
    VQ_TRY(tower_geometry("vq_encoder_create_shared", g, -1));
    return create_handle("vq_encoder_create_shared", g, create_options(false, flags, &parent->opt), nullptr, parent, out);
}

int vq_text_encoder_create(const vq_text_config* cfg, const float* const* weights, int n_weights, int max_batch, int flags, vq_text_encoder** out) {
    VQ_TRY(require_init());
    VQ_CHECK(cfg && weights && out, "vq_text_encoder_create: null argument");
    EncGeometry g = text_geometry_in(*cfg, max_batch);
    VQ_TRY(tower_geometry("vq_text_encoder_create", g, n_weights));
    return create_handle("vq_text_encoder_create", g, create_options(true, flags, nullptr), weights, nullptr, out);
}

// plan_forward's answer and the layout for a handle that is never made (include/vq_amd.h).
int vq_debug_encoder_plan(const vq_vit_config* vit, const vq_text_config* text, int max_batch, int n, int flags, int shared,
                          int run_layers, int keep_stream, vq_encoder_plan* out, int* resid_modes) {
    VQ_CHECK((vit != nullptr) != (text != nullptr) && out && !(text && shared), "vq_debug_encoder_plan: one of a vit and a text config, and a result");
    EncGeometry g;
    if (text) g = text_geometry_in(*text, max_batch);
    else { g.cfg = *vit; g.max_batch = max_batch; }
    VQ_TRY(tower_geometry("vq_debug_encoder_plan", g, -1));
    VQ_CHECK(n > 0 && n <= max_batch, "vq_debug_encoder_plan: n=%d outside (0, max_batch=%d]", n, max_batch);
    EncOptions o = create_options(g.is_text, flags, nullptr);
    o.run_layers = run_layers; o.keep_stream = keep_stream != 0;
    const EncPlan p = plan_forward(g, o, n);
    EncWorkspace ws;      // on a null base: offsets
    const size_t bytes = arena_bytes(g, !shared, &ws);
    auto off = [](const void* q) { return (int64_t)(uintptr_t)q; };
    *out = vq_encoder_plan{p.rows, p.rows_gemm, p.rows_out, p.rows_fc2, p.prows, p.prows_gemm, p.rows_cls,
                           p.k_patch, p.k_qkv, p.k_out, p.k_fc1, p.k_fc2, o.gemm_force, p.patchify, p.attention, p.layers_run,
                           p.cls_only_last, p.fc2_splits, p.split, p.stream_left_split, g.rows_pad, g.prow_pad, (int64_t)bytes,
                           (int64_t)(bytes - arena_tail_bytes(g)), g.is_text ? off(ws.d_ids) : off(ws.d_frames), g.is_text ? off(ws.d_rowidx) : -1,
                           off(ws.ps), off(ws.x), off(ws.d_out), off(ws.h), off(ws.xl), off(ws.qkv), off(ws.att), off(ws.mlp)};
    const int full_blocks = p.layers_run - (p.cls_only_last ? 1 : 0);
    for (int l = 0; resid_modes && l < g.cfg.layers; ++l)
        for (int fc2 = 0; fc2 < 2; ++fc2) resid_modes[2 * l + fc2] = l < full_blocks ? resid_mode(p, l, fc2 != 0) : -1;
    return 0;
}

int vq_text_encoder_encode_ids(vq_text_encoder* e, const int32_t* ids, int n, int seq_len, float* out) {
    VQ_TRY(require_init());
    VQ_CHECK(e && e->is_text, "vq_text_encoder_encode_ids: not a text encoder handle");
    VQ_CHECK(n >= 0 && (n == 0 || (ids && out)), "vq_text_encoder_encode_ids: bad argument");
    VQ_CHECK(seq_len > 0 && seq_len <= e->tokens, "vq_text_encoder_encode_ids: seq_len %d outside (0, %d]", seq_len, e->tokens);
    std::lock_guard<std::mutex> lk(e->mu);
    const int T = e->tokens;
    std::vector<int32_t> padded;
    return encode_slices(e, n, 0, out, [&](int done, int cur) {
        padded.assign((size_t)cur * T, e->eos_id);                       // pad with eos: invisible to the EOS position (causal)
        for (int i = 0; i < cur; ++i)
            std::copy(ids + (size_t)(done + i) * seq_len, ids + (size_t)(done + i + 1) * seq_len, padded.begin() + (size_t)i * T);
        VQ_HIP(hipMemcpyAsync(e->d_ids, padded.data(), padded.size() * 4, hipMemcpyHostToDevice, e->stream));
        return 0;
    });
}

int vq_text_encoder_destroy(vq_text_encoder* e) { return vq_encoder_destroy(e); }

int vq_encoder_destroy(vq_encoder* e) {
    if (!e) return 0;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    for (auto& ev : e->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto ev : e->pool) (void)hipEventDestroy(ev);
    e->arena_owner.reset();          // frees the arena unless a shared handle still reads its weights
    e->weights_owner.reset();
    for (int i = 0; i < 2; ++i) if (e->h_stage[i]) (void)hipHostFree(e->h_stage[i]);
    if (e->h_out_stage) (void)hipHostFree(e->h_out_stage);
    if (e->copy_stream) { (void)hipStreamSynchronize(e->copy_stream); (void)hipStreamDestroy(e->copy_stream); }
    for (int i = 0; i < 2; ++i) {
        if (e->d_slot_frames[i]) (void)hipFree(e->d_slot_frames[i]);
        if (e->h_slot_out[i]) (void)hipHostFree(e->h_slot_out[i]);
        if (e->ev_h2d[i]) (void)hipEventDestroy(e->ev_h2d[i]);
        if (e->ev_fwd[i]) (void)hipEventDestroy(e->ev_fwd[i]);
        if (e->ev_done[i]) (void)hipEventDestroy(e->ev_done[i]);
    }
    delete e;
    return 0;
}

int vq_encoder_output_dim(vq_encoder* e, int* dim) {
    VQ_CHECK(e && dim, "vq_encoder_output_dim: null argument");
    *dim = e->cfg.proj_dim;
    return 0;
}

int vq_encoder_encode_u8_device(vq_encoder* e, const void* d_frames, int n, int swap_rb, void* d_out_f32, void* d_out_f16) {
    VQ_TRY(require_init());
    VQ_CHECK(e && d_frames && d_out_f32, "vq_encoder_encode_u8_device: null argument");
    VQ_CHECK(!e->is_text, "vq_encoder_encode_u8_device: this is a text encoder handle");
    VQ_CHECK(n > 0 && n <= e->max_batch, "vq_encoder_encode_u8_device: n=%d outside (0, max_batch=%d]", n, e->max_batch);
    std::lock_guard<std::mutex> lk(e->mu);
    return forward(e, (const uint8_t*)d_frames, n, swap_rb, (float*)d_out_f32, (uint16_t*)d_out_f16);
}

int vq_encoder_encode_u8(vq_encoder* e, const uint8_t* frames, int n, int swap_rb, float* out) {
    VQ_TRY(require_init());
    VQ_CHECK(e && n >= 0 && (n == 0 || (frames && out)), "vq_encoder_encode_u8: bad argument");
    VQ_CHECK(!e->is_text, "vq_encoder_encode_u8: this is a text encoder handle");
    std::lock_guard<std::mutex> lk(e->mu);
    return encode_slices(e, n, swap_rb, out, [&](int done, int cur) {
        VQ_HIP(hipMemcpyAsync(e->d_frames, frames + done * e->frame_bytes(), cur * e->frame_bytes(), hipMemcpyHostToDevice, e->stream));
        return 0;
    });
}

int vq_encoder_staging(vq_encoder* e, int slot, uint8_t** host_ptr, size_t* bytes) {
    VQ_TRY(require_init());
    VQ_CHECK(e && !e->is_text && host_ptr && bytes && (slot == 0 || slot == 1), "vq_encoder_staging: bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    const size_t sz = e->max_batch * e->frame_bytes();
    if (!e->h_stage[slot]) VQ_HIP(hipHostMalloc((void**)&e->h_stage[slot], sz));
    if (!e->h_out_stage) VQ_HIP(hipHostMalloc((void**)&e->h_out_stage, (size_t)e->max_batch * e->cfg.proj_dim * 4));
    *host_ptr = e->h_stage[slot];
    *bytes = sz;
    return 0;
}

int vq_encoder_encode_staged(vq_encoder* e, int slot, int n, int swap_rb, float* out) {
    VQ_TRY(require_init());
    VQ_CHECK(e && !e->is_text && out && (slot == 0 || slot == 1) && e->h_stage[slot], "vq_encoder_encode_staged: bad argument / slot not staged");
    VQ_CHECK(n > 0 && n <= e->max_batch, "vq_encoder_encode_staged: n=%d outside (0, max_batch=%d]", n, e->max_batch);
    std::lock_guard<std::mutex> lk(e->mu);
    VQ_TRY(encode_slices(e, n, swap_rb, e->h_out_stage, [&](int, int cur) {
        VQ_HIP(hipMemcpyAsync(e->d_frames, e->h_stage[slot], cur * e->frame_bytes(), hipMemcpyHostToDevice, e->stream));
        return 0;
    }));
    memcpy(out, e->h_out_stage, (size_t)n * e->cfg.proj_dim * 4);
    return 0;
}

// Host gather: n separately allocated frames -> pinned staging slot, on up to n_threads threads.
int vq_encoder_stage_frames(vq_encoder* e, int slot, const uint8_t* const* frames, int n, int n_threads) {
    VQ_TRY(require_init());
    VQ_CHECK(e && !e->is_text && frames && (slot == 0 || slot == 1), "vq_encoder_stage_frames: bad argument");
    VQ_CHECK(n > 0 && n <= e->max_batch, "vq_encoder_stage_frames: n=%d outside (0, max_batch=%d]", n, e->max_batch);
    for (int i = 0; i < n; ++i) VQ_CHECK(frames[i], "vq_encoder_stage_frames: frame %d is null", i);
    uint8_t* dst = nullptr;
    size_t bytes = 0;
    VQ_TRY(vq_encoder_staging(e, slot, &dst, &bytes));
    {
        std::lock_guard<std::mutex> lk(e->mu);
        VQ_CHECK(e->slot_n[slot] == 0, "vq_encoder_stage_frames: slot %d still has a submitted batch (wait for it first)", slot);
    }
    const size_t fbytes = e->frame_bytes();
    const int nt = std::max(1, std::min(std::min(n_threads, 16), n / 8));
    auto work = [&](int t) {
        for (int i = t; i < n; i += nt) memcpy(dst + (size_t)i * fbytes, frames[i], fbytes);
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
    return 0;
}

// Asynchronous: upload slot -> forward -> download, ordered by events; the upload runs on the handle's copy
// stream so that it overlaps the forward pass of the other slot.
int vq_encoder_submit_staged(vq_encoder* e, int slot, int n, int swap_rb) {
    VQ_TRY(require_init());
    VQ_CHECK(e && !e->is_text && (slot == 0 || slot == 1) && e->h_stage[slot], "vq_encoder_submit_staged: bad argument / slot not staged");
    VQ_CHECK(n > 0 && n <= e->max_batch, "vq_encoder_submit_staged: n=%d outside (0, max_batch=%d]", n, e->max_batch);
    std::lock_guard<std::mutex> lk(e->mu);
    VQ_CHECK(e->slot_n[slot] == 0, "vq_encoder_submit_staged: slot %d already has a batch in flight", slot);
    const size_t fbytes = e->frame_bytes();
    if (!e->copy_stream) VQ_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    if (!e->d_slot_frames[slot]) {
        VQ_HIP(hipMalloc((void**)&e->d_slot_frames[slot], (size_t)e->max_batch * fbytes));
        VQ_HIP(hipHostMalloc((void**)&e->h_slot_out[slot], (size_t)e->max_batch * e->cfg.proj_dim * 4));
        VQ_HIP(hipEventCreateWithFlags(&e->ev_h2d[slot], hipEventDisableTiming));
        VQ_HIP(hipEventCreateWithFlags(&e->ev_fwd[slot], hipEventDisableTiming));
        VQ_HIP(hipEventCreateWithFlags(&e->ev_done[slot], hipEventDisableTiming));
    } else {
        VQ_HIP(hipStreamWaitEvent(e->copy_stream, e->ev_fwd[slot], 0));    // the slot's previous forward has consumed its frames
    }
    VQ_HIP(hipMemcpyAsync(e->d_slot_frames[slot], e->h_stage[slot], n * fbytes, hipMemcpyHostToDevice, e->copy_stream));
    VQ_HIP(hipEventRecord(e->ev_h2d[slot], e->copy_stream));
    VQ_HIP(hipStreamWaitEvent(e->stream, e->ev_h2d[slot], 0));
    VQ_TRY(forward(e, e->d_slot_frames[slot], n, swap_rb, e->d_out, nullptr));
    VQ_HIP(hipEventRecord(e->ev_fwd[slot], e->stream));
    VQ_HIP(hipMemcpyAsync(e->h_slot_out[slot], e->d_out, (size_t)n * e->cfg.proj_dim * 4, hipMemcpyDeviceToHost, e->stream));
    VQ_HIP(hipEventRecord(e->ev_done[slot], e->stream));
    e->slot_n[slot] = n;
    return 0;
}

int vq_encoder_wait_staged(vq_encoder* e, int slot, float* out) {
    VQ_TRY(require_init());
    VQ_CHECK(e && out && (slot == 0 || slot == 1), "vq_encoder_wait_staged: bad argument");
    int n;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        n = e->slot_n[slot];
        VQ_CHECK(n > 0, "vq_encoder_wait_staged: slot %d has no batch in flight", slot);
    }
    VQ_HIP(hipEventSynchronize(e->ev_done[slot]));
    memcpy(out, e->h_slot_out[slot], (size_t)n * e->cfg.proj_dim * 4);
    std::lock_guard<std::mutex> lk(e->mu);
    e->slot_n[slot] = 0;
    return 0;
}

int vq_encoder_synchronize(vq_encoder* e) {
    VQ_CHECK(e, "vq_encoder_synchronize: null handle");
    VQ_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int vq_encoder_set_stream(vq_encoder* e, void* hip_stream) {
    VQ_CHECK(e, "vq_encoder_set_stream: null handle");
    std::lock_guard<std::mutex> lk(e->mu);
    VQ_HIP(hipStreamSynchronize(e->stream));
    e->stream = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    return 0;
}

int vq_encoder_profile_begin(vq_encoder* e) {
    VQ_CHECK(e, "vq_encoder_profile_begin: null handle");
    std::lock_guard<std::mutex> lk(e->mu);
    VQ_HIP(hipStreamSynchronize(e->stream));
    for (auto& ev : e->events) { e->pool.push_back(ev.a); e->pool.push_back(ev.b); }
    e->events.clear();
    e->profiling = true;
    return 0;
}

int vq_encoder_profile_end(vq_encoder* e, float* ms, int* launches) {
    VQ_CHECK(e && ms && launches, "vq_encoder_profile_end: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    e->profiling = false;
    VQ_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < VQ_ENC_NCLASS; ++i) { ms[i] = 0.f; launches[i] = 0; }
    for (auto& ev : e->events) {
        float t = 0.f;
        VQ_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
        ms[ev.cls] += t; launches[ev.cls] += 1;
        e->pool.push_back(ev.a); e->pool.push_back(ev.b);
    }
    e->events.clear();
    return 0;
}

// What an event bracket measures beyond the kernel inside it: the median of 15 EMPTY brackets on the encoder's stream
// (start record, stop record, nothing between).  A bracket's elapsed time runs from the completion of the start marker to the
// completion of the stop marker, so it carries the marker-to-dispatch and completion-to-marker latencies of the command
// processor; rocprofv3's kernel durations (begin to end of the dispatch) do not.  bench.py reports both.
int vq_encoder_profile_bracket_overhead(vq_encoder* e, float* ms) {
    VQ_CHECK(e && ms, "vq_encoder_profile_bracket_overhead: null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    constexpr int N = 15;
    hipEvent_t a[N], b[N];
    for (int i = 0; i < N; ++i) { a[i] = Prof::get(e); b[i] = Prof::get(e); }
    VQ_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < N; ++i) { VQ_HIP(hipEventRecord(a[i], e->stream)); VQ_HIP(hipEventRecord(b[i], e->stream)); }
    VQ_HIP(hipStreamSynchronize(e->stream));
    float t[N];
    for (int i = 0; i < N; ++i) { VQ_HIP(hipEventElapsedTime(&t[i], a[i], b[i])); e->pool.push_back(a[i]); e->pool.push_back(b[i]); }
    std::sort(t, t + N);
    *ms = t[N / 2];
    return 0;
}

const char* vq_encoder_profile_class_name(int cls) {
    return (cls >= 0 && cls < VQ_ENC_NCLASS) ? kEncClassNames[cls] : "";
}

int vq_encoder_debug_set_layers(vq_encoder* e, int layers) {
    VQ_CHECK(e, "vq_encoder_debug_set_layers: null handle");
    e->opt.run_layers = layers;
    return 0;
}

int vq_encoder_debug_keep_stream(vq_encoder* e, int on) {
    VQ_CHECK(e, "vq_encoder_debug_keep_stream: null handle");
    e->opt.keep_stream = on != 0;
    return 0;
}

int vq_encoder_debug_stream_is_split(vq_encoder* e, int* split) {
    VQ_CHECK(e && split, "vq_encoder_debug_stream_is_split: null argument");
    *split = e->stream_split ? 1 : 0;
    return 0;
}

int vq_encoder_debug_read(vq_encoder* e, const char* name, int rows, float* out) {
    VQ_CHECK(e && name && out, "vq_encoder_debug_read: null argument");
    VQ_CHECK(rows > 0 && rows <= e->rows_pad, "vq_encoder_debug_read: rows out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    VQ_HIP(hipStreamSynchronize(e->stream));
    const size_t H = e->cfg.hidden;
    if (!strcmp(name, "x")) {
        VQ_HIP(hipMemcpy(out, e->x, (size_t)rows * H * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    if (!strcmp(name, "xl")) {                             // the raw bytes; decoding them is the reader's business
        VQ_CHECK(VQ_RESID_XL8, "vq_encoder_debug_read: 'xl' is read as bytes, and this build holds it as fp16");
        std::vector<uint8_t> bytes((size_t)rows * H);
        VQ_HIP(hipMemcpy(bytes.data(), e->xl, bytes.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < bytes.size(); ++i) out[i] = (float)bytes[i];
        return 0;
    }
    const uint16_t* src = nullptr; size_t cols = 0; bool f16 = false;
    if (!strcmp(name, "h")) { src = e->h; cols = H; f16 = e->h_is_f16; }
    else if (!strcmp(name, "qkv")) { src = e->qkv; cols = 3 * H; f16 = e->opt.f16_mask & DT_ATTN; }
    else if (!strcmp(name, "att")) { src = e->att; cols = H; f16 = e->opt.f16_mask & DT_ATTN; }
    else if (!strcmp(name, "mlp")) { src = e->mlp; cols = e->cfg.mlp; f16 = e->opt.f16_mask & DT_FC2; }
    else return fail(VQ_ERR_INVALID, "vq_encoder_debug_read: unknown buffer '%s'", name);
    std::vector<uint16_t> tmp((size_t)rows * cols);
    VQ_HIP(hipMemcpy(tmp.data(), src, tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i)
        out[i] = f16 ? (float)__builtin_bit_cast(_Float16, tmp[i]) : bf16_to_f32(tmp[i]);
    return 0;
}

}  // extern "C"

#ifdef VQ_GEMM_TOWER_STAMPS
// `make STAMPS=1` only: prints and clears the workgroup stamps gemm_tn256d_kernel collected (scripts/gemm_tower_stamps.py)
extern "C" int vq_debug_dump_gemm_stamps(void) {
    unsigned int n = 0;
    static unsigned long long h[4096 * 8];
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(vq::g_dbg_count), 4);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(vq::g_dbg_stamps), sizeof(h));
    if (n > 4096) n = 4096;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned long long* d = h + i * 8;
        fprintf(stderr, "STAMP K %llu tn %llu epi %llu prologue %llu loop %llu epilogue %llu ticks %llu wg %llu\n", d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
    }
    const unsigned int z = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(vq::g_dbg_count), &z, 4);
    return (int)n;
}
#endif
