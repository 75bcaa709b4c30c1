// Filtered exact top-k (vq_index_search_filtered, vq_index_search_grouped_filtered): the plain or grouped search restricted to
// the rows S whose group label (vq_index_set_groups) is in a caller's set, or not in it.
//
// Gather path (mode 1; mode 0 below the crossover, vq_index.hip):
//   1. The allowed groups A, ascending, and their row counts prefix-summed (soff [|A| + 1]).  An include list is small: the host
//      sorts it, drops duplicates and sums the counts from its mirror of the group offsets.  An exclude list can leave most of
//      the groups: filter_allowed_kernel flags every group not in the (sorted) list by a binary search, a three-pass exclusive
//      scan (knn_remove.h) numbers them, filter_compact_groups_kernel writes A and the counts, a second scan turns the counts
//      into soff.
//   2. filter_expand_kernel: the row list of S from the by-group CSR list, group after group (positions soff[j] .. soff[j+1]
//      hold group A[j]'s rows), and each listed row's tie word (the row, or the rank of its id: TieOrder, vq_common.h).
//   3. filter_dist_kernel: the listed rows' distances by the fixed-order fp64 chain of exact_dist_kernel (the oracle's order,
//      one rounding to fp32 at the end), so every distance is the same bits as the unfiltered search's.
//   4. Selection runs the plain path's kernels (select_small_kernel, select_chunk_kernel + merge_topk_kernel) over the list
//      positions with TieOrder {rank = the list's tie words, row = the index's rank -> row map}: a key carries the row's own
//      tie word, so the (distance, tie) order of S is the full index's order restricted to S, and the emitted row is the full
//      index's row number.  The grouped form walks the allowed groups' position ranges instead
//      (group_block_topk_kernel<true, false, true>, the exact path's group minimum and block top-k) and merges with
//      group_merge_kernel.
//   Cost: 4 B x dim per allowed row read through the list, plus the fp64 chains; nothing is read for the other rows.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "knn_grouped.h"

namespace vq {

// K[g] = 1 when group g is not in the sorted exclude list excl[0..ne), else 0; g in [0, G)
__global__ __launch_bounds__(256)
void filter_allowed_kernel(const int32_t* __restrict__ excl, int ne, int32_t G, int32_t* __restrict__ K) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = ne;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (excl[mid] < g) lo = mid + 1; else hi = mid;
        }
        K[g] = (lo < ne && excl[lo] == g) ? 0 : 1;
    }
}

// K = exclusive scan of the allowed flags (K[G] = |A|): A[K[g]] = g and cnt[K[g]] = its row count for every allowed group
__global__ __launch_bounds__(256)
void filter_compact_groups_kernel(const int32_t* __restrict__ K, int32_t G, const int32_t* __restrict__ goff, int32_t* __restrict__ A,
                                  int32_t* __restrict__ cnt) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x)
        if (K[g + 1] > K[g]) { A[K[g]] = (int32_t)g; cnt[K[g]] = goff[g + 1] - goff[g]; }
}

// One wave per allowed group: list[soff[j] + i] = the group's i-th row (by-group CSR order), tie_w[...] = that row's tie word
__global__ __launch_bounds__(256)
void filter_expand_kernel(const int32_t* __restrict__ A, const int32_t* __restrict__ soff, int nA, const int32_t* __restrict__ goff,
                          const int32_t* __restrict__ grows, const TieOrder tie, int32_t* __restrict__ list, int32_t* __restrict__ tie_w) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < nA; j += (int64_t)gridDim.x * 4) {
        const int g = A[j], b = goff[g], c = goff[g + 1] - b, o = soff[j];
        for (int i = lane; i < c; i += 64) {
            const int r = grows[b + i];
            list[o + i] = r;
            tie_w[o + i] = (int32_t)tie_of(tie, r);
        }
    }
}

// ---- distances of the listed rows ----
// Workgroup tile: 64 list positions x QG queries, 256 threads; thread (r = tid & 63, g = tid >> 6) owns position r and queries
// g * QG/4 .. +QG/4 - 1.  64-dim panels: the rows' next panel is fetched into registers (16-byte loads through the list) while
// the current one is multiplied out of LDS; the queries' panel is staged as fp64.  acc += (double)x[c] * (double)q[c] in index
// order from 0: exact_dist_kernel's chain, one rounding to fp32 at the end.
template <int QG>
__global__ __launch_bounds__(256)
void filter_dist_kernel(const float* __restrict__ rows, const int32_t* __restrict__ list, int64_t m, int dim,
                        const float* __restrict__ queries, int nq, float* __restrict__ dist /*[nq][ld]*/, int64_t ld) {
    constexpr int QPT = QG / 4;
    __shared__ float xs[64][65];
    __shared__ double qs[QG][64];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int64_t v0 = (int64_t)blockIdx.x * 64;
    const int q0 = blockIdx.y * QG;
    const int panels = (dim + 63) >> 6;
    // piece p = tid + 256 u of a 64 x 64 panel: position p >> 4, floats (p & 15) * 4 .. +3
    const float* src[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t v = v0 + ((tid + 256 * u) >> 4);
        src[u] = v < m ? rows + (int64_t)list[v] * dim : nullptr;
    }
    float4 nx[4];
    auto fetch = [&](int pi) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = pi * 64 + ((tid + 256 * u) & 15) * 4;
            nx[u] = float4{0.f, 0.f, 0.f, 0.f};
            if (src[u] && c < dim) nx[u] = *(const float4*)(src[u] + c);      // dim % 4 == 0 (vq_index_create)
        }
    };
    fetch(0);
    double acc[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) acc[j] = 0.0;
    for (int pi = 0; pi < panels; ++pi) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = tid + 256 * u, rr = p >> 4, c4 = (p & 15) * 4;
            xs[rr][c4] = nx[u].x; xs[rr][c4 + 1] = nx[u].y; xs[rr][c4 + 2] = nx[u].z; xs[rr][c4 + 3] = nx[u].w;
        }
        for (int i = tid; i < QG * 64; i += 256) {
            const int qq = i >> 6, cc = i & 63, c = pi * 64 + cc;
            qs[qq][cc] = (q0 + qq < nq && c < dim) ? (double)queries[(int64_t)(q0 + qq) * dim + c] : 0.0;
        }
        __syncthreads();
        if (pi + 1 < panels) fetch(pi + 1);
        const int lim = min(64, dim - pi * 64);
        for (int c = 0; c < lim; ++c) {
            const double xv = (double)xs[r][c];
#pragma unroll
            for (int j = 0; j < QPT; ++j) acc[j] += xv * qs[g * QPT + j][c];      // product exact in fp64
        }
        __syncthreads();
    }
    const int64_t v = v0 + r;
    if (v < m) {
#pragma unroll
        for (int j = 0; j < QPT; ++j) {
            const int q = q0 + g * QPT + j;
            if (q < nq) dist[(int64_t)q * ld + v] = 1.0f - (float)acc[j];
        }
    }
}

// ---- the allowed groups as a bitmap: bits preset to 0 (include) or 1 (exclude), then every listed group's bit toggled (the list
// is sorted and unique) ----
__global__ __launch_bounds__(256)
void filter_bitmap_kernel(const int32_t* __restrict__ sel, int ns, uint32_t* __restrict__ bits) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += gridDim.x * blockDim.x)
        atomicXor(bits + (sel[i] >> 5), 1u << (sel[i] & 31));
}

// ---- masked fp16 path of the plain form (mode 2, nq <= SCAN3_MAX_Q, dim 256 / 512 / 768) ----
// scan3_f16_top2_kernel<..., MASK> leaves per (query, stream) the top-2 fp16 keys over the stream's ALLOWED rows (MASKED: none).
// Then, per query:
//   filter_stream_threshold_kernel: T = the k-th largest stream maximum m1 (radix select over the order-preserving uint32 of
//     the scores, "no row" = 0); candidate streams = those with m1 >= T - 2E - FLT_SLACK (every stream holding an allowed row
//     when fewer than k streams do).  E = scan_eps_unit(dim) * max|row| * |q|, as the unfiltered proof.
//   filter_stream_rescore_kernel (FLT_RESCORE_SPLITS workgroups per query): every allowed row of the candidate streams gets its
//     fp16 score recomputed (fp32 accumulation of exact fp16 products: within E of the exact score, like the scan's); rows at
//     >= the threshold are re-scored by the fp64 chain and their (distance, tie) keys listed.
//   filter_stream_finalize_kernel: the k smallest listed keys -> ids / distances.
// Proof: the k streams at or above T each hold an allowed row whose fp16 score is >= T - slack (the key keeps the score's top
// 25 bits), so the k-th best allowed exact score s* is >= T - E - slack.  A row of the answer has exact score >= s* (up to the
// fp32 rounding of 1 - s, inside the slack), so its scan score and its stream's m1 are >= T - 2E - slack: its stream is a
// candidate and its recomputed score passes the same test.  Every floor here is taken over allowed rows only, so the
// unfiltered argument holds unchanged.  A query outside 0.25 <= |q|^2 <= 4 (or not finite), with more than FLT_CAND candidate
// streams or more than FLT_LIST listed rows, or with fewer listed rows than min(k, |S|), is flagged (2) and redone by the masked
// exact fallback (exact_fallback_kernel<true>); nothing is truncated.
constexpr int FLT_CAND = 2048;           // candidate streams per query (262,144 rows)
constexpr int FLT_LIST = 4096;           // re-scored rows per query
constexpr int FLT_RESCORE_SPLITS = 16;
constexpr float FLT_SLACK = 1.0f / 16384;   // 2^-14: the key's 7 dropped mantissa bits, fp32 rounding of 1 - s and of the threshold

__device__ __forceinline__ uint32_t stream_key(uint32_t bits) {          // scan key -> order-preserving uint32, 0 = no allowed row
    const float v = __builtin_bit_cast(float, bits);
    return v > -1.0e38f ? score_key(v) : 0u;
}

__global__ __launch_bounds__(256)
void filter_stream_threshold_kernel(const uint32_t* __restrict__ keys /*[q_pad][streams][2]*/, int64_t streams, int k,
                                    const float* __restrict__ queries, int dim, float eps_rows, int32_t* __restrict__ cand /*[nq][FLT_CAND]*/,
                                    int32_t* __restrict__ cand_n, float* __restrict__ cand_thr, int32_t* __restrict__ list_n,
                                    int32_t* __restrict__ flags) {
    __shared__ uint32_t hist[256];
    __shared__ float red[4];
    __shared__ uint32_t prefix_s;
    __shared__ int kr_s, cnt_s, live_s;
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint32_t* kq = keys + (size_t)q * streams * 2;
    const float* qv = queries + (size_t)q * dim;
    float s2 = 0.f;
    for (int i = tid; i < dim; i += 256) s2 += qv[i] * qv[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    if ((tid & 63) == 0) red[tid >> 6] = s2;
    if (tid == 0) { cnt_s = 0; live_s = 0; }
    __syncthreads();
    const float q2 = (red[0] + red[1]) + (red[2] + red[3]);
    if (tid == 0) list_n[q] = 0;
    if (!(q2 >= SCAN_Q2_MIN && q2 <= SCAN_Q2_MAX)) {        // outside what the fp16 bound covers (NaN included): exact redo
        if (tid == 0) { flags[q] = 2; cand_n[q] = 0; }
        return;
    }
    const float E = eps_rows * sqrtf(q2);
    int live = 0;
    for (int64_t s = tid; s < streams; s += 256) live += stream_key(kq[s * 2]) != 0u;
    if (live) atomicAdd(&live_s, live);
    __syncthreads();
    float thr = -__builtin_inff();
    if (k <= live_s) {                                      // T = the k-th largest stream maximum: radix select, 8 bits at a time
        uint32_t prefix = 0, mask = 0;
        int kr = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int64_t s = tid; s < streams; s += 256) {
                const uint32_t v = stream_key(kq[s * 2]);
                if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0;
                for (int b = 255; b >= 0; --b) {
                    const int h = (int)hist[b];
                    if (cum + h >= kr) { prefix_s = prefix | ((uint32_t)b << shift); kr_s = kr - cum; break; }
                    cum += h;
                }
            }
            __syncthreads();
            prefix = prefix_s; kr = kr_s; mask |= 255u << shift;
        }
        thr = (key_score(prefix) - 2.0f * E) - FLT_SLACK;
    }
    int32_t* cq = cand + (size_t)q * FLT_CAND;
    for (int64_t s = tid; s < streams; s += 256) {
        const uint32_t v = stream_key(kq[s * 2]);
        if (v != 0u && key_score(v) >= thr) {
            const int pos = atomicAdd(&cnt_s, 1);
            if (pos < FLT_CAND) cq[pos] = (int32_t)s;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int c = cnt_s;
        flags[q] = c > FLT_CAND ? 2 : 0;
        cand_n[q] = c > FLT_CAND ? 0 : c;
        cand_thr[q] = thr;
    }
}

__global__ __launch_bounds__(256)
void filter_stream_rescore_kernel(const uint16_t* __restrict__ Q16, const float* __restrict__ queries, const float* __restrict__ rows,
                                  const uint16_t* __restrict__ rows16, int64_t n, int dim, const GroupMask mask,
                                  const int32_t* __restrict__ cand, const int32_t* __restrict__ cand_n, const float* __restrict__ cand_thr,
                                  const int32_t* __restrict__ flags, uint64_t* __restrict__ list /*[nq][FLT_LIST]*/,
                                  int32_t* __restrict__ list_n, const TieOrder tie) {
    __shared__ float qs[768];
    const int q = blockIdx.y, tid = threadIdx.x;
    if (flags[q] != 0) return;                              // block-uniform
    const int c = cand_n[q];
    if (c == 0) return;
    for (int i = tid; i < dim; i += 256) qs[i] = (float)__builtin_bit_cast(_Float16, Q16[(size_t)q * dim + i]);
    __syncthreads();
    const int64_t total = (int64_t)c * 128;
    const int64_t v0 = total * blockIdx.x / gridDim.x, v1 = total * (blockIdx.x + 1) / gridDim.x;
    const float thr = cand_thr[q];
    const float* qv = queries + (size_t)q * dim;
    const int32_t* cq = cand + (size_t)q * FLT_CAND;
    for (int64_t v = v0 + tid; v < v1; v += 256) {
        const int64_t r = (int64_t)cq[v >> 7] * 128 + (v & 127);
        if (r >= n || !group_allowed(mask.bits, mask.group_of[r])) continue;
        const uint16_t* xr = rows16 + (size_t)r * dim;
        float s = 0.f;
        for (int d = 0; d < dim; d += 8) {
            const f16x8 h = __builtin_bit_cast(f16x8, *(const uint4*)(xr + d));
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf((float)h[e], qs[d + e], s);
        }
        if (s >= thr) {
            const float dd = 1.0f - exact_dot_chain_pf(rows + (size_t)r * dim, qv, dim);
            const int pos = atomicAdd(list_n + q, 1);
            if (pos < FLT_LIST) list[(size_t)q * FLT_LIST + pos] = dist_key(dd, tie_of(tie, r));
        }
    }
}

// the k smallest listed keys (k rounds of "smallest key above the previous one"); too many or too few listed rows: exact redo
__global__ __launch_bounds__(256)
void filter_stream_finalize_kernel(const uint64_t* __restrict__ list, const int32_t* __restrict__ list_n, int k, int64_t m,
                                   int32_t* __restrict__ flags, int32_t* __restrict__ ids, float* __restrict__ out_dist, const TieOrder tie) {
    __shared__ uint64_t red[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (flags[q] != 0) return;
    const int c = list_n[q];
    if (c > FLT_LIST || (int64_t)c < min((int64_t)k, m)) {
        __syncthreads();
        if (tid == 0) flags[q] = 2;
        return;
    }
    const uint64_t* p = list + (size_t)q * FLT_LIST;
    uint64_t prev = 0;
    for (int j = 0; j < k; ++j) {
        uint64_t best = ~0ull;
        for (int i = tid; i < c; i += 256) {
            const uint64_t key = p[i];
            if ((j == 0 || key > prev) && key < best) best = key;
        }
        best = block_min_u64(best, red, tid);
        const int64_t o = (int64_t)q * k + j;
        if (tid == 0) {
            if (best == ~0ull) { ids[o] = -1; out_dist[o] = __builtin_inff(); }
            else { ids[o] = tie_row(tie, (uint32_t)best); out_dist[o] = key_dist(best); }
        }
        prev = best;
        if (best == ~0ull) {
            for (int jj = j + 1 + tid; jj < k; jj += 256) { ids[(int64_t)q * k + jj] = -1; out_dist[(int64_t)q * k + jj] = __builtin_inff(); }
            break;
        }
    }
}

}  // namespace vq
