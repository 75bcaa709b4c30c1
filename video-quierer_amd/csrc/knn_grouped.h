// Grouped exact top-k: "the k best VIDEOS, one best frame each" (vq_index_search_grouped).
//
// Every row carries a group label (vq_index_set_groups).  Per query, a group's best row is its row with the smallest
// (distance, tie rank) key — distance = fp32(1 - fp32(dot)) by the fixed-order fp64 chain, tie = the id rank or the row
// (TieOrder, vq_common.h) — and the answer is the first k groups by that key.  It equals walking the plain search's
// exhaustive (distance, id) list and keeping the first row of every group not seen yet.
//
// Exact path (mode 1, and the redo of queries the fp16 proof does not cover):
//   exact distances of the plain path (knn_kernels.h) -> group_block_topk_kernel<true>: workgroup = (256 groups, query), the
//   group minimum of the 64-bit key over the group's rows (by-group CSR list), the block's k smallest group keys ->
//   group_merge_kernel: the query's k smallest over the blocks.  The redo of a flagged query computes the distances inside
//   group_block_topk_kernel<false> instead of reading them (no [nq][n] buffer).
//
// fp16 path (mode 2), three passes:
//   1. scan3_group_max_kernel: the operand streaming of scan3_f16_top2_kernel (knn_scan_small.h: one wave = one stream of
//      128 rows straight into v_mfma_f32_16x16x32_f16 operands, 16 queries in registers, no LDS) with a group-max epilogue:
//      a stream whose 128 rows share one label (precomputed) max-reduces its 32 scores per lane and the four lanes of a query,
//      then issues ONE atomicMax per (stream, query); a mixed stream folds runs of equal labels lane by lane and issues one
//      atomicMax per run.  gbest[q][group] holds the order-preserving uint32 key of the group's largest fp16 score.
//   2. group_threshold_kernel: one workgroup per query; T = the k-th largest gbest by an 8-bit radix select (4 passes over
//      the uint32 keys, any number of groups); candidates = the groups with gbest >= T - 2E (every group when k >= groups),
//      their row counts prefix-summed for pass 3.  E = scan_eps_unit(dim) * max |row| * |q| (knn_scan_f16.h).
//   3. group_rescore_kernel (row slices of the candidates' rows, many workgroups per query): recompute each row's fp16
//      score (fp32 accumulation of exact fp16 products: within E as well), re-score exactly the rows at >= T - 2E and fold
//      them into the candidate's best key (global 64-bit atomicMin); group_finalize_kernel orders the candidates and writes
//      the top k.
//   Proof: the k groups with gbest >= T each hold a row whose exact score is >= T - E, so the k-th best group's exact score
//   s* is >= T - E.  A winning group's best row has exact score >= s* (up to the fp32 rounding of 1 - s, covered by a slack
//   of 2^-18), so its pass-1 score (and its group's gbest) and its recomputed score are >= T - 2E - slack: the group is a
//   candidate and that row is re-scored.  A candidate that is not a winner gets a key >= its true key, which is beyond the
//   k-th.  Comparisons are inclusive.  A query outside 0.25 <= |q|^2 <= 4 (or not finite), with more than GRP_CAND_MAX
//   candidate groups, or with fewer than min(k, groups) re-scored groups is flagged and redone by the exact path on the
//   device; nothing is truncated.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"

namespace vq {

constexpr int GRP_BLOCK = 256;           // groups per workgroup of group_block_topk_kernel
constexpr int GRP_CAND_MAX = 4096;       // candidate groups per query on the fp16 path (more: exact redo)
constexpr int GRP_RESCORE_SPLITS = 32;   // workgroups per query in pass 3
constexpr float GRP_SLACK = 1.0f / 262144;   // 2^-18: fp32 rounding of 1 - s and of the threshold arithmetic

// order-preserving fp32 score <-> uint32 (0 is below every real score: "no row seen")
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float key_score(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ void write_group_result(uint64_t key, size_t o, const int32_t* __restrict__ group_of, int32_t* __restrict__ groups,
                                                   int32_t* __restrict__ rows_out, float* __restrict__ dist, const TieOrder tie) {
    if (key == ~0ull) { groups[o] = -1; rows_out[o] = -1; dist[o] = __builtin_inff(); return; }
    const int32_t r = tie_row(tie, (uint32_t)key);
    groups[o] = group_of[r]; rows_out[o] = r; dist[o] = key_dist(key);
}

// ---- exact path: per (block of GRP_BLOCK groups, query) the group minima of the (distance, tie) key and the block's k_local
// smallest of them.  lpg lanes (1, 4, 16 or 64, from the mean group size) share a group and stride its rows; the row's
// distance is read from dist [nq][ld] (FROM_DIST) or computed by the fp64 chain.  flags != null: only queries whose flag is 2
// (the fp16 path's exact redo) do anything.  Filtered search (knn_filter.h): MASK skips the groups the mask disallows (they
// never reach the lists); POS walks a row LIST instead of the CSR row list — goff = the allowed groups' list offsets, the
// distance and the tie word of list position i are dist[q][i] and tie.rank[i] (no grows).  Both false: the unfiltered kernel. ----
template <bool FROM_DIST, bool MASK = false, bool POS = false>
__global__ __launch_bounds__(256)
void group_block_topk_kernel(const float* __restrict__ dist, int64_t ld, const float* __restrict__ rows, int dim,
                             const float* __restrict__ queries, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                             int n_groups, int lpg, int k_local, int nblocks, uint64_t* __restrict__ partial /*[nq][nblocks][k_local]*/,
                             const int32_t* __restrict__ flags, const TieOrder tie, const uint32_t* __restrict__ allow = nullptr) {
    static_assert(!POS || FROM_DIST, "a row list is walked over precomputed distances");
    __shared__ uint64_t gk[GRP_BLOCK];
    const int q = blockIdx.y, tid = threadIdx.x;
    if (flags && flags[q] != 2) return;                       // block-uniform
    const int g0 = blockIdx.x * GRP_BLOCK;
    const int sub = tid / lpg, ls = tid - sub * lpg, nsub = 256 / lpg;
    const float* qv = queries + (size_t)q * dim;
    for (int gl = sub; gl < GRP_BLOCK; gl += nsub) {          // lpg iterations for every thread: the shuffles below stay uniform
        const int g = g0 + gl;
        uint64_t best = ~0ull;
        bool live = g < n_groups;
        if constexpr (MASK) live = live && group_allowed(allow, g);
        if (live) {
            const int e = goff[g + 1];
            for (int i = goff[g] + ls; i < e; i += lpg) {
                const int r = POS ? i : grows[i];
                float d;
                if constexpr (FROM_DIST) d = dist[(int64_t)q * ld + r];
                else d = exact_row_dist(rows + (size_t)r * dim, qv, dim);
                const uint64_t key = dist_key(d, tie_of(tie, r));
                best = key < best ? key : best;
            }
        }
        for (int o = lpg >> 1; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor(best, o, lpg);
            best = other < best ? other : best;
        }
        if (ls == 0) gk[gl] = best;
    }
    __syncthreads();
    // rank by counting: group keys are distinct (their tie words name different rows); empty slots are ~0
    const uint64_t mine = gk[tid];
    int valid = 0, rank = 0;
    for (int j = 0; j < GRP_BLOCK; ++j) { const uint64_t o = gk[j]; valid += o != ~0ull; rank += o < mine; }
    uint64_t* out = partial + ((int64_t)q * nblocks + blockIdx.x) * k_local;
    if (mine != ~0ull && rank < k_local) out[rank] = mine;
    for (int j = valid + tid; j < k_local; j += 256) out[j] = ~0ull;
}

// ---- the query's k smallest group keys over its blocks' lists -> (group, row, distance); k rounds of "smallest key above the
// previous one" as merge_topk_kernel ----
__global__ __launch_bounds__(256)
void group_merge_kernel(const uint64_t* __restrict__ partial, int total /* nblocks * k_local */, int k, const int32_t* __restrict__ group_of,
                        int32_t* __restrict__ groups, int32_t* __restrict__ rows_out, float* __restrict__ dist,
                        const int32_t* __restrict__ flags, const TieOrder tie) {
    __shared__ uint64_t red[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    if (flags && flags[q] != 2) return;
    const uint64_t* p = partial + (int64_t)q * total;
    uint64_t prev = 0;
    for (int j = 0; j < k; ++j) {
        uint64_t best = ~0ull;
        for (int i = tid; i < total; i += 256) {
            const uint64_t key = p[i];
            if ((j == 0 || key > prev) && key < best) best = key;
        }
        best = block_min_u64(best, red, tid);
        if (tid == 0) write_group_result(best, (size_t)q * k + j, group_of, groups, rows_out, dist, tie);
        prev = best;
        if (best == ~0ull) {                                  // block-uniform
            for (int jj = j + 1 + tid; jj < k; jj += 256) write_group_result(~0ull, (size_t)q * k + jj, group_of, groups, rows_out, dist, tie);
            break;
        }
    }
}

// ---- fp16 pass 1: group-max scan.  Operand streaming and MFMA loop of scan3_f16_top2_kernel<NKS, 1>; Q16 [q_pad][dim] fp16,
// 16 queries per blockIdx.y.  group_of is padded with -1 to whole streams; stream_group[s] = the label all 128 rows of stream s
// share, or -1. ----
// MASK (filtered search): a disallowed uniform stream is not read; in a mixed stream disallowed rows are skipped like rows
// past the end, so a disallowed group's gbest stays 0 ("no row seen").  MASK = false compiles to the unfiltered kernel.
template <int NKS, bool MASK = false>
__global__ __launch_bounds__(256, 2)
void scan3_group_max_kernel(const uint16_t* __restrict__ Q16, const uint16_t* __restrict__ X16, int64_t streams,
                            const int32_t* __restrict__ group_of, const int32_t* __restrict__ stream_group, int nq_real, int n_groups,
                            uint32_t* __restrict__ gbest /*[nq][n_groups]*/, const uint32_t* __restrict__ allow = nullptr) {
    typedef mfma_op<true> op;
    typedef op::frag frag;
    constexpr int DIM = NKS * 32;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stream = (int64_t)blockIdx.x * 4 + wave;
    if (stream >= streams) return;                         // wave-uniform; no barriers below
    const int r16 = lane & 15, g = lane >> 4;
    const int q = blockIdx.y * 16 + r16;
    const bool qlive = q < nq_real;

    frag qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const frag*)(Q16 + (size_t)q * DIM + ks * 32 + g * 8);
    const uint16_t* xrow = X16 + ((size_t)stream * 128 + r16) * DIM + g * 8;
    const int sg = __builtin_amdgcn_readfirstlane(stream_group[stream]);
    if constexpr (MASK)
        if (sg >= 0 && !group_allowed(allow, sg)) return;       // wave-uniform: a disallowed video's stream is not read
    frag xf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) xf[ks] = *(const frag*)(xrow + ks * 32);

    uint32_t* gb = gbest + (size_t)(qlive ? q : 0) * n_groups;
    const int32_t* lab = group_of + stream * 128 + 4 * g;
    float m = -__builtin_inff();
    int cur = -1;                                          // label of the lane's open run (a uniform stream has one run)
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
        int4 l4 = {sg, sg, sg, sg};
        if (sg < 0) l4 = *(const int4*)(lab + rb * 16);    // rows rb*16 + 4g .. +3 (16-byte aligned)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            acc = op::run(xf[ks], qf[ks], acc);
            if (rb + 1 < 8) {
                xf[ks] = *(const frag*)(xrow + (size_t)(rb + 1) * 16 * DIM + ks * 32);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const int lr[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int L = lr[r];
            if constexpr (MASK)
                if (sg < 0 && !group_allowed(allow, L)) L = -1;   // a disallowed row of a mixed stream: as a row past the end
            if (L < 0) continue;                           // rows past the end of the index
            if (L != cur) {                                // a run ends: one atomic for it (never in a uniform stream)
                if (cur >= 0 && qlive) atomicMax(gb + cur, score_key(m));
                cur = L; m = acc[r];
            } else {
                m = fmaxf(m, acc[r]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (sg >= 0) {
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        if (g == 0 && qlive) atomicMax(gb + sg, score_key(m));
    } else if (cur >= 0 && qlive) {
        atomicMax(gb + cur, score_key(m));
    }
}

// ---- fp16 pass 2: threshold and candidate groups, one workgroup per query ----
__global__ __launch_bounds__(256)
void group_threshold_kernel(const uint32_t* __restrict__ gbest, int n_groups, int k, const float* __restrict__ queries, int dim,
                            float eps_rows, const int32_t* __restrict__ goff, int32_t* __restrict__ cand /*[nq][CAND]*/,
                            int32_t* __restrict__ cand_pref /*[nq][CAND + 1]*/, int32_t* __restrict__ cand_n, float* __restrict__ cand_thr,
                            uint64_t* __restrict__ best /*[nq][CAND]*/, int32_t* __restrict__ flags) {
    __shared__ uint32_t hist[256];
    __shared__ int32_t list[GRP_CAND_MAX];
    __shared__ int part[256];
    __shared__ float red[4];
    __shared__ uint32_t prefix_s;
    __shared__ int kr_s, cnt_s;
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint32_t* gb = gbest + (size_t)q * n_groups;
    const float* qv = queries + (size_t)q * dim;
    float s2 = 0.f;
    for (int i = tid; i < dim; i += 256) s2 += qv[i] * qv[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    if ((tid & 63) == 0) red[tid >> 6] = s2;
    if (tid == 0) cnt_s = 0;
    __syncthreads();
    const float q2 = (red[0] + red[1]) + (red[2] + red[3]);
    if (!(q2 >= SCAN_Q2_MIN && q2 <= SCAN_Q2_MAX)) {        // outside what the fp16 bound covers (NaN included): exact redo
        if (tid == 0) { flags[q] = 2; cand_n[q] = 0; }
        return;
    }
    const float E = eps_rows * sqrtf(q2);
    float thr = -__builtin_inff();
    if (k < n_groups) {                                     // T = the k-th largest key: radix select, 8 bits at a time
        uint32_t prefix = 0, mask = 0;
        int kr = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n_groups; i += 256) {
                const uint32_t v = gb[i];
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
        thr = (key_score(prefix) - 2.0f * E) - GRP_SLACK;
    }
    for (int i = tid; i < n_groups; i += 256)
        if (k >= n_groups || key_score(gb[i]) >= thr) {
            const int pos = atomicAdd(&cnt_s, 1);
            if (pos < GRP_CAND_MAX) list[pos] = i;
        }
    __syncthreads();
    const int c = cnt_s;
    if (c > GRP_CAND_MAX) {                                 // more candidate groups than the lists hold: exact redo
        if (tid == 0) { flags[q] = 2; cand_n[q] = 0; }
        return;
    }
    // row counts of the candidates, prefix-summed: thread t owns entries [t*per, (t+1)*per)
    const int per = (c + 255) / 256, j0 = min(c, tid * per), j1 = min(c, j0 + per);
    int sum = 0;
    for (int j = j0; j < j1; ++j) sum += goff[list[j] + 1] - goff[list[j]];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
        cand_pref[(size_t)q * (GRP_CAND_MAX + 1) + c] = run;
        cand_n[q] = c; cand_thr[q] = thr; flags[q] = 0;
    }
    __syncthreads();
    int run = part[tid];
    for (int j = j0; j < j1; ++j) {
        const int gi = list[j];
        cand[(size_t)q * GRP_CAND_MAX + j] = gi;
        cand_pref[(size_t)q * (GRP_CAND_MAX + 1) + j] = run;
        best[(size_t)q * GRP_CAND_MAX + j] = ~0ull;
        run += goff[gi + 1] - goff[gi];
    }
}

// ---- fp16 pass 3a: the candidates' rows, GRP_RESCORE_SPLITS workgroups per query ----
__global__ __launch_bounds__(256)
void group_rescore_kernel(const uint16_t* __restrict__ Q16, const float* __restrict__ queries, const float* __restrict__ rows,
                          const uint16_t* __restrict__ rows16, int dim, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                          const int32_t* __restrict__ cand, const int32_t* __restrict__ cand_pref, const int32_t* __restrict__ cand_n,
                          const float* __restrict__ cand_thr, const int32_t* __restrict__ flags, uint64_t* __restrict__ best,
                          unsigned long long* __restrict__ counters, const TieOrder tie) {
    __shared__ int pref[GRP_CAND_MAX + 1];
    __shared__ float qs[768];
    __shared__ int cnt_s;
    const int q = blockIdx.y, tid = threadIdx.x;
    if (flags[q] != 0) return;                              // block-uniform
    const int c = cand_n[q];
    if (c == 0) return;
    for (int i = tid; i <= c; i += 256) pref[i] = cand_pref[(size_t)q * (GRP_CAND_MAX + 1) + i];
    for (int i = tid; i < dim; i += 256) qs[i] = (float)__builtin_bit_cast(_Float16, Q16[(size_t)q * dim + i]);
    if (tid == 0) cnt_s = 0;
    __syncthreads();
    const int64_t total = pref[c];
    const int64_t v0 = total * blockIdx.x / gridDim.x, v1 = total * (blockIdx.x + 1) / gridDim.x;
    const float thr = cand_thr[q];
    const float* qv = queries + (size_t)q * dim;
    const int32_t* cq = cand + (size_t)q * GRP_CAND_MAX;
    uint64_t* bq = best + (size_t)q * GRP_CAND_MAX;
    int mine = 0;
    for (int64_t v = v0 + tid; v < v1; v += 256) {
        int lo = 0, hi = c;                                 // pref[lo] <= v < pref[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pref[mid] <= v) lo = mid; else hi = mid; }
        const int gi = cq[lo];
        const int r = grows[goff[gi] + (int)(v - pref[lo])];
        // the row's fp16 score, fp32 accumulation of exact fp16 products: within E of the exact score like pass 1's
        const uint16_t* xr = rows16 + (size_t)r * dim;
        float s = 0.f;
        for (int d = 0; d < dim; d += 8) {
            const f16x8 h = __builtin_bit_cast(f16x8, *(const uint4*)(xr + d));
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf((float)h[e], qs[d + e], s);
        }
        if (s >= thr) {
            const float dd = 1.0f - exact_dot_chain_pf(rows + (size_t)r * dim, qv, dim);
            atomicMin((unsigned long long*)(bq + lo), (unsigned long long)dist_key(dd, tie_of(tie, r)));
            ++mine;
        }
    }
    if (mine) atomicAdd(&cnt_s, mine);
    __syncthreads();
    if (tid == 0 && cnt_s) atomicAdd(counters + 1, (unsigned long long)cnt_s);
}

// ---- fp16 pass 3b: order the candidates' best keys, write the top k; too few re-scored groups -> exact redo ----
__global__ __launch_bounds__(256)
void group_finalize_kernel(const int32_t* __restrict__ cand_n, const uint64_t* __restrict__ best, int k, int n_groups,
                           const int32_t* __restrict__ group_of, int32_t* __restrict__ flags, int32_t* __restrict__ groups,
                           int32_t* __restrict__ rows_out, float* __restrict__ dist, unsigned long long* __restrict__ counters,
                           const TieOrder tie) {
    __shared__ uint64_t red[4];
    __shared__ int fin_s;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (flags[q] != 0) {
        if (tid == 0) atomicAdd(counters + 2, 1ull);
        return;
    }
    const int c = cand_n[q];
    const uint64_t* b = best + (size_t)q * GRP_CAND_MAX;
    if (tid == 0) fin_s = 0;
    __syncthreads();
    int f = 0;
    for (int i = tid; i < c; i += 256) f += b[i] != ~0ull;
    if (f) atomicAdd(&fin_s, f);
    __syncthreads();
    if (fin_s < min(k, n_groups)) {                         // the proof did not close: exact redo (not expected)
        if (tid == 0) { flags[q] = 2; atomicAdd(counters + 2, 1ull); }
        return;
    }
    if (tid == 0) atomicAdd(counters + 0, 1ull);
    uint64_t prev = 0;
    for (int j = 0; j < k; ++j) {
        uint64_t bk = ~0ull;
        for (int i = tid; i < c; i += 256) {
            const uint64_t key = b[i];
            if ((j == 0 || key > prev) && key < bk) bk = key;
        }
        bk = block_min_u64(bk, red, tid);
        if (tid == 0) write_group_result(bk, (size_t)q * k + j, group_of, groups, rows_out, dist, tie);
        prev = bk;
        if (bk == ~0ull) {
            for (int jj = j + 1 + tid; jj < k; jj += 256) write_group_result(~0ull, (size_t)q * k + jj, group_of, groups, rows_out, dist, tie);
            break;
        }
    }
}

}  // namespace vq
