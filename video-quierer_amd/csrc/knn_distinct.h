// Distinct-moment search (vq_index_search_distinct): the k best rows of the plain search's exhaustive (distance, tie) list L
// such that two kept rows of one group lie at least min_gap positions apart — greedy over L (DESIGN.md §4 "Distinct moments").
//
//   plan_distinct               host only: the prefix depth D, the producer of the prefix, the redo's slices
//   distinct_prefix_kernel      one wave per query walks the D sorted entries of the plain search, tests each against the kept
//                               (group, position) pairs in LDS, writes the k results and files the query for the redo when
//                               fewer than k rows were kept and L goes on behind the prefix
//   distinct_dist_kernel        exact_dist_kernel (the same fixed-order fp64 chain) for the filed queries only
//   distinct_group_walk_kernel  one wave per (filed query, group): greedy inside the group over its CSR row list; every row of
//                               the group that is not kept gets +inf in the distance buffer
//   (select_small_kernel / select_chunk_kernel + merge_topk_kernel then take the k smallest)
//   distinct_scatter_kernel     the selection's lists -> the filed queries' result slots (+inf = no result: id -1)
//
// Two facts make both paths exact.  PREFIX: a row's fate depends only on rows before it in L, so greedy over the first D
// entries keeps exactly the kept rows among them; k kept rows, or D = the index size, is the whole answer.  PER GROUP:
// conflicts never cross groups, so a group's kept rows follow from that group's rows alone, and kept rows behind a group's k-th
// cannot be among the k best overall.
//
// Every redo workgroup reads the filed count first and leaves at once when its slot is not filed; the number of launches
// depends on the shapes only.  Stream order is the only synchronisation between the launches.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"

#include <algorithm>

namespace vq {

constexpr int DST_MAX_DEPTH = 1024;          // prefix entries a wave holds in LDS = the exact selection's k limit
constexpr int DST_FP16_MAX_K = 100;          // the fp16 search's k limit (RV_K_MAX)
constexpr int DST_MIN_DEPTH = 64;
constexpr int DST_DEPTH_PER_K = 4;
constexpr int64_t DST_FP16_MIN_ROWS = 16384; // mode 0 takes the fp16 scan from here on (FP16_AUTO_MIN_ROWS)
constexpr int64_t DST_DIST_BUDGET = (int64_t)128 << 20;      // fp32 distances per redo slice: 512 MiB, the exact path's allowance
constexpr int DST_DIST_GRID = 2048;          // row-tile workgroups of distinct_dist_kernel (strided over the tiles)
// device counters (unsigned long long): queries proven on the prefix, prefix entries walked, queries filed for the redo
constexpr int DST_PROVEN = 0, DST_WALKED = 1, DST_FILED = 2;

struct DistinctPlan {
    int64_t depth;       // D: prefix entries fetched per query
    int producer;        // 0: exact distances + selection, 1: fp16 scan with proof
    int64_t slice_q;     // filed queries per redo slice
    int slices;          // redo slices queued (0: no query can be filed)
};

// The depth rule (include/vq_amd.h states it): D = max(64, 4 k), capped by the index size and by the producer's k limit;
// k alone when nothing can be suppressed before the k-th kept row (min_gap = 0, k = 1).  depth_override > 0 (tests) replaces
// the rule and is capped the same way.
inline DistinctPlan plan_distinct(int64_t n, int nq, int k, int64_t min_gap, int mode, int64_t depth_override) {
    DistinctPlan p;
    p.producer = (mode == 2 || (mode == 0 && n >= DST_FP16_MIN_ROWS)) ? 1 : 0;
    const int64_t limit = std::min<int64_t>(n, p.producer ? DST_FP16_MAX_K : DST_MAX_DEPTH);
    int64_t d = (min_gap == 0 || k == 1) ? k : std::max<int64_t>(DST_MIN_DEPTH, (int64_t)DST_DEPTH_PER_K * k);
    if (depth_override > 0) d = depth_override;
    p.depth = std::max<int64_t>(1, std::min(d, limit));
    const int64_t ld = round_up(n, 64);
    p.slice_q = std::max<int64_t>(1, std::min<int64_t>(nq, DST_DIST_BUDGET / ld));
    // a query is filed only when its prefix keeps fewer than k rows and L goes on behind it
    const bool can_file = p.depth < n && !(min_gap == 0 && p.depth >= k);
    p.slices = can_file ? (int)((nq + p.slice_q - 1) / p.slice_q) : 0;
    return p;
}

#ifdef __HIPCC__

__device__ __forceinline__ bool within_gap(int32_t a, int32_t b, int64_t gap) {
    const int64_t d = (int64_t)a - (int64_t)b;           // 64-bit: positions near +-2^31 do not wrap
    return (d < 0 ? -d : d) < gap;
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(v, o);
        v = other < v ? other : v;
    }
    return v;
}

// One wave per query.  pre_ids / pre_dist [nq][D]: the plain search's answer at depth D (sorted; -1 ends a list).
__global__ __launch_bounds__(64)
void distinct_prefix_kernel(const int32_t* __restrict__ pre_ids, const float* __restrict__ pre_dist, int D, int64_t n, int k, int64_t gap,
                            const int32_t* __restrict__ group_of, const int32_t* __restrict__ pos_of,
                            int32_t* __restrict__ ids, float* __restrict__ dist, int32_t* __restrict__ slots,
                            unsigned long long* __restrict__ counters) {
    __shared__ int32_t eg[DST_MAX_DEPTH], ep[DST_MAX_DEPTH];      // the entries' group and position
    __shared__ int32_t kg[DST_MAX_DEPTH], kp[DST_MAX_DEPTH];      // the kept rows'
    const int q = blockIdx.x, lane = threadIdx.x;
    const int32_t* pi = pre_ids + (int64_t)q * D;
    const float* pd = pre_dist + (int64_t)q * D;
    int32_t* oi = ids + (int64_t)q * k;
    float* od = dist + (int64_t)q * k;
    for (int i = lane; i < D; i += 64) {
        const int32_t r = pi[i];
        const bool ok = r >= 0 && r < n;
        eg[i] = ok ? group_of[r] : -1;
        ep[i] = ok ? pos_of[r] : 0;
    }
    __syncthreads();
    int c = 0, i = 0;
    bool ended = D >= n;                                          // the prefix is all of L
    for (; i < D && c < k; ++i) {
        const int32_t g = eg[i], p = ep[i];                       // LDS broadcasts: wave-uniform
        if (g < 0) { ended = true; break; }
        bool hit = false;
        for (int j = lane; j < c; j += 64) hit |= kg[j] == g && within_gap(p, kp[j], gap);
        if (__ballot(hit) == 0ull) {
            if (lane == 0) { kg[c] = g; kp[c] = p; oi[c] = pi[i]; od[c] = pd[i]; }
            ++c;
            __syncthreads();                                      // (one wave: orders lane 0's stores before the next test)
        }
    }
    for (int j = c + lane; j < k; j += 64) { oi[j] = -1; od[j] = __builtin_inff(); }
    if (lane == 0) {
        atomicAdd(counters + DST_WALKED, (unsigned long long)i);
        if (c < k && !ended) slots[atomicAdd(counters + DST_FILED, 1ull)] = q;
        else atomicAdd(counters + DST_PROVEN, 1ull);
    }
}

// exact_dist_kernel for the filed queries slot_base .. slot_base + slot_cap: the same tile, the same index-order fp64 chain.
// dist [slot_cap][ld], row s = filed slot slot_base + s.  Grid (row tiles, capped at DST_DIST_GRID and strided; slots / 32).
__global__ __launch_bounds__(256)
void distinct_dist_kernel(const float* __restrict__ rows, int64_t n, int dim, const float* __restrict__ queries,
                          const int32_t* __restrict__ slots, const unsigned long long* __restrict__ counters, int slot_base, int slot_cap,
                          float* __restrict__ dist, int64_t ld) {
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int q0 = blockIdx.y * 32;
    if (q0 >= count) return;
    __shared__ float xs[64][65];
    __shared__ double qs[32][64];
    __shared__ int32_t qn[32];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    if (tid < 32) qn[tid] = q0 + tid < count ? slots[slot_base + q0 + tid] : -1;
    __syncthreads();
    for (int64_t row0 = (int64_t)blockIdx.x * 64; row0 < n; row0 += (int64_t)gridDim.x * 64) {       // (a capped grid: few workgroups to leave)
        double acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0;
        for (int d0 = 0; d0 < dim; d0 += 64) {
            for (int i = tid; i < 64 * 64; i += 256) {
                const int rr = i >> 6, cc = i & 63;
                const int64_t gr = row0 + rr;
                xs[rr][cc] = (gr < n && d0 + cc < dim) ? rows[gr * dim + d0 + cc] : 0.f;
            }
            for (int i = tid; i < 32 * 64; i += 256) {
                const int qq = i >> 6, cc = i & 63;
                qs[qq][cc] = (qn[qq] >= 0 && d0 + cc < dim) ? (double)queries[(int64_t)qn[qq] * dim + d0 + cc] : 0.0;
            }
            __syncthreads();
#pragma unroll 8
            for (int c = 0; c < 64; ++c) {
                const double xv = (double)xs[r][c];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += xv * qs[g * 8 + j][c];   // product exact in fp64
            }
            __syncthreads();
        }
        const int64_t gr = row0 + r;
        if (gr < n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int s = q0 + g * 8 + j;
                if (s < count) dist[(int64_t)s * ld + gr] = 1.0f - (float)acc[j];
            }
        }
    }
}

// Grid (group blocks, slot_cap), four waves per workgroup, one wave per group at a time (groups strided over the grid): the
// wave takes the group's smallest live key (distance, tie) — live = finite and above the previous kept key — and, in the
// same sweep, gives +inf to the live rows within the gap of the row kept last.  A row still live has therefore been tested
// against every kept row.  After the k-th kept row the rest of the group gets +inf.  A lane only ever touches the rows of
// its own stride, so the sweeps need no barrier.
__global__ __launch_bounds__(256)
void distinct_group_walk_kernel(float* __restrict__ dist, int64_t ld, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                                int G, const int32_t* __restrict__ pos_of, const TieOrder tie, int k, int64_t gap,
                                const unsigned long long* __restrict__ counters, int slot_base, int slot_cap) {
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int s = blockIdx.y;
    if (s >= count) return;
    float* d = dist + (int64_t)s * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inf = __builtin_inff();
    for (int g = blockIdx.x * 4 + wave; g < G; g += gridDim.x * 4) {
        const int b = goff[g], e = goff[g + 1];
        if (e - b < 2) continue;                                  // a singleton is kept as it is
        uint64_t prev = 0;
        int32_t lastp = 0;
        int kept = 0;
        for (;;) {
            uint64_t best = ~0ull;
            for (int i = b + lane; i < e; i += 64) {
                const int32_t r = grows[i];
                const float v = d[r];
                if (v == inf) continue;
                const uint64_t key = dist_key(v, tie_of(tie, r));
                if (kept && key <= prev) continue;                // kept earlier
                if (kept == k || (kept && within_gap(pos_of[r], lastp, gap))) { d[r] = inf; continue; }
                best = key < best ? key : best;
            }
            if (kept == k) break;
            best = wave_min_u64(best);
            if (best == ~0ull) break;                             // group exhausted
            prev = best;
            lastp = pos_of[tie_row(tie, (uint32_t)best)];
            ++kept;
        }
    }
}

// sel_ids / sel_dist [slot_cap][k] (the selection over the walked distances) -> the filed queries' result slots
__global__ __launch_bounds__(256)
void distinct_scatter_kernel(const int32_t* __restrict__ sel_ids, const float* __restrict__ sel_dist, int k,
                             const int32_t* __restrict__ slots, const unsigned long long* __restrict__ counters, int slot_base, int slot_cap,
                             int32_t* __restrict__ ids, float* __restrict__ dist) {
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int s = blockIdx.x;
    if (s >= count) return;
    const int64_t q = slots[slot_base + s];
    for (int j = threadIdx.x; j < k; j += 256) {
        const float v = sel_dist[(int64_t)s * k + j];
        ids[q * k + j] = v == __builtin_inff() ? -1 : sel_ids[(int64_t)s * k + j];
        dist[q * k + j] = v;
    }
}

#endif  // __HIPCC__

}  // namespace vq
