// Keyframe summary (vq_index_summarize_groups): the k most representative rows of each listed group (video) by an iterative
// farthest-point (greedy k-centre) pass per group (include/vq_amd.h has the definition; DESIGN.md §4 "Keyframe summary").
//
//   plan_summary              host only: the LDS form's row limit and bytes, whether a wide form runs, the launches queued
//   sum_lds_kernel            one workgroup per listed group of at most lds_rows rows: mean direction, seed, the k steps, the
//                             members, all in one launch; per-row state (near key, owner, row, tie) and the centre in LDS
//   sum_wide_blocksum_kernel  longer groups, one workgroup per 256-row block of a host-built block list: the mean's block sums
//   sum_wide_mean_kernel      one workgroup per long group: block sums -> c
//   sum_wide_update_kernel    per block: distances to the centre, the min-update, the block's maximum to its own slot
//                             (SEED: distances to c, the block's smallest (distance, tie))
//   sum_wide_pick_kernel      one workgroup per long group over its blocks' slots: radius[t], the stop rule, the next centre
//   sum_wide_members_kernel   one workgroup per long group: the members, the unused slots
//   sum_stats_kernel          the call's counters
//
// State per row: near as the order-preserving 32-bit key of the fp32 distance (the high word of dist_key) and the owner.  A
// chosen row's key is SUM_CHOSEN (0: the key of no number), so it never competes again.  The pick is the maximum of the packed
// 64-bit (near key, inverted tie): ties are distinct inside a group, so the packed words are, and thread order never decides.
// The seed is the same maximum over (inverted distance key, inverted tie).
//
// Exact: every distance is the fixed-order fp64 chain of the plain search (exact_dot_chain_pf / exact_dot_chain, here with the
// centre already widened to fp64 in LDS: the products are exact either way, so the bits are the same); the mean's sums run in
// the order the definition fixes (rows of a 256-row block in order, then the blocks in order).  No scratch memory, no global
// atomics; workgroup barriers are the only synchronisation inside a launch, stream order between launches.  The launches
// queued depend on the shapes only: a long group that has stopped sets a flag, and its later blocks return at once.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"

#include <algorithm>

namespace vq {

constexpr int SUM_MAX_K = 256;                                // keyframes per group
constexpr int SUM_LDS_ROWS = 4096;                            // longest group of the LDS form
constexpr int SUM_THREADS = 256;
constexpr int SUM_BLOCK = 256;                                // rows per block: of the mean (part of the definition) and of the wide form
constexpr int SUM_LDS_ROW_BYTES = 4 + 4 + 4 + 2;              // near key, row, tie, owner
constexpr int SUM_LDS_FIXED = 64 + SUM_MAX_K * 4;             // reduction words and the centre's row; the members' counters
constexpr uint32_t SUM_CHOSEN = 0u;                           // near key of a chosen row
constexpr uint32_t SUM_INF_KEY = 0xff800000u;                 // near key of +inf: before the first centre

struct SummaryPlan {
    int lds_rows;        // groups of at most this many rows take the LDS form
    int64_t lds_bytes;   // its dynamic LDS when the longest group it runs holds min(lds_rows, largest_group) rows
    int wide_form;       // 1: the largest group (so at least one) takes the wide form
    int launches;        // kernels queued by one call
};

// dynamic LDS of sum_lds_kernel for groups of at most `rows` rows: centre [dim] fp64 | fixed | per-row arrays
inline int64_t summary_lds_bytes(int64_t rows, int dim) {
    return (int64_t)dim * 8 + SUM_LDS_FIXED + round_up(std::max<int64_t>(rows, 1), 64) * SUM_LDS_ROW_BYTES;
}

// lds_rows_override > 0 (tests) lowers SUM_LDS_ROWS.
inline SummaryPlan plan_summary(int64_t largest_group, int dim, int k, int64_t lds_rows_override) {
    SummaryPlan p;
    p.lds_rows = (int)(lds_rows_override > 0 ? std::min<int64_t>(lds_rows_override, SUM_LDS_ROWS) : SUM_LDS_ROWS);
    p.lds_bytes = summary_lds_bytes(std::min<int64_t>(p.lds_rows, largest_group), dim);
    p.wide_form = largest_group > p.lds_rows ? 1 : 0;
    // the LDS form and the counters; wide: block sums, mean, seed (update + pick), k steps (update + pick), members
    p.launches = 2 + (p.wide_form ? 5 + 2 * k : 0);
    return p;
}

#ifdef __HIPCC__

__device__ __forceinline__ uint32_t sum_key(float d) { return (uint32_t)(dist_key(d, 0) >> 32); }
__device__ __forceinline__ float sum_key_dist(uint32_t key) { return key_dist((uint64_t)key << 32); }

// The chains of knn_scan_f16.h with the query already in fp64 (a centre staged in LDS once per step): the same additions in
// the same order, (double)q[i] done by whoever staged it.
__device__ __forceinline__ float exact_dot_chain_pf(const float* __restrict__ row, const double* __restrict__ q, int dim) {
    double acc = 0.0;
    for (int i = 0; i < dim; i += 32) {
        float4 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = *(const float4*)(row + i + 4 * u);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double* b = q + i + 4 * u;
            acc += (double)a[u].x * b[0];
            acc += (double)a[u].y * b[1];
            acc += (double)a[u].z * b[2];
            acc += (double)a[u].w * b[3];
        }
    }
    return (float)acc;
}
__device__ __forceinline__ float exact_dot_chain(const float* __restrict__ row, const double* __restrict__ q, int dim) {
    double acc = 0.0;
    for (int i = 0; i < dim; i += 4) {
        const float4 a = *(const float4*)(row + i);
        acc += (double)a.x * q[i];
        acc += (double)a.y * q[i + 1];
        acc += (double)a.z * q[i + 2];
        acc += (double)a.w * q[i + 3];
    }
    return (float)acc;
}
__device__ __forceinline__ float exact_row_dist(const float* __restrict__ row, const double* __restrict__ q, int dim) {
    return 1.0f - ((dim & 31) == 0 ? exact_dot_chain_pf(row, q, dim) : exact_dot_chain(row, q, dim));
}
__device__ __forceinline__ uint32_t sum_row_key(const float* rows, int dim, const double* cq, int r) {
    return sum_key(exact_row_dist(rows + (size_t)r * dim, cq, dim));
}

// the workgroup's largest v, in every thread (two barriers: red [4] may still be read from the round before)
__device__ __forceinline__ uint64_t sum_block_max(uint64_t v, uint64_t* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(v, o);
        v = other > v ? other : v;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    uint64_t b = red[0];
#pragma unroll
    for (int w = 1; w < SUM_THREADS / 64; ++w) b = red[w] > b ? red[w] : b;
    return b;
}

// B[c] = the fp64 sum over rows list[0 .. cnt) in order of (double)x[c]: eight independent loads ahead of the eight additions
__device__ __forceinline__ double sum_column(const float* __restrict__ rows, int dim, const int32_t* list, int cnt, int c) {
    double B = 0.0;
    int i = 0;
    for (; i + 8 <= cnt; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = rows[(size_t)list[i + u] * dim + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) B += (double)v[u];
    }
    for (; i < cnt; ++i) B += (double)rows[(size_t)list[i] * dim + c];
    return B;
}

// row r of the matrix -> cq [dim] as fp64 (dim % 4 == 0)
__device__ __forceinline__ void sum_stage_centre(const float* __restrict__ rows, int dim, int r, double* cq, int tid) {
    const float* x = rows + (size_t)r * dim;
    for (int c = tid * 4; c < dim; c += SUM_THREADS * 4) {
        const float4 v = *(const float4*)(x + c);
        cq[c] = (double)v.x; cq[c + 1] = (double)v.y; cq[c + 2] = (double)v.z; cq[c + 3] = (double)v.w;
    }
}

// unused slots kappa .. k - 1 of one entry; members [0, kappa) from the LDS counters
__device__ __forceinline__ void sum_finish(int32_t* ro, float* rad, int32_t* mo, const int* mem, int kappa, int k, int tid) {
    for (int j = tid; j < k; j += SUM_THREADS) {
        if (j >= kappa) { ro[j] = -1; rad[j] = __builtin_inff(); }
        if (mo) mo[j] = j < kappa ? mem[j] : 0;
    }
}

// ---- LDS form: grid = listed entries.  dynamic LDS: summary_lds_bytes(alloc_rows, dim) ----
__global__ __launch_bounds__(SUM_THREADS)
void sum_lds_kernel(const float* __restrict__ rows, int dim, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows, const TieOrder tie,
                    const int32_t* __restrict__ sel, int k, float max_radius, int lds_rows, int alloc_rows, int32_t* __restrict__ rows_out,
                    float* __restrict__ radius_out, int32_t* __restrict__ members_out, int32_t* __restrict__ kap) {
    extern __shared__ __attribute__((aligned(16))) char sum_smem[];
    const int tid = threadIdx.x, e = blockIdx.x;
    const int g = sel[e];
    const int b = goff[g], L = goff[g + 1] - b;
    if (L > lds_rows) return;                                   // the wide form's; whole workgroup leaves before any barrier
    int32_t* ro = rows_out + (size_t)e * k;
    float* rad = radius_out + (size_t)e * k;
    int32_t* mo = members_out ? members_out + (size_t)e * k : nullptr;
    double* cq = (double*)sum_smem;
    uint64_t* red = (uint64_t*)(cq + dim);
    int* cur = (int*)(red + 4);
    int* mem = (int*)((char*)red + 64);
    uint32_t* near = (uint32_t*)(mem + SUM_MAX_K);
    int32_t* row = (int32_t*)(near + alloc_rows);
    uint32_t* tiew = (uint32_t*)(row + alloc_rows);
    uint16_t* owner = (uint16_t*)(tiew + alloc_rows);
    if (L == 0) {                                               // a label that holds no row
        sum_finish(ro, rad, mo, mem, 0, k, tid);
        if (tid == 0) kap[e] = 0;
        return;
    }
    for (int i = tid; i < L; i += SUM_THREADS) {
        const int r = grows[b + i];
        row[i] = r; tiew[i] = tie_of(tie, r); near[i] = SUM_INF_KEY; owner[i] = 0;
    }
    __syncthreads();
    // 1. mean direction: a thread per component, the rows of a block in order, then the blocks in order
    for (int c = tid; c < dim; c += SUM_THREADS) {
        double S = 0.0;
        for (int i0 = 0; i0 < L; i0 += SUM_BLOCK) S += sum_column(rows, dim, row + i0, min(SUM_BLOCK, L - i0), c);
        cq[c] = (double)(float)S;
    }
    __syncthreads();
    // 2. seed: the smallest (distance to c, tie)
    uint64_t best = 0;
    int bi = -1;
    for (int i = tid; i < L; i += SUM_THREADS) {
        const uint64_t p = ((uint64_t)~sum_row_key(rows, dim, cq, row[i]) << 32) | (uint32_t)~tiew[i];
        if (bi < 0 || p > best) { best = p; bi = i; }
    }
    uint64_t gmax = sum_block_max(best, red, tid);
    if (bi >= 0 && best == gmax) { near[bi] = SUM_CHOSEN; ro[0] = row[bi]; *cur = row[bi]; }
    __syncthreads();
    // 3. - 5. centre s_t -> LDS; min-update of the rows not yet chosen; their largest (near, smallest tie) is radius[t] and s_{t+1}
    int t = 0;
    for (;;) {
        sum_stage_centre(rows, dim, *cur, cq, tid);
        __syncthreads();
        best = 0; bi = -1;
        for (int i = tid; i < L; i += SUM_THREADS) {
            uint32_t nk = near[i];
            if (nk == SUM_CHOSEN) continue;
            const uint32_t kd = sum_row_key(rows, dim, cq, row[i]);
            if (kd < nk) { nk = kd; near[i] = kd; owner[i] = (uint16_t)t; }
            const uint64_t p = ((uint64_t)nk << 32) | (uint32_t)~tiew[i];
            if (bi < 0 || p > best) { best = p; bi = i; }
        }
        gmax = sum_block_max(best, red, tid);
        const bool none = (gmax >> 32) == 0;
        const float radius = none ? 0.0f : sum_key_dist((uint32_t)(gmax >> 32));
        if (tid == 0) rad[t] = radius;
        if (t + 1 == k || none || radius <= max_radius) break;
        if (bi >= 0 && best == gmax) { near[bi] = SUM_CHOSEN; owner[bi] = (uint16_t)(t + 1); ro[t + 1] = row[bi]; *cur = row[bi]; }
        __syncthreads();
        ++t;
    }
    // 6. members: LDS counters
    const int kappa = t + 1;
    for (int j = tid; j < k; j += SUM_THREADS) mem[j] = 0;
    __syncthreads();
    for (int i = tid; i < L; i += SUM_THREADS) atomicAdd(&mem[owner[i]], 1);
    __syncthreads();
    sum_finish(ro, rad, mo, mem, kappa, k, tid);
    if (tid == 0) kap[e] = kappa;
}

// ---- wide form.  Host-built lists (vq_index.hip summarize_run): per long entry w its output slot, its group, its first block
// (boff [nw + 1]) and its first state row (soff [nw + 1]); per block its entry.  State near / owner [W], W the rows of all long
// entries; per block a slot bmax / bidx (the packed maximum and the group-local index of the row that attains it, -1: none);
// per entry cur (the centre's row), done, kappa. ----
struct SumWide {
    const int32_t* slot; const int32_t* group; const int32_t* boff; const int32_t* soff; const int32_t* blk_entry;
    uint32_t* near; int32_t* owner; uint64_t* bmax; int32_t* bidx; int32_t* cur; int32_t* done; int32_t* kappa;
    double* bsum /*[nb][dim]*/; double* cvec /*[nw][dim]*/;
};

// grid = blocks: the mean's block sums, and the state before the first centre
__global__ __launch_bounds__(SUM_THREADS)
void sum_wide_blocksum_kernel(const float* __restrict__ rows, int dim, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                              const SumWide w) {
    __shared__ int32_t list[SUM_BLOCK];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int e = w.blk_entry[blk], g = w.group[e];
    const int b = goff[g], L = goff[g + 1] - b;
    const int i0 = (blk - w.boff[e]) * SUM_BLOCK, cnt = min(SUM_BLOCK, L - i0);
    if (tid < cnt) {
        list[tid] = grows[b + i0 + tid];
        w.near[w.soff[e] + i0 + tid] = SUM_INF_KEY;
        w.owner[w.soff[e] + i0 + tid] = 0;
    }
    __syncthreads();
    for (int c = tid; c < dim; c += SUM_THREADS) w.bsum[(size_t)blk * dim + c] = sum_column(rows, dim, list, cnt, c);
}

// grid = long entries: S = B_0 + B_1 + .. in block order, c = (float)S, kept widened
__global__ __launch_bounds__(SUM_THREADS)
void sum_wide_mean_kernel(int dim, const SumWide w) {
    const int e = blockIdx.x;
    for (int c = threadIdx.x; c < dim; c += SUM_THREADS) {
        double S = 0.0;
        for (int blk = w.boff[e]; blk < w.boff[e + 1]; ++blk) S += w.bsum[(size_t)blk * dim + c];
        w.cvec[(size_t)e * dim + c] = (double)(float)S;
    }
}

// grid = blocks, dynamic LDS dim * 8 + 64.  SEED: the block's smallest (distance to c, tie).  Otherwise step t: the centre is
// row cur [e]; min-update; the block's largest (near, smallest tie) among the rows not yet chosen.
template <bool SEED>
__global__ __launch_bounds__(SUM_THREADS)
void sum_wide_update_kernel(const float* __restrict__ rows, int dim, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                            const TieOrder tie, const SumWide w, int t) {
    extern __shared__ __attribute__((aligned(16))) char sum_smem[];
    double* cq = (double*)sum_smem;
    uint64_t* red = (uint64_t*)(cq + dim);
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int e = w.blk_entry[blk];
    if (!SEED && w.done[e]) return;                             // the group has stopped (the flag is one word: workgroup-uniform)
    const int g = w.group[e];
    const int b = goff[g], L = goff[g + 1] - b;
    const int i = (blk - w.boff[e]) * SUM_BLOCK + tid;
    if (SEED) {
        for (int c = tid; c < dim; c += SUM_THREADS) cq[c] = w.cvec[(size_t)e * dim + c];
    } else {
        sum_stage_centre(rows, dim, w.cur[e], cq, tid);
    }
    __syncthreads();
    uint64_t p = 0;
    bool cand = false;
    if (i < L) {
        const int r = grows[b + i];
        const int64_t st = (int64_t)w.soff[e] + i;
        if (SEED) {
            p = ((uint64_t)~sum_row_key(rows, dim, cq, r) << 32) | (uint32_t)~tie_of(tie, r);
            cand = true;
        } else {
            uint32_t nk = w.near[st];
            if (nk != SUM_CHOSEN) {
                const uint32_t kd = sum_row_key(rows, dim, cq, r);
                if (kd < nk) { nk = kd; w.near[st] = kd; w.owner[st] = t; }
                p = ((uint64_t)nk << 32) | (uint32_t)~tie_of(tie, r);
                cand = true;
            }
        }
    }
    const uint64_t gmax = sum_block_max(cand ? p : 0, red, tid);
    const bool win = cand && p == gmax;
    if (win) { w.bmax[blk] = gmax; w.bidx[blk] = i; }
    if (!__syncthreads_or(win) && tid == 0) { w.bmax[blk] = 0; w.bidx[blk] = -1; }
}

// grid = long entries.  seed: s_0 from the blocks' slots.  Otherwise step t: radius [t], the stop rule, s_{t+1}.
__global__ __launch_bounds__(SUM_THREADS)
void sum_wide_pick_kernel(const int32_t* __restrict__ goff, const int32_t* __restrict__ grows, const SumWide w, int seed, int t, int k,
                          float max_radius, int32_t* __restrict__ rows_out, float* __restrict__ radius_out) {
    __shared__ uint64_t red[SUM_THREADS / 64];
    const int tid = threadIdx.x, e = blockIdx.x;
    if (!seed && w.done[e]) return;
    uint64_t best = 0;
    int bb = -1;
    for (int blk = w.boff[e] + tid; blk < w.boff[e + 1]; blk += SUM_THREADS) {
        if (w.bidx[blk] < 0) continue;
        const uint64_t p = w.bmax[blk];
        if (bb < 0 || p > best) { best = p; bb = blk; }
    }
    const uint64_t gmax = sum_block_max(best, red, tid);
    const bool win = bb >= 0 && best == gmax;
    const int b = goff[w.group[e]];
    int32_t* ro = rows_out + (size_t)w.slot[e] * k;
    if (seed) {
        if (win) {
            const int i = w.bidx[bb], r = grows[b + i];
            w.near[(int64_t)w.soff[e] + i] = SUM_CHOSEN;
            ro[0] = r; w.cur[e] = r; w.done[e] = 0;
        }
        return;
    }
    const bool none = (gmax >> 32) == 0;
    const float radius = none ? 0.0f : sum_key_dist((uint32_t)(gmax >> 32));
    const bool stop = t + 1 == k || none || radius <= max_radius;
    if (tid == 0) {
        radius_out[(size_t)w.slot[e] * k + t] = radius;
        if (stop) { w.done[e] = 1; w.kappa[e] = t + 1; }
    }
    if (!stop && win) {
        const int i = w.bidx[bb], r = grows[b + i];
        const int64_t st = (int64_t)w.soff[e] + i;
        w.near[st] = SUM_CHOSEN; w.owner[st] = t + 1;
        ro[t + 1] = r; w.cur[e] = r;
    }
}

// grid = long entries: members from the owners, the unused slots, the entry's keyframe count
__global__ __launch_bounds__(SUM_THREADS)
void sum_wide_members_kernel(const SumWide w, int k, int32_t* __restrict__ rows_out, float* __restrict__ radius_out,
                             int32_t* __restrict__ members_out, int32_t* __restrict__ kap) {
    __shared__ int mem[SUM_MAX_K];
    const int tid = threadIdx.x, e = blockIdx.x;
    const int64_t s0 = w.soff[e], s1 = w.soff[e + 1];
    for (int j = tid; j < k; j += SUM_THREADS) mem[j] = 0;
    __syncthreads();
    for (int64_t s = s0 + tid; s < s1; s += SUM_THREADS) atomicAdd(&mem[w.owner[s]], 1);
    __syncthreads();
    const size_t o = (size_t)w.slot[e] * k;
    sum_finish(rows_out + o, radius_out + o, members_out ? members_out + o : nullptr, mem, w.kappa[e], k, tid);
    if (tid == 0) kap[w.slot[e]] = w.kappa[e];
}

// ---- the call's counters: the two figures the host knows, and the keyframes written ----
__global__ __launch_bounds__(256)
void sum_stats_kernel(const int32_t* __restrict__ kap, int n_sel, unsigned long long lds_groups, unsigned long long wide_groups,
                      unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long red[4];
    const int tid = threadIdx.x;
    unsigned long long c = 0;
    for (int i = tid; i < n_sel; i += 256) c += (unsigned long long)kap[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        counters[0] = lds_groups;
        counters[1] = wide_groups;
        counters[2] = red[0] + red[1] + red[2] + red[3];
    }
}

#endif  // __HIPCC__

}  // namespace vq
