// Sequence search (vq_index_search_sequence): the k GROUPS (videos) that show the steps q_0 .. q_{m-1} IN ORDER — a chain of m
// rows of one group whose positions increase by min_gap .. max_gap from step to step, of the smallest summed distance
// (include/vq_amd.h has the definition; DESIGN.md §4 "Sequence search").
//
//   plan_sequence            host only: the step chunks, the LDS form's row limit and bytes, the back-pointer scheme
//   (exact_dist_kernel)      per chunk of steps: [chunk][n] fp32 distances, the plain search's fixed-order fp64 chain
//   seq_dp_lds_kernel        one workgroup per allowed group of at most lds_rows rows: positions, ties, rows, the predecessor
//                            ranges and two cost arrays in LDS; all steps of the chunk
//   seq_dp_global_kernel     the same arithmetic over global arrays for every longer group
//   seq_final_kernel         C_{m-1} -> each group's (D, label) order key and its end row
//   (set_select_block_kernel / set_select_merge_kernel: the clip search's selection, unchanged)
//   seq_trace_kernel         the k winners' chains from the back-pointer table the DP kernels wrote, when [m-1][n] int32 stays
//                            within SEQ_BP_BYTES; otherwise
//   seq_chain_redo_kernel    one workgroup per winner runs the DP again (distances recomputed by the same fp64 chain) and keeps
//                            the back-pointers of one slice of steps at a time, last slice first
//   seq_stats_kernel         the call's counters
//
// The rows of a group are walked in (position, tie) order — `sorder`, a second permutation next to the by-group row list,
// with the positions and ties in that order beside it (built on the host, vq_index.hip seq_order_prepare).  In that order the
// admissible predecessors of row i are a contiguous range [lo(i), hi(i)) in front of it (min_gap >= 1: hi(i) <= i), found once
// per row and launch by two binary searches and reused by every step.
//
// Costs are kept as 64-bit order-preserving keys of the fp64 value (seq_key: negative costs order correctly); SEQ_UNDEF, above
// every key of a number, marks "no chain ends here".  The smallest (cost, tie) of a range: ranges of at most 64 rows are read
// one by one; longer ones take the rows in front of the first 64-row block boundary, one stored minimum per whole block (a
// wave reduction per block and step, done only when some row of the group has such a range) and the rows behind the last
// boundary: at most 126 + L / 64 reads per row and step for a group of L rows, against L for the plain walk.  The global
// form adds one level (a minimum per 64 blocks) above 64 whole blocks: at most 252 + L / 4096 reads.
//
// Exact: every C_j(r) is one fp64 addition of two values the definition names, the minimum is taken over exactly the
// admissible rows under the total order (cost key, tie), and ties are distinct inside a group, so no step depends on the
// order in which threads run.  No scratch memory, no global atomics; workgroup barriers are the only synchronisation inside a
// launch, stream order between launches.  The launches queued depend on the shapes only.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"

#include <algorithm>

namespace vq {

constexpr int SEQ_MAX_M = 64;                                 // steps per call
constexpr int SEQ_LDS_ROWS = 4096;                            // longest group of the LDS form
constexpr int SEQ_LDS_ROW_BYTES = 2 * 8 + 5 * 4;              // two cost keys; position, tie, row, lo, hi
constexpr int64_t SEQ_DIST_BYTES = (int64_t)512 << 20;        // fp32 distances per step chunk: the exact path's allowance
constexpr int64_t SEQ_BP_BYTES = (int64_t)256 << 20;          // int32 back-pointers
constexpr uint64_t SEQ_UNDEF = ~0ull;
constexpr int SEQ_THREADS = 256;

struct SequencePlan {
    int chunk_steps;     // steps per distance chunk
    int step_chunks;     // chunks queued
    int lds_rows;        // groups of at most this many rows take the LDS form
    int lds_alloc_rows;  // rows the LDS form's arrays hold (a multiple of 64)
    int64_t lds_bytes;   // its dynamic LDS
    int global_form;     // 1: the largest group (so at least one) takes the global form
    int bp_table;        // 1: the DP writes the [m-1][n] back-pointer table, 0: the winners are redone slice by slice
    int bp_slice_steps;  // redo: steps whose back-pointers one slice holds
    int bp_slices;       // redo: slices
};

// lds_rows_override / dist_bytes_override / bp_bytes_override > 0 (tests) replace the constants above.
inline SequencePlan plan_sequence(int64_t n, int64_t largest_group, int m, int64_t lds_rows_override, int64_t dist_bytes_override,
                                  int64_t bp_bytes_override) {
    SequencePlan p;
    const int64_t ld = round_up(n, 64);
    const int64_t dist_bytes = dist_bytes_override > 0 ? dist_bytes_override : SEQ_DIST_BYTES;
    p.chunk_steps = (int)std::max<int64_t>(1, std::min<int64_t>(m, dist_bytes / (ld * 4)));
    p.step_chunks = (m + p.chunk_steps - 1) / p.chunk_steps;
    p.lds_rows = (int)(lds_rows_override > 0 ? std::min<int64_t>(lds_rows_override, SEQ_LDS_ROWS) : SEQ_LDS_ROWS);
    p.lds_alloc_rows = (int)round_up(std::max<int64_t>(1, std::min<int64_t>(p.lds_rows, largest_group)), 64);
    p.lds_bytes = (int64_t)p.lds_alloc_rows * SEQ_LDS_ROW_BYTES + (p.lds_alloc_rows / 64) * 4;
    p.global_form = largest_group > p.lds_rows ? 1 : 0;
    const int64_t bp_entries = (bp_bytes_override > 0 ? bp_bytes_override : SEQ_BP_BYTES) / 4;
    const int64_t tr = m - 1;                                  // transitions
    p.bp_table = tr * n <= bp_entries ? 1 : 0;
    p.bp_slice_steps = (int)std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(tr, 1), bp_entries / n));
    p.bp_slices = p.bp_table || tr == 0 ? 0 : (int)((tr + p.bp_slice_steps - 1) / p.bp_slice_steps);
    return p;
}

#ifdef __HIPCC__

// fp64 -> a key whose unsigned order is the order of the numbers (the 64-bit form of dist_key's transform), and back
__device__ __forceinline__ uint64_t seq_key(double c) {
    const uint64_t u = __builtin_bit_cast(uint64_t, c);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double seq_cost(uint64_t k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

struct SeqBest { uint64_t key; uint32_t tie; int32_t idx; };

__device__ __forceinline__ void seq_take(SeqBest& b, const uint64_t* c, const uint32_t* tie, int p) {
    const uint64_t k = c[p];
    if (k < b.key) { b.key = k; b.tie = tie[p]; b.idx = p; }
    else if (k == b.key && k != SEQ_UNDEF) {
        const uint32_t t = tie[p];
        if (t < b.tie) { b.tie = t; b.idx = p; }
    }
}

// the smallest (cost key, tie) of c[lo .. hi); idx -1: no defined cost in the range
// SUPER (global form): above 64 whole blocks, the blocks between 4,096-row boundaries are read as one stored minimum each (smin)
template <bool SUPER>
__device__ __forceinline__ SeqBest seq_range_min(const uint64_t* c, const uint32_t* tie, const int32_t* bmin, const int32_t* smin, int lo, int hi) {
    SeqBest b{SEQ_UNDEF, 0xffffffffu, -1};
    if (hi - lo <= 64) {
        for (int p = lo; p < hi; ++p) seq_take(b, c, tie, p);
        return b;
    }
    auto take_min = [&](const int32_t* mins, int from, int to) {
        for (int i = from; i < to; ++i) {
            const int p = mins[i];
            if (p >= 0) seq_take(b, c, tie, p);
        }
    };
    const int b0 = (lo + 63) >> 6, b1 = hi >> 6;              // whole blocks [b0, b1): b0 <= b1 for a range above 64 rows
    for (int p = lo; p < b0 * 64; ++p) seq_take(b, c, tie, p);
    if (SUPER && b1 - b0 > 64) {
        const int s0 = (b0 + 63) >> 6, s1 = b1 >> 6;          // whole superblocks [s0, s1): s0 <= s1 likewise
        take_min(bmin, b0, s0 * 64);
        take_min(smin, s0, s1);
        take_min(bmin, s1 * 64, b1);
    } else {
        take_min(bmin, b0, b1);
    }
    for (int p = b1 * 64; p < hi; ++p) seq_take(b, c, tie, p);
    return b;
}

// (key, tie << 32 | idx) minimum over a wave; ties are distinct inside a group, so idx never decides
__device__ __forceinline__ void seq_wave_min(uint64_t& key, uint64_t& ti) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ok = __shfl_xor(key, o), ot = __shfl_xor(ti, o);
        if (ok < key || (ok == key && ot < ti)) { key = ok; ti = ot; }
    }
}

// One group of L rows, one workgroup of SEQ_THREADS: steps j0 .. j0 + steps - 1 of the DP.  pos / tie / row [L]: the group in
// (position, tie) order; lo / hi [L], bmin [cdiv(L, 64)] (SUPER: [L], the superblock minima behind the block minima; L >= 2),
// c0 / c1 [L]: working arrays (LDS or global).  Step 0 fills the costs
// from the distances, a later first step takes them from carry [L]; the last step's costs go back to carry (when given).
// FROM_DIST: d(j, r) = dist[(j - j0) * ld + r]; else the fp64 chain of rows[r] . queries[j], recomputed.
// bp (or null): the predecessor's index in the group of step j's row i -> bp[(j - bp_j0) * bp_ld + i], for bp_j0 <= j < bp_j1.
template <bool FROM_DIST, bool SUPER>
__device__ __forceinline__ void seq_dp_group(const int32_t* pos, const uint32_t* tie, const int32_t* row, int32_t* lo, int32_t* hi,
                                             int32_t* bmin, uint64_t* c0, uint64_t* c1, int L, int j0, int steps, int64_t min_gap,
                                             int64_t max_gap, const float* dist, int64_t ld, const float* rows, int dim,
                                             const float* queries, uint64_t* carry, int32_t* bp, int64_t bp_ld, int bp_j0, int bp_j1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto d_of = [&](int j, int r) -> double {
        if constexpr (FROM_DIST) return (double)dist[(int64_t)(j - j0) * ld + r];
        else return (double)exact_row_dist(rows + (size_t)r * dim, queries + (size_t)j * dim, dim);
    };
    int wide = 0;
    for (int i = tid; i < L; i += SEQ_THREADS) {
        const int64_t p = pos[i];
        const int64_t first = p - max_gap, last = p - min_gap;  // admissible predecessor positions (64-bit: no wrap)
        int a = 0, b = i;                                       // first index with pos >= first
        while (a < b) { const int mid = (a + b) >> 1; if ((int64_t)pos[mid] < first) a = mid + 1; else b = mid; }
        const int l = a;
        b = i;                                                  // first index with pos > last
        while (a < b) { const int mid = (a + b) >> 1; if ((int64_t)pos[mid] <= last) a = mid + 1; else b = mid; }
        lo[i] = l; hi[i] = a;
        wide |= a - l > 64;
        c0[i] = j0 == 0 ? seq_key(d_of(0, row[i])) : carry[i];
    }
    wide = __syncthreads_or(wide);
    uint64_t* prev = c0;
    uint64_t* cur = c1;
    const int nblk = (L + 63) >> 6, nsup = (nblk + 63) >> 6;
    int32_t* smin = bmin + nblk;                                // (SUPER only: nblk + nsup <= L for every L >= 2)
    for (int s = j0 == 0 ? 1 : 0; s < steps; ++s) {
        const int j = j0 + s;
        if (wide) {
            for (int blk = wave; blk < nblk; blk += SEQ_THREADS / 64) {
                const int p = blk * 64 + lane;
                uint64_t key = p < L ? prev[p] : SEQ_UNDEF;
                uint64_t ti = p < L ? ((uint64_t)tie[p] << 32) | (uint32_t)p : ~0ull;
                seq_wave_min(key, ti);
                if (lane == 0) bmin[blk] = key == SEQ_UNDEF ? -1 : (int32_t)(uint32_t)ti;
            }
            __syncthreads();
            if constexpr (SUPER) {                              // one minimum per 64 blocks, behind the block minima
                for (int sup = wave; sup < nsup; sup += SEQ_THREADS / 64) {
                    const int blk = sup * 64 + lane;
                    const int p = blk < nblk ? bmin[blk] : -1;
                    uint64_t key = p >= 0 ? prev[p] : SEQ_UNDEF;
                    uint64_t ti = p >= 0 ? ((uint64_t)tie[p] << 32) | (uint32_t)p : ~0ull;
                    seq_wave_min(key, ti);
                    if (lane == 0) smin[sup] = key == SEQ_UNDEF ? -1 : (int32_t)(uint32_t)ti;
                }
                __syncthreads();
            }
        }
        const bool keep = bp && j >= bp_j0 && j < bp_j1;
        for (int i = tid; i < L; i += SEQ_THREADS) {
            const SeqBest best = seq_range_min<SUPER>(prev, tie, bmin, smin, lo[i], hi[i]);
            cur[i] = best.idx < 0 ? SEQ_UNDEF : seq_key(seq_cost(best.key) + d_of(j, row[i]));
            if (keep) bp[(int64_t)(j - bp_j0) * bp_ld + i] = best.idx;
        }
        __syncthreads();
        uint64_t* t = prev; prev = cur; cur = t;
    }
    if (carry)
        for (int i = tid; i < L; i += SEQ_THREADS) carry[i] = prev[i];
}

// ---- LDS form: grid = groups.  dynamic LDS: alloc_rows * SEQ_LDS_ROW_BYTES + alloc_rows / 64 * 4 (plan_sequence) ----
__global__ __launch_bounds__(SEQ_THREADS)
void seq_dp_lds_kernel(const float* __restrict__ dist, int64_t ld, int j0, int steps, const int32_t* __restrict__ goff,
                       const int32_t* __restrict__ sorder, const int32_t* __restrict__ spos, const int32_t* __restrict__ stie, int lds_rows,
                       int alloc_rows, int64_t min_gap, int64_t max_gap, uint64_t* __restrict__ carry /*[n]*/, int32_t* __restrict__ bp /*[m-1][n] or null*/,
                       int64_t n, int m, const uint32_t* __restrict__ allow) {
    extern __shared__ __attribute__((aligned(16))) char seq_smem[];
    const int g = blockIdx.x;
    if (allow && !group_allowed(allow, g)) return;              // whole workgroup leaves before any barrier
    const int b = goff[g], L = goff[g + 1] - b;
    if (L > lds_rows) return;
    uint64_t* c0 = (uint64_t*)seq_smem;
    uint64_t* c1 = c0 + alloc_rows;
    int32_t* pos = (int32_t*)(c1 + alloc_rows);
    uint32_t* tie = (uint32_t*)(pos + alloc_rows);
    int32_t* row = (int32_t*)(tie + alloc_rows);
    int32_t* lo = row + alloc_rows;
    int32_t* hi = lo + alloc_rows;
    int32_t* bmin = hi + alloc_rows;
    for (int i = threadIdx.x; i < L; i += SEQ_THREADS) {
        pos[i] = spos[b + i];
        tie[i] = (uint32_t)stie[b + i];
        row[i] = sorder[b + i];
    }
    __syncthreads();
    seq_dp_group<true, false>(pos, tie, row, lo, hi, bmin, c0, c1, L, j0, steps, min_gap, max_gap, dist, ld, nullptr, 0, nullptr, carry + b,
                       bp ? bp + b : nullptr, n, 1, m);
}

// ---- global form: every group above lds_rows; work arrays lo | hi | bmin [3][n] int32 and cost [2][n], at the group's offset ----
__global__ __launch_bounds__(SEQ_THREADS)
void seq_dp_global_kernel(const float* __restrict__ dist, int64_t ld, int j0, int steps, const int32_t* __restrict__ goff,
                          const int32_t* __restrict__ sorder, const int32_t* __restrict__ spos, const int32_t* __restrict__ stie, int lds_rows,
                          int64_t min_gap, int64_t max_gap, uint64_t* carry /*[n]*/, int32_t* work /*[3][n]*/, uint64_t* cost /*[2][n]*/,
                          int32_t* bp /*[m-1][n] or null*/, int64_t n, int m, const uint32_t* __restrict__ allow) {
    const int g = blockIdx.x;
    if (allow && !group_allowed(allow, g)) return;
    const int b = goff[g], L = goff[g + 1] - b;
    if (L <= lds_rows) return;
    seq_dp_group<true, true>(spos + b, (const uint32_t*)stie + b, sorder + b, work + b, work + n + b, work + 2 * n + b, cost + b, cost + n + b, L,
                       j0, steps, min_gap, max_gap, dist, ld, nullptr, 0, nullptr, carry + b, bp ? bp + b : nullptr, n, 1, m);
}

// ---- C_{m-1} -> ekey[g] = the order key of (D, label) (~0: no chain, or not allowed), end_idx[g] = the end row's index ----
__global__ __launch_bounds__(SEQ_THREADS)
void seq_final_kernel(const uint64_t* __restrict__ carry, const int32_t* __restrict__ goff, const int32_t* __restrict__ stie, int m,
                      const uint32_t* __restrict__ allow, uint64_t* __restrict__ ekey, int32_t* __restrict__ end_idx) {
    __shared__ uint64_t rk[SEQ_THREADS / 64], rt[SEQ_THREADS / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    if (allow && !group_allowed(allow, g)) {
        if (tid == 0) { ekey[g] = ~0ull; end_idx[g] = -1; }
        return;
    }
    const int b = goff[g], L = goff[g + 1] - b;
    uint64_t key = SEQ_UNDEF, ti = ~0ull;
    for (int i = tid; i < L; i += SEQ_THREADS) {
        const uint64_t k = carry[b + i], t = ((uint64_t)(uint32_t)stie[b + i] << 32) | (uint32_t)i;
        if (k < key || (k == key && t < ti)) { key = k; ti = t; }
    }
    seq_wave_min(key, ti);
    if ((tid & 63) == 0) { rk[tid >> 6] = key; rt[tid >> 6] = ti; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SEQ_THREADS / 64; ++w)
            if (rk[w] < key || (rk[w] == key && rt[w] < ti)) { key = rk[w]; ti = rt[w]; }
        const bool none = key == SEQ_UNDEF;
        ekey[g] = none ? ~0ull : dist_key((float)(seq_cost(key) / (double)m), (uint32_t)g);
        end_idx[g] = none ? -1 : (int32_t)(uint32_t)ti;
    }
}

// ---- chains of the k winners from the table: one thread per winner ----
__global__ __launch_bounds__(64)
void seq_trace_kernel(const int32_t* __restrict__ groups_out, int k, int m, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                      const int32_t* __restrict__ end_idx, const int32_t* __restrict__ bp /*[m-1][n]*/, int64_t n, int32_t* __restrict__ chain /*[k][m]*/) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= k) return;
    const int g = groups_out[w];
    int32_t* out = chain + (size_t)w * m;
    if (g < 0) {
        for (int j = 0; j < m; ++j) out[j] = -1;
        return;
    }
    const int b = goff[g];
    int e = end_idx[g];
    out[m - 1] = sorder[b + e];
    for (int j = m - 1; j >= 1; --j) {
        e = bp[(int64_t)(j - 1) * n + b + e];
        out[j - 1] = sorder[b + e];
    }
}

// ---- chains of the k winners without the table: grid = k, one workgroup per winner.  Slices of slice_steps transitions, the
// last first: the DP runs from step 0 to the slice's last step (global form, distances recomputed) and keeps the slice's
// back-pointers in bp [slice_steps][n] at the group's offset; thread 0 then follows them. ----
__global__ __launch_bounds__(SEQ_THREADS)
void seq_chain_redo_kernel(const int32_t* __restrict__ groups_out, int m, int slice_steps, const float* __restrict__ rows, int dim,
                           const float* __restrict__ queries, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                           const int32_t* __restrict__ spos, const int32_t* __restrict__ stie, int64_t min_gap, int64_t max_gap,
                           const int32_t* __restrict__ end_idx, int32_t* work /*[3][n]*/, uint64_t* cost /*[2][n]*/, int32_t* bp, int64_t n,
                           int32_t* chain /*[k][m]*/) {
    __shared__ int e_s;
    const int w = blockIdx.x, tid = threadIdx.x;
    const int g = groups_out[w];
    int32_t* out = chain + (size_t)w * m;
    if (g < 0) {
        for (int j = tid; j < m; j += SEQ_THREADS) out[j] = -1;
        return;
    }
    const int b = goff[g], L = goff[g + 1] - b;
    if (tid == 0) { e_s = end_idx[g]; out[m - 1] = sorder[b + e_s]; }
    for (int top = m - 1; top >= 1; top -= slice_steps) {       // transitions bot .. top of this slice
        const int bot = max(1, top - slice_steps + 1);
        __syncthreads();
        seq_dp_group<false, true>(spos + b, (const uint32_t*)stie + b, sorder + b, work + b, work + n + b, work + 2 * n + b, cost + b, cost + n + b,
                            L, 0, top + 1, min_gap, max_gap, nullptr, 0, rows, dim, queries, nullptr, bp + b, n, bot, top + 1);
        __syncthreads();
        if (tid == 0) {
            int e = e_s;
            for (int j = top; j >= bot; --j) {
                e = bp[(int64_t)(j - bot) * n + b + e];
                out[j - 1] = sorder[b + e];
            }
            e_s = e;
        }
    }
}

// ---- the call's counters: groups that hold a chain, and the two figures the host knows ----
__global__ __launch_bounds__(256)
void seq_stats_kernel(const uint64_t* __restrict__ ekey, int n_groups, unsigned long long global_groups, unsigned long long chunks,
                      unsigned long long* __restrict__ counters) {
    __shared__ int red[4];
    const int tid = threadIdx.x;
    int c = 0;
    for (int g = tid; g < n_groups; g += 256) c += ekey[g] != ~0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        counters[0] = (unsigned long long)(red[0] + red[1] + red[2] + red[3]);
        counters[1] = global_groups;
        counters[2] = chunks;
    }
}

#endif  // __HIPCC__

}  // namespace vq
