// Warped clip alignment (vq_index_align_clip): the k GROUPS (videos) that show a clip of m frames under a monotone time warp —
// a subsequence dynamic time warp of the clip against every allowed group, both ends free, over the integer costs
// c = rint(d * 2^24)  (include/vq_amd.h has the definition; DESIGN.md §4 "Warped alignment").
//
//   plan_align               host only: the clip chunks, the LDS form's row limit and bytes, the carried state, the winner batches
//   (exact_dist_kernel)      per chunk of clip frames: [chunk][n] fp32 distances, the plain search's fixed-order fp64 chain
//   align_dp_lds_kernel      one workgroup per allowed group of at most lds_rows rows: the chunk's clip frames one after the
//                            other over the group's rows, the DP row (cost, start) in LDS
//   align_dp_global_kernel   the same arithmetic on the carried state in global memory for every longer group
//   align_final_kernel       the last DP row -> each group's (D, label) key, cost and (a, b); "none" above max_dist
//   (set_select_block_kernel / set_select_merge_kernel: the clip search's selection, unchanged; seq_stats_kernel: the counters)
//   align_order_kernel       the selected groups by (C, label) where different costs round to one D
//   align_finish_kernel      the k winners' costs and (start, end) rows
//   align_trace_dp_kernel    one workgroup per winner runs its group's DP again and writes the entry column of every cell
//   align_walk_kernel        ... and one thread per winner walks that table back from (m - 1, b)
//
// The rows of a group are walked in the sequence search's (position, tie) order (vq_index.hip seq_order_prepare).  A path
// enters DP row i at some column j' — from row i - 1 at j' - 1 (diagonal) or at j' (vertical), whichever key (C, -a) is the
// smaller, ties to the diagonal; at i = 0 it starts there, at no cost — and then runs along the row to j.  With
// P = the exclusive prefix sums of c(i, .) that is
//   cell(i, j) = P[j + 1] + min over j' <= j of (E(j').C - P[j'], -E(j').a, -j'),
// one prefix sum and one prefix minimum over 256-row tiles, the running values carried from tile to tile by every thread
// alike (as knn_span.h does).  The scanned keys hold j', so they are distinct and the order in which lanes combine them does not
// matter; ties go to the later start, then to the later entry: the predecessor order diagonal, vertical, horizontal.
//
// Exact: the cost is the last floating-point operation.  Everything behind it is integer addition and comparison under total
// orders whose keys are distinct, so the two forms agree bit for bit.  No scratch memory, no global atomics; workgroup barriers
// are the only synchronisation inside a launch, stream order between launches.  The launches queued depend on the shapes and
// the arguments only.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"

#include <algorithm>

namespace vq {

constexpr int ALIGN_MAX_M = 4096;                              // clip frames per call
constexpr int ALIGN_LDS_ROWS = 4096;                           // longest group of the LDS form
constexpr int ALIGN_LDS_ROW_BYTES = 8 + 4 + 4;                 // cost, start; the row's number in the full index
constexpr int64_t ALIGN_DIST_BYTES = (int64_t)512 << 20;       // fp32 distances per clip chunk: the exact path's allowance
constexpr int64_t ALIGN_BP_BYTES = (int64_t)256 << 20;         // entry-column tables of one batch of winners
constexpr int64_t ALIGN_TABLE_MAX_BYTES = (int64_t)1 << 30;    // one winner's table [m][rows of the largest allowed group] int32
constexpr int64_t ALIGN_CU_LDS_BYTES = (int64_t)160 << 10;     // what a CU holds
constexpr int ALIGN_THREADS = 256;
constexpr int64_t ALIGN_COST_CAP = (int64_t)1 << 31;           // |c| saturates here: sums over 4,096 frames and 2^31 rows stay inside int64

struct AlignPlan {
    int chunk_frames;      // clip frames per distance chunk
    int frame_chunks;      // chunks queued
    int lds_rows;          // groups of at most this many rows take the LDS form
    int lds_alloc_rows;    // rows the LDS form's arrays hold (a multiple of 64)
    int64_t lds_bytes;     // its dynamic LDS
    int global_form;       // 1: the largest allowed group (so at least one) takes the global form
    int64_t state_bytes;   // the DP row carried between chunks (and the global form's working row): [n] int64 + [n] int32
    int winners_per_batch; // with alignments: winners whose tables one batch holds (0 without)
    int winner_batches;    // batches queued
    int64_t table_bytes;   // the batch's tables
};

// dynamic LDS of the LDS form for arrays of `rows` rows (a multiple of 64)
constexpr int64_t align_lds_bytes(int64_t rows) { return rows * ALIGN_LDS_ROW_BYTES; }
static_assert(align_lds_bytes(ALIGN_LDS_ROWS) <= ALIGN_CU_LDS_BYTES, "align_dp_lds_kernel: 4,096 rows must fit a CU's LDS");

// largest_group: the largest ALLOWED group; winners: min(k, allowed groups).  The *_override values > 0 (tests) replace the
// constants above.  The caller has refused a table above ALIGN_TABLE_MAX_BYTES.
inline AlignPlan plan_align(int64_t n, int64_t largest_group, int m, int winners, bool with_align, int64_t lds_rows_override,
                            int64_t dist_bytes_override, int64_t bp_bytes_override) {
    AlignPlan p;
    const int64_t ld = round_up(n, 64);
    const int64_t dist_bytes = dist_bytes_override > 0 ? dist_bytes_override : ALIGN_DIST_BYTES;
    p.chunk_frames = (int)std::max<int64_t>(1, std::min<int64_t>(m, dist_bytes / (ld * 4)));
    p.frame_chunks = (m + p.chunk_frames - 1) / p.chunk_frames;
    p.lds_rows = (int)(lds_rows_override > 0 ? std::min<int64_t>(lds_rows_override, ALIGN_LDS_ROWS) : ALIGN_LDS_ROWS);
    p.lds_alloc_rows = (int)round_up(std::max<int64_t>(1, std::min<int64_t>(p.lds_rows, largest_group)), 64);
    p.lds_bytes = align_lds_bytes(p.lds_alloc_rows);
    p.global_form = largest_group > p.lds_rows ? 1 : 0;
    p.state_bytes = n * 12;
    p.winners_per_batch = 0; p.winner_batches = 0; p.table_bytes = 0;
    if (with_align && winners > 0) {
        const int64_t one = (int64_t)m * largest_group * 4;
        const int64_t budget = bp_bytes_override > 0 ? bp_bytes_override : ALIGN_BP_BYTES;
        p.winners_per_batch = (int)std::max<int64_t>(1, std::min<int64_t>(winners, budget / std::max<int64_t>(one, 1)));
        p.winner_batches = (winners + p.winners_per_batch - 1) / p.winners_per_batch;
        p.table_bytes = one * p.winners_per_batch;
    }
    return p;
}

#ifdef __HIPCC__

// the integer cost of a distance (the definition's only floating-point step; a NaN distance takes the largest cost)
__device__ __forceinline__ int64_t align_cost(float d) {
    if (d != d) return ALIGN_COST_CAP;
    const double c = rint((double)d * 16777216.0);
    return (int64_t)fmin(fmax(c, -(double)ALIGN_COST_CAP), (double)ALIGN_COST_CAP);
}
// D of a cost: fp32((double)C * 2^-24 / (double)m)
__device__ __forceinline__ float align_rank_value(int64_t cost, int m) { return (float)((double)cost * (1.0 / 16777216.0) / (double)m); }

// An entry candidate of a DP row: v = E.C - P[j'], a = E's start, code = 2 j' + (1: E came down the diagonal).
// Order: smallest v, then the latest start, then the latest entry column.
struct AlignKey { int64_t v; int32_t a; uint32_t code; };
__device__ __forceinline__ bool align_before(const AlignKey& x, const AlignKey& y) {
    if (x.v != y.v) return x.v < y.v;
    if (x.a != y.a) return x.a > y.a;
    return x.code > y.code;
}
__device__ __forceinline__ AlignKey align_shfl_up(const AlignKey& k, int o) {
    AlignKey r;
    r.v = __shfl_up((long long)k.v, o); r.a = __shfl_up(k.a, o); r.code = (uint32_t)__shfl_up((int)k.code, o);
    return r;
}

struct AlignShared {
    int64_t sum[ALIGN_THREADS / 64];
    int64_t mv[ALIGN_THREADS / 64]; int32_t ma[ALIGN_THREADS / 64]; uint32_t mc[ALIGN_THREADS / 64];
    int64_t edge_c; int32_t edge_a;                            // the previous DP row's cell in front of the next tile
    int64_t rc[ALIGN_THREADS / 64]; int32_t rl[ALIGN_THREADS / 64]; int32_t ra[ALIGN_THREADS / 64];
};

// One DP row (clip frame i) over a group of L rows, one workgroup of ALIGN_THREADS.  row [L]: the group's rows in (position,
// tie) order as full-index row numbers; drow [n]: frame i's distances by full-index row; C / A [L]: the previous DP row in, this
// one out (LDS or global); first: i = 0, nothing is read.  bp (BP only) [L]: the entry column of every cell, top bit = the path
// came down the diagonal into it.  Ends behind a barrier: C / A are complete.
template <bool BP>
__device__ __forceinline__ void align_row(const int32_t* row, const float* drow, bool first, int64_t* C, int32_t* A, int L, int32_t* bp,
                                          AlignShared* sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry_sum = 0;
    AlignKey carry{INT64_MAX, -1, 0u};
    int64_t edge_c = 0; int32_t edge_a = 0;                    // C / A [t0 - 1] of the previous DP row (tile 0 never reads it)
    for (int t0 = 0; t0 < L; t0 += ALIGN_THREADS) {
        const int j = t0 + tid;
        const bool in = j < L;
        const int64_t w = in ? align_cost(drow[row[j]]) : 0;
        AlignKey e{INT64_MAX, -1, 0u};                         // E(j): where a path may enter this DP row at column j
        int64_t own_c = 0; int32_t own_a = 0;
        if (in) {
            if (first) {
                e = AlignKey{0, j, 2u * (uint32_t)j};
            } else {
                own_c = C[j]; own_a = A[j];
                e = AlignKey{own_c, own_a, 2u * (uint32_t)j};
                if (j > 0) {
                    const int64_t lc = tid == 0 ? edge_c : C[j - 1];
                    const int32_t la = tid == 0 ? edge_a : A[j - 1];
                    if (lc < own_c || (lc == own_c && la >= own_a)) e = AlignKey{lc, la, 2u * (uint32_t)j + 1u};
                }
            }
        }
        // inclusive wave scan: the sum of the costs
        int64_t s = w;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t os = __shfl_up((long long)s, o);
            if (lane >= o) s += os;
        }
        if (lane == 63) sh->sum[wave] = s;
        if (tid == ALIGN_THREADS - 1) { sh->edge_c = own_c; sh->edge_a = own_a; }     // (a full tile whenever another follows)
        __syncthreads();
        int64_t front = carry_sum, total = carry_sum;
#pragma unroll
        for (int v = 0; v < ALIGN_THREADS / 64; ++v) {
            if (v < wave) front += sh->sum[v];
            total += sh->sum[v];
        }
        edge_c = sh->edge_c; edge_a = sh->edge_a;
        const int64_t excl = front + s - w;                    // P[j]
        // inclusive wave scan: the best entry so far
        AlignKey k = e;
        if (in) k.v = e.v - excl;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const AlignKey ok = align_shfl_up(k, o);
            if (lane >= o && align_before(ok, k)) k = ok;
        }
        if (lane == 63) { sh->mv[wave] = k.v; sh->ma[wave] = k.a; sh->mc[wave] = k.code; }
        __syncthreads();
        AlignKey fk = carry, tk = carry;
#pragma unroll
        for (int v = 0; v < ALIGN_THREADS / 64; ++v) {
            const AlignKey ok{sh->mv[v], sh->ma[v], sh->mc[v]};
            if (v < wave && align_before(ok, fk)) fk = ok;
            if (align_before(ok, tk)) tk = ok;
        }
        if (align_before(fk, k)) k = fk;
        if (in) {                                              // (every thread has read its C / A [j - 1], [j] two barriers ago)
            C[j] = excl + w + k.v;
            A[j] = k.a;
            if constexpr (BP) bp[j] = (int32_t)((k.code >> 1) | ((k.code & 1u) << 31));
        }
        carry_sum = total; carry = tk;
        // (no barrier: the next tile writes sh->sum / edge, which nobody reads behind the second barrier above, and sh->mv / ma /
        // mc only behind its own first barrier)
    }
    __syncthreads();                                           // the next DP row reads what this one wrote
}

// ---- LDS form: grid = groups.  dynamic LDS: align_lds_bytes(alloc_rows).  i0: the chunk's first clip frame; the DP row
// comes in from state_c / state_a (i0 > 0) and goes back out at the group's offset. ----
__global__ __launch_bounds__(ALIGN_THREADS)
void align_dp_lds_kernel(const float* __restrict__ dist, int64_t ld, int i0, int cur, const int32_t* __restrict__ goff,
                         const int32_t* __restrict__ sorder, int lds_rows, int alloc_rows, int64_t* __restrict__ state_c,
                         int32_t* __restrict__ state_a, const uint32_t* __restrict__ allow) {
    extern __shared__ __attribute__((aligned(16))) char align_smem[];
    __shared__ AlignShared sh;
    const int g = blockIdx.x;
    if (allow && !group_allowed(allow, g)) return;             // whole workgroup leaves before any barrier
    const int b = goff[g], L = goff[g + 1] - b;
    if (L == 0 || L > lds_rows) return;                        // a label no row carries; the global form's
    int64_t* C = (int64_t*)align_smem;
    int32_t* A = (int32_t*)(C + alloc_rows);
    int32_t* row = A + alloc_rows;
    for (int j = threadIdx.x; j < L; j += ALIGN_THREADS) {
        row[j] = sorder[b + j];
        if (i0 > 0) { C[j] = state_c[b + j]; A[j] = state_a[b + j]; }
    }
    __syncthreads();
    for (int i = 0; i < cur; ++i) align_row<false>(row, dist + (int64_t)i * ld, i0 + i == 0, C, A, L, nullptr, &sh);
    for (int j = threadIdx.x; j < L; j += ALIGN_THREADS) { state_c[b + j] = C[j]; state_a[b + j] = A[j]; }
}

// ---- global form: grid = groups; every allowed group above lds_rows, on the carried state itself ----
__global__ __launch_bounds__(ALIGN_THREADS)
void align_dp_global_kernel(const float* __restrict__ dist, int64_t ld, int i0, int cur, const int32_t* __restrict__ goff,
                            const int32_t* __restrict__ sorder, int lds_rows, int64_t* state_c, int32_t* state_a,
                            const uint32_t* __restrict__ allow) {
    __shared__ AlignShared sh;
    const int g = blockIdx.x;
    if (allow && !group_allowed(allow, g)) return;
    const int b = goff[g], L = goff[g + 1] - b;
    if (L <= lds_rows) return;
    for (int i = 0; i < cur; ++i) align_row<false>(sorder + b, dist + (int64_t)i * ld, i0 + i == 0, state_c + b, state_a + b, L, nullptr, &sh);
}

// ---- the last DP row -> the group's result: grid = groups.  The end b with the smallest (C, b - a + 1, a); ekey: the (D, label)
// order key, ~0 for "none" (not allowed, no row, D above max_dist); gcost / gab: C and (a, b). ----
__global__ __launch_bounds__(ALIGN_THREADS)
void align_final_kernel(const int64_t* __restrict__ state_c, const int32_t* __restrict__ state_a, const int32_t* __restrict__ goff, int m,
                        float max_dist, const uint32_t* __restrict__ allow, uint64_t* __restrict__ ekey, int64_t* __restrict__ gcost,
                        int32_t* __restrict__ gab) {
    __shared__ AlignShared sh;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int base = goff[g], L = goff[g + 1] - base;
    if ((allow && !group_allowed(allow, g)) || L == 0) {
        if (tid == 0) { ekey[g] = ~0ull; gcost[g] = 0; gab[2 * g] = -1; gab[2 * g + 1] = -1; }
        return;
    }
    int64_t bc = INT64_MAX; int32_t bl = 0x7fffffff, ba = 0x7fffffff;
    auto take = [&](int64_t c, int32_t l, int32_t a) {
        if (c < bc || (c == bc && (l < bl || (l == bl && a < ba)))) { bc = c; bl = l; ba = a; }
    };
    for (int j = tid; j < L; j += ALIGN_THREADS) {
        const int32_t a = state_a[base + j];
        take(state_c[base + j], j - a + 1, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t oc = __shfl_xor((long long)bc, o);
        const int32_t ol = __shfl_xor(bl, o), oa = __shfl_xor(ba, o);
        take(oc, ol, oa);
    }
    if ((tid & 63) == 0) { sh.rc[tid >> 6] = bc; sh.rl[tid >> 6] = bl; sh.ra[tid >> 6] = ba; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < ALIGN_THREADS / 64; ++v) take(sh.rc[v], sh.rl[v], sh.ra[v]);
        const float D = align_rank_value(bc, m);
        const bool none = !(D <= max_dist);
        ekey[g] = none ? ~0ull : dist_key(D, (uint32_t)g);
        gcost[g] = bc; gab[2 * g] = ba; gab[2 * g + 1] = ba + bl - 1;
    }
}

// ---- the selection orders by (D, label), the definition by (C, label).  D never decreases as C grows, so the two differ only
// among groups whose different costs round to one fp32 D.  grid = k, one workgroup per result slot: slot j, the t-th of the
// slots that hold its D, takes the group of rank t by (C, label) among ALL the groups that hold that D (of which the selection
// took the first by label).  Costs that share a D lie within m x 2^24 x ulp(D) <= 2^19 of each other, so (C - the smallest of
// them, label) is one 64-bit key.  sel [k]: the selection's groups; at most j + 1 <= k passes over the groups. ----
__global__ __launch_bounds__(256)
void align_order_kernel(const uint64_t* __restrict__ ekey, int n_groups, const int64_t* __restrict__ gcost, const int32_t* __restrict__ sel,
                        int32_t* __restrict__ groups_out) {
    __shared__ uint64_t red[4];
    __shared__ int64_t rmin[4];
    __shared__ int rt[4], rn[4];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int g0 = sel[j];
    if (g0 < 0) {                                              // block-uniform
        if (tid == 0) groups_out[j] = -1;
        return;
    }
    const uint32_t hi = (uint32_t)(ekey[g0] >> 32);            // (never that of ~0: D is no NaN)
    int t = 0, members = 0;
    int64_t cmin = INT64_MAX;
    for (int i = tid; i < j; i += 256) t += (uint32_t)(ekey[sel[i]] >> 32) == hi;          // (slots in front of a filled one are filled)
    for (int g = tid; g < n_groups; g += 256)
        if ((uint32_t)(ekey[g] >> 32) == hi) { ++members; const int64_t c = gcost[g]; cmin = c < cmin ? c : cmin; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t += __shfl_xor(t, o); members += __shfl_xor(members, o);
        const int64_t oc = __shfl_xor((long long)cmin, o);
        cmin = oc < cmin ? oc : cmin;
    }
    if ((tid & 63) == 0) { rt[tid >> 6] = t; rn[tid >> 6] = members; rmin[tid >> 6] = cmin; }
    __syncthreads();
    t = rt[0] + rt[1] + rt[2] + rt[3]; members = rn[0] + rn[1] + rn[2] + rn[3];
    cmin = rmin[0];
#pragma unroll
    for (int v = 1; v < 4; ++v) cmin = rmin[v] < cmin ? rmin[v] : cmin;
    if (members == 1) {                                        // block-uniform: the common case
        if (tid == 0) groups_out[j] = g0;
        return;
    }
    uint64_t prev = 0;
    for (int r = 0; r <= t; ++r) {                             // the smallest key above the previous one, t + 1 times
        uint64_t best = ~0ull;
        for (int g = tid; g < n_groups; g += 256) {
            if ((uint32_t)(ekey[g] >> 32) != hi) continue;
            const uint64_t key = ((uint64_t)(gcost[g] - cmin) << 32) | (uint32_t)g;
            if ((r == 0 || key > prev) && key < best) best = key;
        }
        prev = block_min_u64(best, red, tid);
    }
    if (tid == 0) groups_out[j] = (int32_t)(uint32_t)prev;
}

// ---- the k winners' costs and rows: one thread per result slot; cost / rows may each be null ----
__global__ __launch_bounds__(64)
void align_finish_kernel(const int32_t* __restrict__ groups_out, int k, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                         const int64_t* __restrict__ gcost, const int32_t* __restrict__ gab, int64_t* __restrict__ cost,
                         int32_t* __restrict__ rows /*[k][2]*/) {
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= k) return;
    const int g = groups_out[w];
    if (cost) cost[w] = g < 0 ? 0 : gcost[g];
    if (rows) {
        rows[2 * w] = g < 0 ? -1 : sorder[goff[g] + gab[2 * g]];
        rows[2 * w + 1] = g < 0 ? -1 : sorder[goff[g] + gab[2 * g + 1]];
    }
}

// ---- winners' tables: grid = the batch's winners (result slots w0 ..), one workgroup per winner.  The group's DP again over
// the chunk's clip frames, on the carried state at the group's offset (winners are distinct groups, and the first pass is
// over); table [batch][stride] int32: the winner's [m][L] entry columns. ----
__global__ __launch_bounds__(ALIGN_THREADS)
void align_trace_dp_kernel(const float* __restrict__ dist, int64_t ld, int i0, int cur, const int32_t* __restrict__ groups_out, int w0,
                           const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder, int64_t* state_c, int32_t* state_a,
                           int32_t* table, int64_t stride) {
    __shared__ AlignShared sh;
    const int g = groups_out[w0 + blockIdx.x];
    if (g < 0) return;
    const int b = goff[g], L = goff[g + 1] - b;
    int32_t* bp = table + (int64_t)blockIdx.x * stride;
    for (int i = 0; i < cur; ++i)
        align_row<true>(sorder + b, dist + (int64_t)i * ld, i0 + i == 0, state_c + b, state_a + b, L, bp + (int64_t)(i0 + i) * L, &sh);
}

// ---- ... walked back from (m - 1, b): one thread per winner of the batch.  align [k][m][2]: per clip frame the first and the
// last stored row paired with it (full-index row numbers); -1 in an unused slot. ----
__global__ __launch_bounds__(64)
void align_walk_kernel(const int32_t* __restrict__ groups_out, int w0, int count, int m, const int32_t* __restrict__ goff,
                       const int32_t* __restrict__ sorder, const int32_t* __restrict__ gab, const int32_t* __restrict__ table, int64_t stride,
                       int32_t* __restrict__ align) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= count) return;
    const int g = groups_out[w0 + t];
    int32_t* out = align + (int64_t)(w0 + t) * m * 2;
    if (g < 0) {
        for (int i = 0; i < 2 * m; ++i) out[i] = -1;
        return;
    }
    const int b = goff[g], L = goff[g + 1] - b;
    const int32_t* bp = table + (int64_t)t * stride;
    int j = gab[2 * g + 1];
    for (int i = m - 1; i >= 0; --i) {
        const uint32_t e = (uint32_t)bp[(int64_t)i * L + j];
        const int col = (int)(e & 0x7fffffffu);
        out[2 * i] = sorder[b + col];
        out[2 * i + 1] = sorder[b + j];
        j = (e >> 31) ? col - 1 : col;
    }
}

#endif  // __HIPCC__

}  // namespace vq
