// Span search (vq_index_search_spans): per query the k GROUPS (videos) with the best TIME SPAN — a run of consecutive rows of
// one group, in (position, tie) order, whose summed integer gain  w = rint((tau - d) * 2^24)  is the largest among the runs
// that respect max_gap (between neighbours) and max_span (first to last)  (include/vq_amd.h has the definition; DESIGN.md §4
// "Span search").
//
//   plan_spans               host only: the query chunks, the LDS form's row limit and bytes, the global form's scratch
//   (exact_dist_kernel)      per chunk of queries: [chunk][n] fp32 distances, the plain search's fixed-order fp64 chain
//   span_lds_kernel          one workgroup per (allowed group of at most lds_rows rows, query of the chunk): positions, prefix
//                            sums, range starts and prefix minima in LDS
//   span_global_kernel       the same arithmetic over global arrays for every longer group, one workgroup per group that takes
//                            the chunk's queries one after the other
//   (set_select_block_kernel / set_select_merge_kernel: the clip search's selection, unchanged, once per query)
//   span_finish_kernel       the k winners of every query: mass, length, start, end and peak rows
//   span_stats_kernel        the call's counters
//
// The rows of a group are walked in the sequence search's (position, tie) order (vq_index.hip seq_order_prepare).  One pass
// over 256-row tiles, the running values carried from tile to tile by every thread alike, builds
//   P[0 .. L]   the exclusive prefix sums of the gains (int64),
//   lo[b]       the first admissible start of a span that ends at b: the larger of the start of b's segment (a max-scan over
//               the indices behind a gap above max_gap) and the first index whose position is within max_span of b's (a binary
//               search over the sorted positions),
//   pm[b]       the index in [0, b] with the smallest P, ties to the largest index (a min-scan).
// The best start for b is a(b) = the index in [lo(b), b] with the smallest P, ties to the largest: pm[b] where lo(b) = 0 (always,
// when both limits are unlimited); otherwise a range minimum.  Ranges of at most 64 rows are read one by one; longer ones take the
// rows in front of the first 64-row block boundary, one stored minimum per whole block and the rows behind the last boundary: at
// most 126 + L / 64 reads per row for a group of L rows.  The global form adds one level (a minimum per 64 blocks) above 64 whole
// blocks: at most 252 + L / 4096 reads.  The block minima are built only when some row of the group has a range above 64 rows
// that does not start at 0.  The candidate of b is (P[b+1] - P[a(b)], b - a(b) + 1, a(b)); the group's span is the candidate
// with the largest mass, then the shortest, then the earliest, if its mass is positive.
//
// Exact: the gain is the last floating-point operation.  Everything behind it is integer addition and comparison under total
// orders whose keys are distinct, so no result depends on the order in which threads run, and the two forms agree bit for bit.
// No scratch memory, no global atomics; workgroup barriers are the only synchronisation inside a launch, stream order between
// launches.  The launches queued depend on the shapes only.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"

#include <algorithm>

namespace vq {

constexpr int SPAN_MAX_Q = 64;                                // queries per call
constexpr int SPAN_LDS_ROWS = 4096;                           // longest group of the LDS form
constexpr int SPAN_LDS_ROW_BYTES = 8 + 3 * 4;                 // prefix sum; position, range start, prefix minimum
constexpr int64_t SPAN_DIST_BYTES = (int64_t)512 << 20;       // fp32 distances per query chunk: the exact path's allowance
constexpr int64_t SPAN_CU_LDS_BYTES = (int64_t)160 << 10;     // what a CU holds
constexpr int SPAN_THREADS = 256;
constexpr int64_t SPAN_GAIN_CAP = (int64_t)1 << 31;           // |w| saturates here: sums over fewer than 2^31 rows stay inside int64

struct SpanPlan {
    int chunk_queries;   // queries per distance chunk
    int query_chunks;    // chunks queued
    int lds_rows;        // groups of at most this many rows take the LDS form
    int lds_alloc_rows;  // rows the LDS form's arrays hold (a multiple of 64)
    int64_t lds_bytes;   // its dynamic LDS
    int global_form;     // 1: the largest group (so at least one) takes the global form
    int64_t scratch_bytes;  // the global form's arrays (0 without it)
};

// dynamic LDS of the LDS form for arrays of `rows` rows (a multiple of 64): P [rows + 2] int64, three int32 arrays, block minima
constexpr int64_t span_lds_bytes(int64_t rows) { return (rows + 2) * 8 + rows * 12 + (rows / 64) * 4; }
static_assert(span_lds_bytes(SPAN_LDS_ROWS) <= SPAN_CU_LDS_BYTES, "span_lds_kernel: 4,096 rows must fit a CU's LDS");
static_assert(SPAN_LDS_ROW_BYTES * SPAN_LDS_ROWS <= SPAN_CU_LDS_BYTES, "span_lds_kernel: per-row bytes");

// lds_rows_override / dist_bytes_override > 0 (tests) replace the constants above.
inline SpanPlan plan_spans(int64_t n, int64_t n_groups, int64_t largest_group, int nq, int64_t lds_rows_override, int64_t dist_bytes_override) {
    SpanPlan p;
    const int64_t ld = round_up(n, 64);
    const int64_t dist_bytes = dist_bytes_override > 0 ? dist_bytes_override : SPAN_DIST_BYTES;
    p.chunk_queries = (int)std::max<int64_t>(1, std::min<int64_t>(nq, dist_bytes / (ld * 4)));
    p.query_chunks = (nq + p.chunk_queries - 1) / p.chunk_queries;
    p.lds_rows = (int)(lds_rows_override > 0 ? std::min<int64_t>(lds_rows_override, SPAN_LDS_ROWS) : SPAN_LDS_ROWS);
    p.lds_alloc_rows = (int)round_up(std::max<int64_t>(1, std::min<int64_t>(p.lds_rows, largest_group)), 64);
    p.lds_bytes = span_lds_bytes(p.lds_alloc_rows);
    p.global_form = largest_group > p.lds_rows ? 1 : 0;
    p.scratch_bytes = p.global_form ? (n + n_groups) * 8 + 3 * n * 4 : 0;     // P [n + groups] int64; lo | pm | minima [3][n] int32
    return p;
}

#ifdef __HIPCC__

// the integer gain of a distance (the definition's only floating-point step; NaN distances take the most negative gain)
__device__ __forceinline__ int64_t span_gain(float tau, float d) {
    const double g = rint(((double)tau - (double)d) * 16777216.0);
    return (int64_t)fmin(fmax(g, -(double)SPAN_GAIN_CAP), (double)SPAN_GAIN_CAP);
}
// D of a mass: fp32(-(double)S * 2^-24)
__device__ __forceinline__ float span_rank_value(int64_t mass) { return (float)(-(double)mass * (1.0 / 16777216.0)); }

// (value, index): is (v, i) in front of (bv, bi) under "smallest value, ties to the largest index"?
__device__ __forceinline__ bool span_min_before(int64_t v, int i, int64_t bv, int bi) { return v < bv || (v == bv && i > bi); }

struct SpanMin { int64_t v; int32_t idx; };
__device__ __forceinline__ void span_take(SpanMin& m, const int64_t* P, int p) {
    const int64_t v = P[p];
    if (span_min_before(v, p, m.v, m.idx)) { m.v = v; m.idx = p; }
}

// the index of the smallest P[lo .. hi), ties to the largest index; hi > lo
// SUPER (global form): above 64 whole blocks, the blocks between 4,096-row boundaries are read as one stored minimum each (smin)
template <bool SUPER>
__device__ __forceinline__ int span_range_min(const int64_t* P, const int32_t* bmin, const int32_t* smin, int lo, int hi) {
    SpanMin m{INT64_MAX, -1};
    if (hi - lo <= 64) {
        for (int p = lo; p < hi; ++p) span_take(m, P, p);
        return m.idx;
    }
    const int b0 = (lo + 63) >> 6, b1 = hi >> 6;              // whole blocks [b0, b1): b0 <= b1 for a range above 64 rows
    for (int p = lo; p < b0 * 64; ++p) span_take(m, P, p);
    if (SUPER && b1 - b0 > 64) {
        const int s0 = (b0 + 63) >> 6, s1 = b1 >> 6;          // whole superblocks [s0, s1): s0 <= s1 likewise
        for (int i = b0; i < s0 * 64; ++i) span_take(m, P, bmin[i]);
        for (int i = s0; i < s1; ++i) span_take(m, P, smin[i]);
        for (int i = s1 * 64; i < b1; ++i) span_take(m, P, bmin[i]);
    } else {
        for (int i = b0; i < b1; ++i) span_take(m, P, bmin[i]);
    }
    for (int p = b1 * 64; p < hi; ++p) span_take(m, P, p);
    return m.idx;
}

// the smallest (value, ties to the largest index) of a wave, in every lane
__device__ __forceinline__ void span_wave_min(int64_t& v, int& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t ov = __shfl_xor((long long)v, o);
        const int oi = __shfl_xor(idx, o);
        if (span_min_before(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
}

// a span candidate: is (s, len, a) in front of (bs, bl, ba) under "largest mass, then shortest, then earliest"?
struct SpanCand { int64_t s; int32_t len; int32_t a; };
__device__ __forceinline__ bool span_cand_before(const SpanCand& c, const SpanCand& b) {
    if (c.s != b.s) return c.s > b.s;
    if (c.len != b.len) return c.len < b.len;
    return c.a < b.a;
}

// One group of L rows and one query, one workgroup of SPAN_THREADS.  pos / row [L]: the group in (position, tie) order (LDS or
// global); drow [n]: the query's distances by full-index row.  Work arrays (LDS or global): P [L + 1], lo / pm [L], bmin
// [cdiv(L, 64)] (SUPER: the superblock minima behind the block minima; [L] holds both for every L >= 2).  sh: the LDS through
// which the waves exchange their scan totals and candidates.  Returns the group's span to thread 0 (s <= 0: none).
struct SpanShared { int64_t sum[4]; int64_t mv[4]; int32_t brk[4]; int32_t mi[4]; int64_t cs[4]; int32_t cl[4]; int32_t ca[4]; };

template <bool SUPER>
__device__ __forceinline__ SpanCand span_group(const int32_t* pos, const int32_t* row, const float* drow, float tau, int64_t max_gap,
                                               int64_t max_span, int64_t* P, int32_t* lo, int32_t* pm, int32_t* bmin, int L, SpanShared* sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool span_limited = max_span < ((int64_t)1 << 32);
    // the carries: the sum in front of the tile, the last break index, the prefix minimum (P[0] = 0 at index 0 to begin with;
    // the first element of the first tile replaces nothing: it IS (0, 0))
    int64_t carry_sum = 0;
    int carry_brk = 0;
    int64_t carry_mv = INT64_MAX;
    int carry_mi = -1;
    int wide = 0;
    for (int t0 = 0; t0 < L; t0 += SPAN_THREADS) {
        const int i = t0 + tid;
        const bool in = i < L;
        const int64_t w = in ? span_gain(tau, drow[row[i]]) : 0;
        const int64_t p_i = in ? (int64_t)pos[i] : 0;
        int brk = in && i > 0 && p_i - (int64_t)pos[i - 1] > max_gap ? i : 0;
        // inclusive wave scans: the sum of the gains, the largest break index
        int64_t s = w;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t os = __shfl_up((long long)s, o);
            const int ob = __shfl_up(brk, o);
            if (lane >= o) { s += os; brk = max(brk, ob); }
        }
        if (lane == 63) { sh->sum[wave] = s; sh->brk[wave] = brk; }
        __syncthreads();
        int64_t front = carry_sum, total = carry_sum;
        int fbrk = carry_brk, tbrk = carry_brk;
#pragma unroll
        for (int v = 0; v < SPAN_THREADS / 64; ++v) {
            if (v < wave) { front += sh->sum[v]; fbrk = max(fbrk, sh->brk[v]); }
            total += sh->sum[v]; tbrk = max(tbrk, sh->brk[v]);
        }
        const int64_t excl = front + s - w;                    // P[i]
        brk = max(brk, fbrk);                                  // the start of i's segment
        // inclusive wave scan: the smallest P so far, ties to the largest index
        int64_t mv = in ? excl : INT64_MAX;
        int mi = in ? i : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t ov = __shfl_up((long long)mv, o);
            const int oi = __shfl_up(mi, o);
            if (lane >= o && !span_min_before(mv, mi, ov, oi)) { mv = ov; mi = oi; }
        }
        if (lane == 63) { sh->mv[wave] = mv; sh->mi[wave] = mi; }
        __syncthreads();
        int64_t fmv = carry_mv, tmv = carry_mv;
        int fmi = carry_mi, tmi = carry_mi;
#pragma unroll
        for (int v = 0; v < SPAN_THREADS / 64; ++v) {
            const int64_t ov = sh->mv[v];
            const int oi = sh->mi[v];
            if (v < wave && !span_min_before(fmv, fmi, ov, oi)) { fmv = ov; fmi = oi; }
            if (!span_min_before(tmv, tmi, ov, oi)) { tmv = ov; tmi = oi; }
        }
        if (!span_min_before(mv, mi, fmv, fmi)) { mv = fmv; mi = fmi; }
        if (in) {
            P[i] = excl;
            if (i == L - 1) P[L] = excl + w;
            pm[i] = mi;
            int l = brk;
            if (span_limited) {                                // first index in [l, i] whose position is within max_span of pos[i]
                const int64_t first = p_i - max_span;
                int a = l, b = i;
                while (a < b) { const int mid = (a + b) >> 1; if ((int64_t)pos[mid] < first) a = mid + 1; else b = mid; }
                l = a;
            }
            lo[i] = l;
            wide |= l > 0 && i + 1 - l > 64;
        }
        carry_sum = total; carry_brk = tbrk; carry_mv = tmv; carry_mi = tmi;
        // (no barrier: the next tile writes sh->sum / brk, which nobody reads behind the barrier above, and sh->mv / mi only
        // behind its own first barrier)
    }
    wide = __syncthreads_or(wide);                             // (also: P, lo, pm are complete)
    const int nblk = (L + 63) >> 6, nsup = (nblk + 63) >> 6;
    int32_t* smin = bmin + nblk;                               // (SUPER only: nblk + nsup <= L for every L >= 2)
    if (wide) {
        for (int blk = wave; blk < nblk; blk += SPAN_THREADS / 64) {
            const int p = blk * 64 + lane;
            int64_t v = p < L ? P[p] : INT64_MAX;
            int idx = p < L ? p : -1;
            span_wave_min(v, idx);
            if (lane == 0) bmin[blk] = idx;                    // (every block holds a row: idx >= 0)
        }
        __syncthreads();
        if constexpr (SUPER) {                                 // one minimum per 64 blocks, behind the block minima
            for (int sup = wave; sup < nsup; sup += SPAN_THREADS / 64) {
                const int blk = sup * 64 + lane;
                int idx = blk < nblk ? bmin[blk] : -1;
                int64_t v = idx >= 0 ? P[idx] : INT64_MAX;
                span_wave_min(v, idx);
                if (lane == 0) smin[sup] = idx;
            }
            __syncthreads();
        }
    }
    SpanCand best{0, 0x7fffffff, 0x7fffffff};                  // only positive masses come in front of it
    for (int b = tid; b < L; b += SPAN_THREADS) {
        const int l = lo[b];
        const int a = l == 0 ? pm[b] : span_range_min<SUPER>(P, bmin, smin, l, b + 1);
        const SpanCand c{P[b + 1] - P[a], b - a + 1, a};
        if (span_cand_before(c, best)) best = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        SpanCand c;
        c.s = __shfl_xor((long long)best.s, o); c.len = __shfl_xor(best.len, o); c.a = __shfl_xor(best.a, o);
        if (span_cand_before(c, best)) best = c;
    }
    if (lane == 0) { sh->cs[wave] = best.s; sh->cl[wave] = best.len; sh->ca[wave] = best.a; }
    __syncthreads();
    if (tid == 0)
        for (int v = 1; v < SPAN_THREADS / 64; ++v) {
            const SpanCand c{sh->cs[v], sh->cl[v], sh->ca[v]};
            if (span_cand_before(c, best)) best = c;
        }
    return best;
}

// thread 0 files the group's span for one query: the (D, label) order key (~0: none) and (a, b)
__device__ __forceinline__ void span_file(const SpanCand& c, int g, uint64_t* ekey, int32_t* ab) {
    const bool none = c.s <= 0;
    *ekey = none ? ~0ull : dist_key(span_rank_value(c.s), (uint32_t)g);
    ab[0] = none ? -1 : c.a;
    ab[1] = none ? -1 : c.a + c.len - 1;
}

// ---- LDS form: grid = (groups, queries of the chunk).  dynamic LDS: span_lds_bytes(alloc_rows).  Also files "none" for every
// group that is not allowed. ----
__global__ __launch_bounds__(SPAN_THREADS)
void span_lds_kernel(const float* __restrict__ dist, int64_t ld, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                     const int32_t* __restrict__ spos, int lds_rows, int alloc_rows, float tau, int64_t max_gap, int64_t max_span,
                     int n_groups, const uint32_t* __restrict__ allow, uint64_t* __restrict__ ekey /*[chunk][groups]*/,
                     int32_t* __restrict__ ab /*[chunk][groups][2]*/) {
    extern __shared__ __attribute__((aligned(16))) char span_smem[];
    __shared__ SpanShared sh;
    const int g = blockIdx.x, q = blockIdx.y;
    const int64_t slot = (int64_t)q * n_groups + g;
    if (allow && !group_allowed(allow, g)) {                   // whole workgroup leaves before any barrier
        if (threadIdx.x == 0) span_file(SpanCand{0, 0, 0}, g, ekey + slot, ab + 2 * slot);
        return;
    }
    const int b = goff[g], L = goff[g + 1] - b;
    if (L > lds_rows) return;                                  // the global form's
    if (L == 0) {                                              // (a label no row carries)
        if (threadIdx.x == 0) span_file(SpanCand{0, 0, 0}, g, ekey + slot, ab + 2 * slot);
        return;
    }
    int64_t* P = (int64_t*)span_smem;
    int32_t* pos = (int32_t*)(P + alloc_rows + 2);
    int32_t* lo = pos + alloc_rows;
    int32_t* pm = lo + alloc_rows;
    int32_t* bmin = pm + alloc_rows;
    for (int i = threadIdx.x; i < L; i += SPAN_THREADS) pos[i] = spos[b + i];
    __syncthreads();
    const SpanCand c = span_group<false>(pos, sorder + b, dist + (int64_t)q * ld, tau, max_gap, max_span, P, lo, pm, bmin, L, &sh);
    if (threadIdx.x == 0) span_file(c, g, ekey + slot, ab + 2 * slot);
}

// ---- global form: grid = groups; every allowed group above lds_rows, the chunk's queries one after the other.
// Work arrays at the group's offset: P [n + groups] int64 (L + 1 entries per group), lo | pm | minima [3][n] int32. ----
__global__ __launch_bounds__(SPAN_THREADS)
void span_global_kernel(const float* __restrict__ dist, int64_t ld, int chunk, const int32_t* __restrict__ goff,
                        const int32_t* __restrict__ sorder, const int32_t* __restrict__ spos, int lds_rows, float tau, int64_t max_gap,
                        int64_t max_span, int n_groups, const uint32_t* __restrict__ allow, int64_t* gP, int32_t* work, int64_t n,
                        uint64_t* __restrict__ ekey, int32_t* __restrict__ ab) {
    __shared__ SpanShared sh;
    const int g = blockIdx.x;
    if (allow && !group_allowed(allow, g)) return;
    const int b = goff[g], L = goff[g + 1] - b;
    if (L <= lds_rows) return;
    for (int q = 0; q < chunk; ++q) {
        const SpanCand c = span_group<true>(spos + b, sorder + b, dist + (int64_t)q * ld, tau, max_gap, max_span, gP + b + g, work + b,
                                            work + n + b, work + 2 * n + b, L, &sh);
        const int64_t slot = (int64_t)q * n_groups + g;
        if (threadIdx.x == 0) span_file(c, g, ekey + slot, ab + 2 * slot);
        __syncthreads();                                       // the arrays and sh are written again by the next query
    }
}

// ---- the k winners of the chunk's queries: grid = (k, queries of the chunk).  The mass is the sum of the span's gains again
// (integers: any order), the peak its smallest (d, tie).  mass / len / rows (each may be null) are the chunk's first query's. ----
__global__ __launch_bounds__(SPAN_THREADS)
void span_finish_kernel(const float* __restrict__ dist, int64_t ld, const int32_t* __restrict__ groups_out /*[chunk][k]*/, int k,
                        const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder, const int32_t* __restrict__ stie, float tau,
                        int n_groups, const int32_t* __restrict__ ab, int64_t* __restrict__ mass, int32_t* __restrict__ len,
                        int32_t* __restrict__ rows /*[chunk][k][3]*/) {
    __shared__ int64_t rs[SPAN_THREADS / 64];
    __shared__ uint64_t rk[SPAN_THREADS / 64];
    __shared__ int32_t ri[SPAN_THREADS / 64];
    const int j = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int64_t out = (int64_t)q * k + j;
    const int g = groups_out[out];
    if (g < 0) {
        if (tid == 0) {
            if (mass) mass[out] = 0;
            if (len) len[out] = 0;
            if (rows) { rows[3 * out] = -1; rows[3 * out + 1] = -1; rows[3 * out + 2] = -1; }
        }
        return;
    }
    const int base = goff[g];
    const int32_t* span = ab + 2 * ((int64_t)q * n_groups + g);
    const int a = span[0], b = span[1];
    const float* drow = dist + (int64_t)q * ld;
    int64_t s = 0;
    uint64_t key = ~0ull;
    int idx = -1;
    for (int i = a + tid; i <= b; i += SPAN_THREADS) {
        const float d = drow[sorder[base + i]];
        s += span_gain(tau, d);
        const uint64_t kk = dist_key(d, (uint32_t)stie[base + i]);
        if (kk < key) { key = kk; idx = i; }                   // (ties are distinct inside a group)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor((long long)s, o);
        const uint64_t ok = __shfl_xor((unsigned long long)key, o);
        const int oi = __shfl_xor(idx, o);
        if (ok < key) { key = ok; idx = oi; }
    }
    if ((tid & 63) == 0) { rs[tid >> 6] = s; rk[tid >> 6] = key; ri[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < SPAN_THREADS / 64; ++v) {
            s += rs[v];
            if (rk[v] < key) { key = rk[v]; idx = ri[v]; }
        }
        if (mass) mass[out] = s;
        if (len) len[out] = b - a + 1;
        if (rows) { rows[3 * out] = sorder[base + a]; rows[3 * out + 1] = sorder[base + b]; rows[3 * out + 2] = sorder[base + idx]; }
    }
}

// ---- the call's counters: (query, group) pairs that hold a span, summed over the chunks in stream order (first: the call's
// first chunk), and the two figures the host knows ----
__global__ __launch_bounds__(256)
void span_stats_kernel(const uint64_t* __restrict__ ekey, int64_t count, int first, unsigned long long global_groups,
                       unsigned long long chunks, unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long red[4];
    const int tid = threadIdx.x;
    unsigned long long c = 0;
    for (int64_t i = tid; i < count; i += 256) c += ekey[i] != ~0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        counters[0] = (first ? 0ull : counters[0]) + red[0] + red[1] + red[2] + red[3];
        counters[1] = global_groups;
        counters[2] = chunks;
    }
}

#endif  // __HIPCC__

}  // namespace vq
