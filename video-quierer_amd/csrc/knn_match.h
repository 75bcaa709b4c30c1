// Shared-footage search (vq_index_match_runs): the k GROUPS (videos) that reuse a run of a clip's frames, and where.
// include/vq_amd.h has the definition; DESIGN.md §4 "Shared footage".  Every other search reduces the [m][n] scores to a
// best row or a best sum; this one keeps ONE BIT of every score (distance <= max_dist) and looks for diagonal runs of bits
// along each group's (position, tie) order.
//
//   plan_match               host only: the path, the bit table, the exact path's query chunks, the tile path's geometry, the
//                            filed-pair capacity, the run key's field widths, the launches
//   match_threshold_kernel   exact path (mode 1, and the redo of a flagged call): d <= max_dist packed 32 rows to a word; the
//                            distances come from exact_dist_kernel's [chunk][n] table (FROM_DIST) or, in the redo, from the
//                            fp64 chain run in place
//   match_query_norm_kernel  tile path: e_i = E_i + MATCH_SLACK per query and the |q|^2 range test
//   match_tile_kernel        tile path: 256 queries x 2,048 rows per workgroup; every score classified sure hit / sure miss /
//                            filed; one whole bit word per (query, 32 rows) leaves by a plain store
//   match_patch_kernel       tile path: every filed pair decided by the exact chain, its bit set by an integer atomicOr
//   match_run_kernel         one thread per diagonal of every allowed group: the diagonal's best run -> the group's best run,
//                            a 64-bit integer atomicMin per (workgroup, group)
//   match_final_kernel       the group's (-hits, span, label) order key
//   (set_select_block_kernel / set_select_merge_kernel: the clip search's selection, unchanged)
//   match_score_kernel       the k winners: rows of the run's ends, and mean_dist by the exact chain over the hit cells
//   match_stats_kernel       the call's counters
//
// Bit table: bits[i][w], i = query, w = row >> 5, bit = row & 31, W = cdiv(n, 32) words per query.  Query-major because
// of who reads it: thread delta of match_run_kernel reads, at step i, the bit of row b_{i + delta}; the threads of a wave hold
// neighbouring delta, so at one step they read neighbouring entries of the (position, tie) order of ONE query — for a video stored
// as consecutive rows, one or two words.  Row-major ([r][m / 32]) would make the same 64 reads hit 64 different rows' words.
// It also suits the writer: the quadrant a wave finishes in the tile kernel is 64 queries x 32 rows, exactly one word per query.
//
// Tile path.  The workgroup and the workgroup order are set_group_max_kernel's (knn_set.h), the mainloop is the shared one
// (scan_stream256.h): queries on the A side, 2,048-row ranges of the fp16 matrix streamed past them in one continuous K loop.  A lane of
// wave (wr, wc) holds, for query m0 + 128 wr + 16 mi + (lane & 15), the scores of rows 64 wc + 16 ni + 4 (lane >> 4) + r of the
// row tile; a finished quadrant (hm, hn) is 4 query blocks x rows 64 wc + 32 hn .. + 31: the four lanes lane & 15 = const hold
// the 32 bits of one word between them, 8 each.  They are OR-ed across the four 16-lane rows by two permlane swaps and lane
// group (lane >> 4) = i stores the word of query block i: 64 word stores per wave and quadrant, no atomics, no [m][n] scores.
//
// Proof.  s = the real dot product, s16 = the fp16 score (fp32 accumulator), |s16 - s| <= E_i = scan_eps_unit(dim) * max|row|
// * |q_i| (knn_scan_f16.h; needs 0.25 <= |q_i|^2 <= 4 and near-unit rows, so |s| < 2.83 and |d| < 4).  The reported distance
// is d = fp32(1 - fp32(dot)), dot the fp64 chain: two roundings of at most 2^-23 each and the chain's own error (below 2^-40):
// |d - (1 - s)| <= 2^-22 + 2^-40.  T = 1 - max_dist is evaluated in fp64 on the host and rounded to fp32 (|T| < 4: error
// <= 2^-23; |T| >= 4 is at least 1.1 away from every score, and every distance is on the same side of max_dist).  The kernel
// computes x = fp32(s16 - T), relative error 2^-24, and compares it with e_i = fp32(E_i + MATCH_SLACK) (< 0.1, so x's rounding
// matters only below 2^-27 when |x| is near e_i; E_i's own fp32 evaluation is inside the 2 % scan_eps_unit carries).
//   x > e_i  =>  s - T_real > E_i + slack - E_i - 2^-23 - 2^-27 - 2^-27 >= 2^-22 + 2^-40 once slack >= 2^-21  =>  1 - s + (d's
//   error) < max_dist: a SURE HIT.  x < -e_i  =>  a SURE MISS by the mirror image.  MATCH_SLACK = 2^-19 (SET_SLACK's value).
//   Otherwise the pair is FILED and match_patch_kernel decides it by the chain itself.  Comparisons with max_dist are inclusive.
// A filed pair therefore has |s16 - T| <= e_i, so |(1 - d) - T| <= 2 E_i + slack + 2^-22: the band the list must hold.
// Not provable -> the call's flag goes to 2 and match_threshold_kernel<false> rewrites the WHOLE table exactly on the device:
// a query with |q|^2 outside [0.25, 4] or not finite (the tile kernel then leaves at once), or more filed pairs than the list
// holds (MATCH_FILED_CAP = 16M pairs of 8 B; the cursor is a 64-bit integer atomic, one per wave and quadrant that files
// anything; once the flag is up no wave touches the cursor again).  That redo runs one fp64 chain per cell: it is the bounded
// way out, not a path to plan for (DESIGN.md has its rate).
//
// Run pass.  Diagonals are numbered over the whole library: group g owns indices base(g) .. base(g + 1) - 1, base(g) =
// goff[g] + g (m - 1) (a group of L rows has L + m - 1 diagonals); a thread finds its group by a binary search over goff.  It
// walks its cells by ascending i carrying (hits, first, last, misses) and keeps the smallest key
//   ((m - hits) << (2 bm + bd)) | ((span - 1) << (bm + bd)) | ((delta + m - 1) << bm) | s
// bm = the bits of m - 1, bd = the bits of n + m - 2: 3 bm + bd <= 63 whenever the bit table is within its bound (m n <= 2^32),
// so ~0 is free to mean "no run".  Unsigned order of the key = the definition's (-hits, span, delta, s).  A workgroup whose 256
// diagonals belong to one group reduces first and issues one atomicMin; one that straddles groups issues one per thread that
// found a run.  Integer minima: the answer does not depend on the order in which anything runs.
//
// No floating-point atomics, no waiting of one workgroup on another, every loop bounded by the shapes.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "scan_stream256.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "knn_grouped.h"

#include <algorithm>

namespace vq {

constexpr int MATCH_MAX_M = 4096;                              // clip frames per call
constexpr int64_t MATCH_BITS_BYTES = (int64_t)512 << 20;       // the bit table's bound
constexpr int64_t MATCH_FILED_CAP = (int64_t)16 << 20;         // filed pairs (8 B each)
constexpr int64_t MATCH_DIST_WORDS = (int64_t)128 << 20;       // exact path: 512 MiB of fp32 distances per chunk
constexpr float MATCH_SLACK = 1.0f / 524288;                   // 2^-19 >= 2^-21 (derivation above)
constexpr int64_t MATCH_AUTO_MIN_ROWS = 16384;                 // mode 0 takes the tile path from this many rows (the plain search's bound) ...
// ... and clip frames.  Measured, not guessed (profiles/match_runs/probe.txt, 1M x 512): the exact path costs 0.059 ms per frame
// (3.77 ms at m = 64, 29.9 at 500, 240 at 4,096), the tile path 1.4 ms for any m up to 256: they cross near 24 frames
constexpr int MATCH_AUTO_MIN_M = 32;
constexpr int MATCH_RUN_THREADS = 256;
constexpr int MATCH_LDS_BYTES = G2_LDS_BYTES + SCAN2_QT * 4;   // the mainloop's buffers + the tile's 256 threshold half-widths

struct MatchPlan {
    int fp16;              // 1: the tile path answers the call
    int64_t words;         // bit words per query
    int64_t bits_bytes;    // the table; above MATCH_BITS_BYTES the call is refused
    int exact_chunk;       // exact path: queries per chunk of distances
    int exact_chunks;
    int64_t exact_bytes;   // its distance scratch
    int q_tiles;           // tile path: 256-query tiles, 2,048-row ranges, workgroups launched
    int ranges;
    int64_t tile_grid;
    int64_t filed_cap;     // pairs the filed list holds
    int key_m_bits;        // run key: bits of hits / span / s, and of the diagonal number
    int key_d_bits;
    int64_t diagonals;     // n + n_groups * (m - 1)
    int64_t run_blocks;
    int launches;          // kernels a call queues (memsets and copies not counted)
};

inline int match_bits_of(int64_t v) { int b = 0; while (v > 0) { ++b; v >>= 1; } return b; }

// near_unit: the index's rows are (knn_kernels.h row_norm_range_kernel); mode 2 is refused by the caller when !fp16 below.
// filed_cap_override > 0 (tests) lowers the capacity.
inline MatchPlan plan_match(int64_t n, int64_t n_groups, int dim, int m, int mode, bool near_unit, int64_t filed_cap_override) {
    MatchPlan p;
    const bool ok = scan_fp16_dim(dim) && near_unit && n >= 1;
    p.fp16 = (mode == 2 && ok) || (mode == 0 && ok && n >= MATCH_AUTO_MIN_ROWS && m >= MATCH_AUTO_MIN_M) ? 1 : 0;
    p.words = (std::max<int64_t>(n, 1) + 31) / 32;
    p.bits_bytes = (int64_t)m * p.words * 4;
    const int64_t ld = round_up(std::max<int64_t>(n, 1), 64);
    int64_t c = std::max<int64_t>(1, std::min<int64_t>(m, MATCH_DIST_WORDS / ld));
    if (c >= 32) c = c / 32 * 32;                              // whole 32-query tiles of exact_dist_kernel
    p.exact_chunk = (int)c;
    p.exact_chunks = cdiv(m, c);
    p.exact_bytes = c * ld * 4;
    p.q_tiles = cdiv(m, SCAN2_QT);
    p.ranges = cdiv(std::max<int64_t>(n, 1), SCAN2_RANGE);
    p.tile_grid = (int64_t)cdiv(p.ranges, 4) * cdiv(p.q_tiles, 8) * 32;
    p.filed_cap = filed_cap_override > 0 ? std::min(filed_cap_override, MATCH_FILED_CAP) : MATCH_FILED_CAP;
    p.key_m_bits = match_bits_of(m - 1);
    p.key_d_bits = std::max(1, match_bits_of(n + m - 2));
    p.diagonals = n + n_groups * (int64_t)(m - 1);
    p.run_blocks = (p.diagonals + MATCH_RUN_THREADS - 1) / MATCH_RUN_THREADS;
    // tile path: norms, fp16 queries, tile, patch, the gated redo; exact path: two per chunk; then run, final, two of the
    // selection, score, stats
    p.launches = (p.fp16 ? 5 : 2 * p.exact_chunks) + 6;
    return p;
}

#ifdef __HIPCC__

// control words of a call: the filed list's cursor (64-bit), then the flag
struct MatchCtl { unsigned long long cursor; int32_t flag; int32_t pad; };

// ---- exact path: hit bits of `cur` queries (grid.y) over all rows, 256 rows per workgroup, two words per wave.  bits /
// queries / dist: at the chunk's first query.  gate != null: only a call flagged 2 does anything. ----
template <bool FROM_DIST>
__global__ __launch_bounds__(256)
void match_threshold_kernel(const float* __restrict__ dist, int64_t ld, const float* __restrict__ rows, int64_t n, int dim,
                            const float* __restrict__ queries, float max_dist, uint32_t* __restrict__ bits, int64_t W,
                            const MatchCtl* __restrict__ gate) {
    if (gate && gate->flag != 2) return;
    const int i = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (r < n) {
        float d;
        if constexpr (FROM_DIST) d = dist[(int64_t)i * ld + r];
        else d = exact_row_dist(rows + (size_t)r * dim, queries + (size_t)i * dim, dim);
        hit = d <= max_dist;                                   // inclusive; a NaN distance never hits
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
    if (lane == 0) {
        const int64_t w = (r >> 5);                            // r is the wave's first row: a multiple of 64
        uint32_t* out = bits + (size_t)i * W;
        if (w < W) out[w] = (uint32_t)mask;
        if (w + 1 < W) out[w + 1] = (uint32_t)(mask >> 32);
    }
}

// ---- tile path: e_i = eps_rows |q_i| + MATCH_SLACK, and the |q|^2 range test: one wave per query ----
__global__ __launch_bounds__(64)
void match_query_norm_kernel(const float* __restrict__ queries, int dim, float eps_rows, float* __restrict__ qe /*[m]*/,
                             MatchCtl* __restrict__ ctl) {
    const int q = blockIdx.x;
    wave_query_norm2(queries + (size_t)q * dim, dim, [&](float s2, bool covered) {
        qe[q] = eps_rows * sqrtf(s2) + MATCH_SLACK;
        if (!covered) ctl->flag = 2;
    });
}

// OR across the four 16-lane rows of a wave (lane ^ 16, lane ^ 32), the result in every lane: rows4_sum's two swaps on bits
__device__ __forceinline__ uint32_t rows4_or(uint32_t x) {
    float a, b;
    rows_swap16(__builtin_bit_cast(float, x), a, b);
    x = __builtin_bit_cast(uint32_t, a) | __builtin_bit_cast(uint32_t, b);
    rows_swap32(__builtin_bit_cast(float, x), a, b);
    return __builtin_bit_cast(uint32_t, a) | __builtin_bit_cast(uint32_t, b);
}

// ---- tile path: hit bits of a 256-query tile over a 2,048-row range per workgroup (SCAN2_QT, SCAN2_RANGE: 8 row tiles, one
// continuous K loop: scan_stream256.h); the workgroup order is set_group_max_kernel's.  Q16 [q_tiles * 256][dim] (pad
// queries zero), X16 the index's fp16 copy (whole ranges allocated).  T = fp32(1 - max_dist), qe [nq_real]. ----
__global__ __launch_bounds__(G2_THREADS, 2)
void match_tile_kernel(const uint16_t* __restrict__ Q16, const uint16_t* __restrict__ X16, int dim, int64_t n, int q_tiles, int n_ranges,
                       int range_groups, int nq_real, float T, const float* __restrict__ qe, uint32_t* __restrict__ bits, int64_t W,
                       MatchCtl* __restrict__ ctl, unsigned long long* __restrict__ filed, unsigned long long cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int skip_s;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const Stream256Lane ln = stream256_lane();
    const int wr = ln.wr, wc = ln.wc, frow = ln.frow, fgrp = ln.fgrp;

    int range, qtile;
    if (!scan2_block_tile(range_groups, n_ranges, q_tiles, range, qtile)) return;   // whole workgroup leaves before any barrier
    const int m0 = qtile * SCAN2_QT;
    const int64_t n0 = (int64_t)range * SCAN2_RANGE;

    // the tile's 256 threshold half-widths e_i sit behind the mainloop's buffers (MATCH_LDS_BYTES): 8 registers per lane less
    float* const es = (float*)(smem + G2_LDS_BYTES);
    if (tid < SCAN2_QT) es[tid] = m0 + tid < nq_real ? qe[m0 + tid] : 0.f;
    // a call already flagged (a query outside the bound's range) is answered by the redo: one thread reads the flag, so the
    // whole workgroup leaves, or stays, together
    if (tid == 0) skip_s = __atomic_load_n(&ctl->flag, __ATOMIC_RELAXED);
    __syncthreads();
    if (skip_s == 2) return;

    const int qbase = m0 + wr * 128 + frow;              // the lane's query of block mi: qbase + 16 mi

    // the undecided cells of the lane's 8 scores of (query block mi, quadrant column hn): |score - T| <= e, the row exists
    auto undecided = [&](const f32x4 (&acc)[8][4], int mi, int hn, float ei, uint32_t live) __attribute__((always_inline)) -> uint32_t {
        uint32_t un = 0u;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = acc[mi][hn * 2 + j][r] - T;
                un |= (!(x > ei) && !(x < -ei) ? 1u : 0u) << (j * 16 + 4 * fgrp + r);
            }
        return qbase + 16 * mi < nq_real ? un & live : 0u;
    };
    // The undecided cells of a quadrant go to the filed list: one cursor atomic for the wave, then plain stores.  Entered by whole
    // waves (the caller's test is a ballot) and it contains no barrier of the mainloop.  Rare: it recomputes what it files.
    auto file = [&](const f32x4 (&acc)[8][4], int hm, int hn, int64_t rbase, uint32_t live) __attribute__((always_inline)) {
        const bool up = __atomic_load_n(&ctl->flag, __ATOMIC_RELAXED) == 2;
        if (__builtin_amdgcn_ballot_w64(up) != 0) return;      // the redo answers the call: leave the cursor alone
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) cnt += __builtin_popcount(undecided(acc, hm * 4 + i, hn, es[wr * 128 + frow + 16 * (hm * 4 + i)], live));
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int prev = __shfl_up(incl, o);
            if (lane >= o) incl += prev;
        }
        const int all = __shfl(incl, 63);
        unsigned long long base = 0ull;
        if (lane == 63) base = atomicAdd(&ctl->cursor, (unsigned long long)all);
        base = __shfl(base, 63);
        if (lane == 63 && base + (unsigned long long)all > cap) __atomic_store_n(&ctl->flag, 2, __ATOMIC_RELAXED);   // the list overflows
        unsigned long long at = base + (unsigned long long)(incl - cnt);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mi = hm * 4 + i;
            uint32_t u = undecided(acc, mi, hn, es[wr * 128 + frow + 16 * mi], live);
            const unsigned long long q = (unsigned long long)(qbase + 16 * mi);
            while (u) {
                const int bp = __builtin_ctz(u);
                u &= u - 1u;
                if (at < cap) filed[at] = (q << 32) | (unsigned long long)(uint32_t)(rbase + bp);
                ++at;
            }
        }
    };
    // Classify quadrant (hm, hn) of row tile t, store its 64 words, file what is undecided, and clear it.
    auto fold = [&](f32x4 (&acc)[8][4], int hm, int hn, int t) __attribute__((always_inline)) {
        const int64_t rbase = n0 + (int64_t)t * 256 + wc * 64 + hn * 32;       // first row of the wave's word (wave-uniform)
        const int64_t left = n - rbase;                                        // rows of it that exist
        const uint32_t live = left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
        uint32_t mine = 0u, any = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mi = hm * 4 + i;
            const float ei = es[wr * 128 + frow + 16 * mi];
            uint32_t sure = 0u;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sure |= (acc[mi][hn * 2 + j][r] - T > ei ? 1u : 0u) << (j * 16 + 4 * fgrp + r);
            const uint32_t word = rows4_or(qbase + 16 * mi < nq_real ? sure & live : 0u);
            mine = fgrp == i ? word : mine;                                    // lane group i stores the word of query block i
            any |= undecided(acc, mi, hn, ei, live);
        }
        const int q = qbase + 16 * (hm * 4 + fgrp);
        const int64_t w = rbase >> 5;
        if (q < nq_real && w < W) bits[(size_t)q * W + w] = mine;
        if (__builtin_amdgcn_ballot_w64(any != 0u) != 0) file(acc, hm, hn, rbase, live);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[hm * 4 + i][hn * 2] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc[hm * 4 + i][hn * 2 + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    // (the stores and the rare atomic sit ahead of the mainloop's counted wait: scan_stream256.h says why that is safe)
    stream256_run(smem, ln, Q16 + (size_t)m0 * dim, X16 + (size_t)n0 * dim, dim, 8, fold);
}

// ---- tile path: every filed pair by the exact chain; a hit sets its bit.  One lane per pair: a chain is one fixed-order sum. ----
__global__ __launch_bounds__(256)
void match_patch_kernel(const float* __restrict__ rows, int dim, const float* __restrict__ queries, float max_dist,
                        const MatchCtl* __restrict__ ctl, const unsigned long long* __restrict__ filed, unsigned long long cap,
                        uint32_t* __restrict__ bits, int64_t W) {
    if (ctl->flag != 0) return;
    const unsigned long long count = ctl->cursor < cap ? ctl->cursor : cap;
    for (unsigned long long p = (unsigned long long)blockIdx.x * 256 + threadIdx.x; p < count; p += (unsigned long long)gridDim.x * 256) {
        const unsigned long long pair = filed[p];
        const uint32_t i = (uint32_t)(pair >> 32), r = (uint32_t)pair;
        const float d = exact_row_dist(rows + (size_t)r * dim, queries + (size_t)i * dim, dim);
        if (d <= max_dist) atomicOr(bits + (size_t)i * W + (r >> 5), 1u << (r & 31));
    }
}

// ---- run pass ----
struct MatchKey { int bm, bd; };                       // field widths (plan_match)
__device__ __forceinline__ uint64_t match_key(const MatchKey f, int m, int hits, int span, int64_t doff, int s) {
    return ((((((uint64_t)(m - hits) << f.bm) | (uint64_t)(span - 1)) << f.bd) | (uint64_t)doff) << f.bm) | (uint64_t)s;
}
__device__ __forceinline__ void match_unkey(const MatchKey f, int m, uint64_t key, int& hits, int& span, int64_t& doff, int& s) {
    const uint64_t mm = (1ull << f.bm) - 1ull, md = (1ull << f.bd) - 1ull;
    s = (int)(key & mm);
    doff = (int64_t)((key >> f.bm) & md);
    span = (int)((key >> (f.bm + f.bd)) & mm) + 1;
    hits = m - (int)(key >> (2 * f.bm + f.bd));
}

// thread = diagonal number t of the whole library (header comment); gkey [G] starts at ~0
__global__ __launch_bounds__(MATCH_RUN_THREADS)
void match_run_kernel(const uint32_t* __restrict__ bits, int64_t W, int m, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                      int n_groups, int64_t diagonals, int min_len, int max_miss, const MatchKey f, const uint32_t* __restrict__ allow,
                      unsigned long long* __restrict__ gkey) {
    __shared__ uint64_t red[4];
    __shared__ int ends[2];
    const int tid = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * MATCH_RUN_THREADS + tid;
    int g = -1;
    uint64_t best = ~0ull;
    int i0 = 1, i1 = 0;                                         // the thread's cells i0 .. i1 (none: a disallowed group, past the end)
    int64_t doff = 0;
    const int32_t* ord = sorder;                                // ord[i] = row b_{i + delta}
    if (t < diagonals) {
        int lo = 0, hi = n_groups;                              // the first group whose base is above t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)goff[mid] + (int64_t)mid * (m - 1) > t) hi = mid; else lo = mid + 1;
        }
        g = lo - 1;
        if (!allow || group_allowed(allow, g)) {
            const int b = goff[g], L = goff[g + 1] - b;
            doff = t - ((int64_t)b + (int64_t)g * (m - 1));
            const int64_t delta = doff - (m - 1), past = (int64_t)L - 1 - delta;      // past: the last i whose row exists
            i0 = delta < 0 ? (int)-delta : 0;
            i1 = past < m - 1 ? (int)past : m - 1;
            ord = sorder + b + delta;
        }
    }
    // The lanes of a wave step through the SAME query i together, each inside its own i0 .. i1: at one step they read the bits of
    // neighbouring rows of one query (a word or two).  Stepping each lane from its own i0 makes the 64 reads of a step hit 64
    // different queries' words wherever delta < 0: measured 57.7 ms against 6.8 ms this way for 4,096 x 1M.
    int wlo = i0 <= i1 ? i0 : 0x7fffffff, whi = i0 <= i1 ? i1 : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, o));
        whi = max(whi, __shfl_xor(whi, o));
    }
    int hits = 0, first = -1, last = -1, misses = 0;
    auto close = [&]() {
        if (first >= 0 && hits >= min_len) {
            const uint64_t key = match_key(f, m, hits, last - first + 1, doff, first);
            best = key < best ? key : best;
        }
        first = -1; hits = 0;
    };
#pragma unroll 4
    for (int i = wlo; i <= whi; ++i) {
        const bool in = i >= i0 && i <= i1;
        bool hit = false;
        if (in) {
            const uint32_t r = (uint32_t)ord[i];
            hit = (bits[(size_t)i * W + (r >> 5)] >> (r & 31)) & 1u;
        }
        if (hit) {
            if (first < 0) first = i;
            ++hits; last = i; misses = 0;
        } else if (in && first >= 0 && ++misses > max_miss) {
            close();
        }
    }
    close();
    if (tid == 0) ends[0] = g;
    if (tid == MATCH_RUN_THREADS - 1) ends[1] = g;
    __syncthreads();
    if (ends[0] == ends[1] && ends[0] >= 0) {                   // block-uniform: one group -> one atomic
        best = block_min_u64(best, red, tid);
        if (tid == 0 && best != ~0ull) atomicMin(gkey + g, (unsigned long long)best);
    } else if (best != ~0ull) {
        atomicMin(gkey + g, (unsigned long long)best);
    }
}

// ---- ekey[g] = the order key of (-hits, span, label): the run key's two leading fields above the label (~0: no run) ----
__global__ __launch_bounds__(256)
void match_final_kernel(const unsigned long long* __restrict__ gkey, int n_groups, const MatchKey f, uint64_t* __restrict__ ekey) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const uint64_t key = gkey[g];
    ekey[g] = key == ~0ull ? ~0ull : ((key >> (f.bm + f.bd)) << 32) | (uint32_t)g;
}

// ---- the k winners: one workgroup per slot.  The run's cells by the exact chain, then thread 0 adds the hit cells' distances
// in ascending i in fp64. ----
__global__ __launch_bounds__(256)
void match_score_kernel(const int32_t* __restrict__ groups_out, const unsigned long long* __restrict__ gkey, const MatchKey f, int m,
                        const uint32_t* __restrict__ bits, int64_t W, const float* __restrict__ rows, int dim,
                        const float* __restrict__ queries, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                        int32_t* __restrict__ hits_out, int32_t* __restrict__ span_out, int32_t* __restrict__ qfirst_out,
                        int32_t* __restrict__ rfirst_out, int32_t* __restrict__ rlast_out, float* __restrict__ mean_out) {
    __shared__ float cell[MATCH_MAX_M];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int g = groups_out[j];
    if (g < 0) {
        if (tid == 0) {
            hits_out[j] = 0; span_out[j] = 0; qfirst_out[j] = -1; rfirst_out[j] = -1; rlast_out[j] = -1;
            mean_out[j] = __builtin_inff();
        }
        return;
    }
    int hits, span, s;
    int64_t doff;
    match_unkey(f, m, gkey[g], hits, span, doff, s);
    const int32_t* ord = sorder + goff[g] + (doff - (m - 1));
    for (int c = tid; c < span; c += 256) {
        const int i = s + c;
        const uint32_t r = (uint32_t)ord[i];
        const bool hit = (bits[(size_t)i * W + (r >> 5)] >> (r & 31)) & 1u;
        cell[c] = hit ? exact_row_dist(rows + (size_t)r * dim, queries + (size_t)i * dim, dim) : __builtin_nanf("");
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int c = 0; c < span; ++c) {
            const float d = cell[c];
            if (d == d) sum += (double)d;                       // a hit's distance is never NaN
        }
        hits_out[j] = hits; span_out[j] = span; qfirst_out[j] = s;
        rfirst_out[j] = ord[s]; rlast_out[j] = ord[s + span - 1];
        mean_out[j] = (float)(sum / (double)hits);
    }
}

// ---- the call's counters: groups with a run, pairs filed (a flagged call: 0), the flag.  forced: the host form saw a query
// outside the bound's range and took the chunked exact path instead of the tile path: reported as the flag it stands for. ----
__global__ __launch_bounds__(256)
void match_stats_kernel(const uint64_t* __restrict__ ekey, int n_groups, const MatchCtl* __restrict__ ctl, unsigned long long cap,
                        int forced, unsigned long long* __restrict__ counters) {
    __shared__ int red[4];
    const int tid = threadIdx.x;
    int c = 0;
    for (int g = tid; g < n_groups; g += 256) c += ekey[g] != ~0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        const int flag = forced ? 2 : ctl->flag;
        counters[0] = (unsigned long long)(red[0] + red[1] + red[2] + red[3]);
        counters[1] = flag ? 0ull : (ctl->cursor < cap ? ctl->cursor : cap);
        counters[2] = (unsigned long long)flag;
    }
}

#endif  // __HIPCC__

}  // namespace vq
