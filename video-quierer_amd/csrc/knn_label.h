// Zero-shot labelling (vq_index_label_rows): per ROW the prompt it shows best, per GROUP (video) the tags its rows vote for.
// include/vq_amd.h has the definition; DESIGN.md §4 "Zero-shot labelling".  Every other search reduces along the row axis per
// query; this one reduces along the prompt axis per row.
//
//   plan_label                 host only: which path a call takes, the exact path's prompt chunks, the tile path's geometry
//                              and scratch, the error bound a caller may rely on
//   label_colmin_kernel        exact path: the running (distance, prompt) key of every row over one chunk of distances
//   label_prompt_norm_kernel   tile path: the largest |p|^2 and the |p|^2 range test (one wave per prompt)
//   label_tile_kernel          tile path: 256 rows x up to 2,048 prompts per workgroup, the three largest keys of every row
//   label_finalize_kernel      tile path: proven label / exact re-score of two prompts / filed for the redo, per row
//   label_redo_kernel          tile path: filed rows (or, for a flagged call, all rows) over ALL prompts, exactly
//   label_group_kernel         votes, the m tags and their show rows of one group per workgroup (groups up to 4,096 rows)
//   label_piece_hist_kernel .. label_long_show_kernel   the same for longer groups, split into pieces over workgroups
//
// Exact path (mode 1): per chunk of prompts, in order, exact_dist_kernel writes [chunk][n] distances (the chunk is sized so
// that they stay within 512 MiB) and label_colmin_kernel folds the chunk's columns into run[r], the smallest 64-bit
// (distance, prompt) key of row r so far: dist_key's order is (distance ascending, prompt ascending), the definition's.
//
// Tile path (mode 2): the ROWS take the place the queries have in set_group_max_kernel (knn_set.h) and the PROMPTS the place
// of its streamed rows: a workgroup holds one 256-row tile of the fp16 matrix and streams up to eight 256-prompt tiles past it
// through the same streamed mainloop (scan_stream256.h), one continuous K loop.  Wave (wr, wc) owns rows 128 wr .. +127
// and prompts 64 wc .. +63 of every prompt tile; a lane holds, for each of its 8 rows, scores of 16 prompts per tile.  So the
// reduction over the prompt axis runs along the lane's own registers, tile after tile, and needs no exchange until the range
// is done: per row the lane keeps k1 >= k2 >= f, the three largest keys it has seen.  A key is the order-preserving word of
// the fp32 score (score_key) with the lane-local prompt index (t * 16 + ni * 4 + r, 7 bits, inverted) in its low 7 bits; pad
// prompts get key 0, below every score.  After the last tile every lane writes its keys, with the two prompt numbers spelled
// out, to LDS (the mainloop's buffers are free by then); thread R < 256 merges the 16 (wc, lane group) parts of row R in part
// order and stores (k1, j1, k2, j2, f) for (prompt range, row): 20 B per row and range, P <= 4,096 makes at most two ranges.
// The [P][n] score table never exists; the matrix is read once per range of 2,048 prompts (the 256-row tile's K-tiles are
// re-staged per prompt tile, from L2).
//
// Proof.  E = scan_eps_unit(dim) * max|row| * max_j |p_j| bounds |decoded key - exact score| for every (row, prompt) (knn_scan_f16.h
// derives it; its 2^-16 term covers the 7 index bits packed here exactly as in the scans: 128 ulp of a score are at most
// 2^-16 of it).  Decoding clears the index bits.  Per row let K1 >= K2 >= F be its three largest decoded keys over ALL
// prompts (the top three of a union are among the parts' top threes), J1, J2 the prompts of the first two, and
// T = 2 E + LABEL_SLACK.
//   (a) K1 - K2 > T (or there is no second prompt).  Every j != J1 has s(j) <= K2 + E < K1 - E - LABEL_SLACK <= s(J1) - LABEL_SLACK.
//       A reported distance is fp32(1 - fp32(dot)): within 2^-23 + 2^-23 of 1 - s (|dot| < 4).  Scores more than 2^-21 apart
//       therefore give strictly ordered distances, LABEL_SLACK = 2^-19 leaves room for the fp32 evaluation of T and of the
//       difference (two roundings of <= 2^-23 each, and E's own evaluation inside the 2 % scan_eps_unit carries).  So
//       d(r, J1) < d(r, j) for every other j: L(r) = J1 whatever the indices, and best(r) is ONE exact fp64-chain dot.
//   (b) else K1 - F > T (or there is no third prompt).  By the same argument every prompt other than J1, J2 has a strictly
//       larger distance than J1; the floor F bounds all of them, so the list {J1, J2} is complete.  Both are re-scored by the
//       exact chain; the smaller (distance, prompt) wins.
//   (c) else the row is filed: label_redo_kernel scores it against all prompts exactly, one wave per filed row.
//   A prompt with |p|^2 outside [0.25, 4] (or not finite) breaks E's premises (knn_scan_f16.h): the call's flag goes to 2,
//   label_finalize_kernel leaves, and the redo answers every row.  The host form tests the norms before it queues anything and
//   takes the chunked exact path instead, which is far faster at that size: the redo runs about 3.9e9 exact dots per second
//   at dim 512 (25,486 filed rows x 4,096 prompts in ~27 ms), so a flagged device call of 1M rows x 4,096 prompts takes about
//   a second where the chunked path takes 0.25 s.
// Stats: rows of (a), (b), (c); a flagged call reports (0, 0, n).
//
// Groups: a group of at most 4,096 rows is one workgroup (label_group_kernel) that walks its by-group row list twice.
// Sweep 1: an LDS histogram of the labels (at most 4,096 counters) and the unlabelled count.  Then m rounds of "largest
// (votes, inverted label)" over the histogram, each winner's counter cleared.  Sweep 2: for the m chosen labels the smallest
// (best, tie) key among the group's rows that carry them (64-bit LDS minima).  A longer group takes the split form: the host cuts
// its row list into pieces of 4,096 entries; label_piece_hist_kernel (a workgroup per piece) writes the piece's histogram,
// label_long_select_kernel (a workgroup per long group) adds its pieces' histograms in piece order and runs the rounds,
// label_piece_show_kernel takes each piece's show keys for the chosen labels, label_long_show_kernel merges them in piece
// order.  The pieces' histograms are the only table: P counters per 4,096 rows of a LONG group, at most 4 B per such row; no
// [G][P] table goes to global memory.  Integer sums and minima: the answer does not depend on which form ran.
//
// Stores are plain vector stores; global atomics: the counters, the filed-row list's cursor, the largest |p|^2.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "scan_stream256.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "knn_grouped.h"

#include <algorithm>

namespace vq {

constexpr int LABEL_MAX_P = 4096;                    // prompts per call (= the group kernel's LDS counters)
constexpr int LABEL_MAX_M = 16;                      // tags per group
constexpr int LABEL_PT = 256;                        // prompts per tile of the tile path
constexpr int LABEL_RANGE_TILES = 8;                 // prompt tiles a workgroup streams
constexpr int LABEL_ROW_TILE = 256;                  // rows per workgroup
constexpr int64_t LABEL_AUTO_MIN_ROWS = 16384;       // mode 0 takes the tile path from this many rows (the plain search's bound) ...
constexpr int64_t LABEL_AUTO_MIN_WORK = (int64_t)1 << 22;  // ... and n x P scores: the measured crossover (profiles/label_rows/probe.txt)
constexpr int64_t LABEL_DIST_WORDS = (int64_t)128 << 20;   // exact path: 512 MiB of fp32 distances per chunk
constexpr float LABEL_SLACK = 1.0f / 524288;         // 2^-19 (derivation above)
constexpr int LABEL_GROUP_SPLIT_ROWS = 4096;            // groups above this many rows are split over workgroups ...
constexpr int LABEL_GROUP_PIECE_ROWS = 4096;            // ... in pieces of this many rows (16 rows per thread and sweep)
constexpr int LABEL_PART_WORDS = 5;                  // k1, j1, k2, j2, f
constexpr int LABEL_PART_STRIDE = LABEL_PART_WORDS * LABEL_ROW_TILE + 16;     // words per part in LDS (+16: parts on different banks)
constexpr int LABEL_LDS_BYTES = G2_LDS_BYTES;        // the merge (16 parts, 82,944 B) reuses the mainloop's buffers
static_assert(16 * LABEL_PART_STRIDE * 4 <= G2_LDS_BYTES, "the merge parts fit the mainloop's LDS");
static_assert(LABEL_RANGE_TILES * 16 <= 128, "the lane-local prompt index fits 7 bits");

struct LabelPlan {
    int fp16;             // 1: the tile path answers the call
    int exact_chunk;      // exact path: prompts per chunk of distances (whole call, or the host form's flagged redo)
    int exact_chunks;
    int64_t exact_bytes;  // its distance scratch
    int prompt_tiles;     // tile path: 256-prompt tiles, ranges of up to 8 of them, 256-row tiles, the parts' bytes
    int prompt_ranges;
    int64_t row_tiles;
    int64_t part_bytes;
    float eps;            // unit rows and prompts whose best and second exact scores differ by more than 4 eps are proven
    int group_split_rows; // groups of more rows than this take the split form ...
    int group_piece_rows; // ... in pieces of this many entries of the by-group row list
    int64_t largest_group_pieces;   // pieces of the longest group (0: it runs as one workgroup)
};

// near_unit: the index's rows are (knn_kernels.h row_norm_range_kernel); mode 2 is refused by the caller when !fp16 below.
inline LabelPlan plan_label(int64_t n, int dim, int P, int mode, bool near_unit, int64_t largest_group) {
    LabelPlan p;
    const bool ok = scan_fp16_dim(dim) && near_unit && n >= 1;
    p.fp16 = (mode == 2 && ok) || (mode == 0 && ok && n >= LABEL_AUTO_MIN_ROWS && n * P >= LABEL_AUTO_MIN_WORK) ? 1 : 0;
    const int64_t ld = round_up(std::max<int64_t>(n, 1), 64);
    int64_t c = std::max<int64_t>(1, std::min<int64_t>(P, LABEL_DIST_WORDS / ld));
    if (c >= 32) c = c / 32 * 32;                                   // whole 32-query tiles of exact_dist_kernel
    p.exact_chunk = (int)c;
    p.exact_chunks = cdiv(P, c);
    p.exact_bytes = c * ld * 4;
    p.prompt_tiles = cdiv(P, LABEL_PT);
    p.prompt_ranges = cdiv(p.prompt_tiles, LABEL_RANGE_TILES);
    p.row_tiles = (n + LABEL_ROW_TILE - 1) / LABEL_ROW_TILE;
    p.part_bytes = (int64_t)p.prompt_ranges * LABEL_PART_WORDS * p.row_tiles * LABEL_ROW_TILE * 4;
    // the bound for |row| <= 1.0001 (what normalised rows measure) and |p| <= 1.0001, with the slack's half
    p.eps = scan_fp16_dim(dim) ? scan_eps_unit(dim) * 1.0001f * 1.0001f + 0.5f * LABEL_SLACK : 0.f;
    p.group_split_rows = LABEL_GROUP_SPLIT_ROWS;
    p.group_piece_rows = LABEL_GROUP_PIECE_ROWS;
    p.largest_group_pieces = largest_group > LABEL_GROUP_SPLIT_ROWS ? (largest_group + LABEL_GROUP_PIECE_ROWS - 1) / LABEL_GROUP_PIECE_ROWS : 0;
    return p;
}

#ifdef __HIPCC__

// ---- exact path: run[r] = min(run[r], (dist[i][r], j0 + i)) over the chunk's i; the last chunk also writes the answer ----
__global__ __launch_bounds__(256)
void label_colmin_kernel(const float* __restrict__ dist, int64_t ld, int64_t n, int cur, int j0, int first, int last, float max_dist,
                         uint64_t* __restrict__ run /*[n]*/, int32_t* __restrict__ lab, float* __restrict__ best) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        uint64_t key = first ? ~0ull : run[r];
        for (int i = 0; i < cur; ++i) {
            const uint64_t k = dist_key(dist[(int64_t)i * ld + r], (uint32_t)(j0 + i));
            key = k < key ? k : key;
        }
        if (last) {
            const float d = key_dist(key);
            lab[r] = d > max_dist ? -1 : (int32_t)(uint32_t)key;
            best[r] = d;
        } else {
            run[r] = key;
        }
    }
}

// ---- tile path: ctl = {filed rows, flag, bits of the largest |p|^2} (zeroed by the caller); one wave per prompt ----
__global__ __launch_bounds__(64)
void label_prompt_norm_kernel(const float* __restrict__ prompts, int dim, int32_t* __restrict__ ctl) {
    const int j = blockIdx.x;
    wave_query_norm2(prompts + (size_t)j * dim, dim, [&](float s2, bool covered) {
        if (!covered) ctl[1] = 2;
        else atomicMax((uint32_t*)ctl + 2, __builtin_bit_cast(uint32_t, s2));   // positive floats order like their bits
    });
}

__device__ __forceinline__ float label_key_score(uint32_t key) { return key_score(key & ~127u); }

// insert (key, j) / a floor into the running (K1, J1, K2, J2, F); key 0 = nothing
__device__ __forceinline__ void label_insert(uint32_t key, int32_t j, uint32_t& K1, int32_t& J1, uint32_t& K2, int32_t& J2, uint32_t& F) {
    if (key > K1) { F = K2; K2 = K1; J2 = J1; K1 = key; J1 = j; }
    else if (key > K2) { F = K2; K2 = key; J2 = j; }
    else if (key > F) F = key;
}

// ---- tile path: X16 [row tiles * 256][dim] (the index's fp16 copy), P16 [p_tiles * 256][dim] (pad prompts zero).  Grid:
// row_tiles * p_ranges workgroups, range fastest.  parts [p_ranges][5][n_pad], n_pad = row tiles * 256. ----
__global__ __launch_bounds__(G2_THREADS, 2)
void label_tile_kernel(const uint16_t* __restrict__ X16, const uint16_t* __restrict__ P16, int dim, int P, int p_tiles, int p_ranges,
                       int64_t n_pad, uint32_t* __restrict__ parts) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const Stream256Lane ln = stream256_lane();
    const int wr = ln.wr, wc = ln.wc, frow = ln.frow, fgrp = ln.fgrp;

    const int64_t rtile = blockIdx.x / p_ranges;
    const int range = blockIdx.x - (int)rtile * p_ranges;
    const int64_t m0 = rtile * LABEL_ROW_TILE;                       // first row
    const int j00 = range * (LABEL_RANGE_TILES * LABEL_PT);          // first prompt
    const int nt = min(LABEL_RANGE_TILES, p_tiles - range * LABEL_RANGE_TILES);   // prompt tiles of this range (>= 1)

    uint32_t k1[8], k2[8], fl[8];                        // per row block mi: the lane's three largest keys so far
#pragma unroll
    for (int i = 0; i < 8; ++i) { k1[i] = 0u; k2[i] = 0u; fl[i] = 0u; }
    const int jlane = j00 + wc * 64 + 4 * fgrp;          // the lane's prompt of (t, ni, r): jlane + t * 256 + ni * 16 + r

    // Fold quadrant (hm, hn) of prompt tile t into the rows' running keys and clear it.
    auto fold = [&](f32x4 (&acc)[8][4], int hm, int hn, int t) __attribute__((always_inline)) {
        const bool ragged = j00 + (t + 1) * LABEL_PT > P;             // uniform: the tile holds pad prompts
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mi = hm * 4 + i;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ni = hn * 2 + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    uint32_t key = (score_key(acc[mi][ni][r]) & ~127u) | (uint32_t)(127 - (t * 16 + ni * 4 + r));
                    if (ragged && jlane + t * LABEL_PT + ni * 16 + r >= P) key = 0u;
                    const uint32_t lo = min(k1[mi], key);
                    k1[mi] = max(k1[mi], key);
                    const uint32_t lo2 = min(k2[mi], lo);
                    k2[mi] = max(k2[mi], lo);
                    fl[mi] = max(fl[mi], lo2);
                }
                acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    stream256_run(smem, ln, X16 + (size_t)m0 * dim, P16 + (size_t)j00 * dim, dim, nt, fold);

    // ---- merge: behind this barrier every wave is past its last LDS read; every LDS-DMA has landed (scan_stream256.h) ----
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    uint32_t* const lw = (uint32_t*)smem;
    {
        uint32_t* part = lw + (wc * 4 + fgrp) * LABEL_PART_STRIDE + wr * 128 + frow;
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const int l1 = 127 - (int)(k1[mi] & 127u), l2 = 127 - (int)(k2[mi] & 127u);
            uint32_t* o = part + mi * 16;
            o[0 * LABEL_ROW_TILE] = k1[mi];
            o[1 * LABEL_ROW_TILE] = (uint32_t)(jlane + (l1 >> 4) * LABEL_PT + ((l1 >> 2) & 3) * 16 + (l1 & 3));
            o[2 * LABEL_ROW_TILE] = k2[mi];
            o[3 * LABEL_ROW_TILE] = (uint32_t)(jlane + (l2 >> 4) * LABEL_PT + ((l2 >> 2) & 3) * 16 + (l2 & 3));
            o[4 * LABEL_ROW_TILE] = fl[mi];
        }
    }
    __syncthreads();
    if (tid < LABEL_ROW_TILE) {
        uint32_t K1 = 0u, K2 = 0u, F = 0u;
        int32_t J1 = -1, J2 = -1;
        for (int p = 0; p < 16; ++p) {
            const uint32_t* in = lw + p * LABEL_PART_STRIDE + tid;
            label_insert(in[0 * LABEL_ROW_TILE], (int32_t)in[1 * LABEL_ROW_TILE], K1, J1, K2, J2, F);
            label_insert(in[2 * LABEL_ROW_TILE], (int32_t)in[3 * LABEL_ROW_TILE], K1, J1, K2, J2, F);
            F = max(F, in[4 * LABEL_ROW_TILE]);
        }
        uint32_t* out = parts + (size_t)range * LABEL_PART_WORDS * n_pad + m0 + tid;
        out[0 * n_pad] = K1; out[1 * n_pad] = (uint32_t)J1; out[2 * n_pad] = K2; out[3 * n_pad] = (uint32_t)J2; out[4 * n_pad] = F;
    }
}

// ---- tile path: per row, the ranges' parts in order -> proven / re-scored / filed.  counters {proven, re-scored, filed}. ----
__global__ __launch_bounds__(256)
void label_finalize_kernel(const uint32_t* __restrict__ parts, int p_ranges, int64_t n_pad, int64_t n, const float* __restrict__ rows, int dim,
                           const float* __restrict__ prompts, float eps_rows, float max_dist, int32_t* __restrict__ ctl,
                           int32_t* __restrict__ filed /*[n]*/, int32_t* __restrict__ lab, float* __restrict__ best,
                           unsigned long long* __restrict__ counters) {
    if (ctl[1] != 0) return;                                 // a prompt outside the bound's range: the redo answers every row
    const float T = 2.0f * (eps_rows * sqrtf(__builtin_bit_cast(float, (uint32_t)ctl[2]))) + LABEL_SLACK;
    const int lane = threadIdx.x & 63;
    for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < n; r0 += (int64_t)gridDim.x * 256) {    // block-uniform trip count
        const int64_t r = r0 + threadIdx.x;
        int state = -1;
        if (r < n) {
            uint32_t K1 = 0u, K2 = 0u, F = 0u;
            int32_t J1 = -1, J2 = -1;
            for (int g = 0; g < p_ranges; ++g) {
                const uint32_t* in = parts + (size_t)g * LABEL_PART_WORDS * n_pad + r;
                label_insert(in[0 * n_pad], (int32_t)in[1 * n_pad], K1, J1, K2, J2, F);
                label_insert(in[2 * n_pad], (int32_t)in[3 * n_pad], K1, J1, K2, J2, F);
                F = max(F, in[4 * n_pad]);
            }
            const float s1 = label_key_score(K1);
            const float* rv = rows + (size_t)r * dim;
            if (K2 == 0u || s1 - label_key_score(K2) > T) {
                const float d = exact_row_dist(rv, prompts + (size_t)J1 * dim, dim);
                lab[r] = d > max_dist ? -1 : J1;
                best[r] = d;
                state = 0;
            } else if (F == 0u || s1 - label_key_score(F) > T) {
                const float d1 = exact_row_dist(rv, prompts + (size_t)J1 * dim, dim);
                const float d2 = exact_row_dist(rv, prompts + (size_t)J2 * dim, dim);
                const bool second = dist_key(d2, (uint32_t)J2) < dist_key(d1, (uint32_t)J1);
                const float d = second ? d2 : d1;
                lab[r] = d > max_dist ? -1 : (second ? J2 : J1);
                best[r] = d;
                state = 1;
            } else {
                filed[atomicAdd(ctl, 1)] = (int32_t)r;
                state = 2;
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const unsigned long long votes = __builtin_amdgcn_ballot_w64(state == s);
            if (lane == 0 && votes) atomicAdd(counters + s, (unsigned long long)__builtin_popcountll(votes));
        }
    }
}

// ---- tile path: one wave per filed row (flag 2: per row of the index) against all prompts by the exact chain ----
__global__ __launch_bounds__(256)
void label_redo_kernel(const float* __restrict__ rows, int64_t n, int dim, const float* __restrict__ prompts, int P, float max_dist,
                       const int32_t* __restrict__ ctl, const int32_t* __restrict__ filed, int32_t* __restrict__ lab,
                       float* __restrict__ best, unsigned long long* __restrict__ counters) {
    const bool all = ctl[1] != 0;
    const int64_t count = all ? n : (int64_t)ctl[0];
    const int lane = threadIdx.x & 63;
    if (all && blockIdx.x == 0 && threadIdx.x == 0) { counters[0] = 0ull; counters[1] = 0ull; counters[2] = (unsigned long long)n; }
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < count; i += (int64_t)gridDim.x * 4) {      // wave-uniform
        const int64_t r = all ? i : (int64_t)filed[i];
        const float* rv = rows + (size_t)r * dim;
        uint64_t key = ~0ull;
        for (int j = lane; j < P; j += 64) {
            const uint64_t k = dist_key(exact_row_dist(rv, prompts + (size_t)j * dim, dim), (uint32_t)j);
            key = k < key ? k : key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor(key, o);
            key = other < key ? other : key;
        }
        if (lane == 0) {
            const float d = key_dist(key);
            lab[r] = d > max_dist ? -1 : (int32_t)(uint32_t)key;
            best[r] = d;
        }
    }
}

// ---- groups ----
// m rounds of the workgroup's largest (votes, inverted label) over hist [P]; each winner goes to tags / votes / sel and its
// counter is cleared; the unused slots of tags / votes / show are filled.  Every thread of the 256 calls it; returns the number
// of labels chosen (block-uniform).  hist is complete and visible (a barrier behind its last write).
__device__ __forceinline__ int label_select_rounds(uint32_t* hist, int P, int m, unsigned long long* red /*[4]*/, int32_t* sel /*[m]*/,
                                                   int32_t* __restrict__ tags, int32_t* __restrict__ votes, int32_t* __restrict__ show) {
    const int tid = threadIdx.x;
    int chosen = 0;
    for (int t = 0; t < m; ++t) {
        unsigned long long top = 0ull;
        for (int j = tid; j < P; j += 256) {
            const uint32_t v = hist[j];
            const unsigned long long key = v ? ((unsigned long long)v << 32) | (uint32_t)(0xffffffffu - (uint32_t)j) : 0ull;
            top = key > top ? key : top;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(top, o);
            top = other > top ? other : top;
        }
        __syncthreads();                                     // the previous round's readers are done with red[]
        if ((tid & 63) == 0) red[tid >> 6] = top;
        __syncthreads();
        top = max(max(red[0], red[1]), max(red[2], red[3]));
        if (top == 0ull) break;                              // block-uniform: a label without votes never competes
        const int j = (int)(0xffffffffu - (uint32_t)top);
        if (tid == 0) {
            tags[t] = j; votes[t] = (int32_t)(top >> 32);
            sel[t] = j; hist[j] = 0u;
        }
        ++chosen;
        __syncthreads();                                     // the cleared counter, before the next round reads it
    }
    for (int t = chosen + tid; t < m; t += 256) { tags[t] = -1; votes[t] = 0; show[t] = -1; }
    __syncthreads();
    return chosen;
}

// the smallest (best, tie) key per chosen label over rows grows[b .. e) -> show_key [chosen] (LDS, ~0 before)
__device__ __forceinline__ void label_show_sweep(const int32_t* __restrict__ grows, int b, int e, const int32_t* __restrict__ lab,
                                                 const float* __restrict__ best, const TieOrder tie, const int32_t* sel, int chosen,
                                                 unsigned long long* show_key) {
    for (int i = b + threadIdx.x; i < e; i += 256) {
        const int r = grows[i];
        const int L = lab[r];
        if (L < 0) continue;
        for (int t = 0; t < chosen; ++t)
            if (sel[t] == L) { atomicMin(&show_key[t], (unsigned long long)dist_key(best[r], tie_of(tie, r))); break; }
    }
}

// One workgroup per group of at most split_rows rows (longer ones leave at once: the split form below answers them).
// tags / votes / show [G][m], unlabelled [G].
__global__ __launch_bounds__(256)
void label_group_kernel(const int32_t* __restrict__ goff, const int32_t* __restrict__ grows, const int32_t* __restrict__ lab,
                        const float* __restrict__ best, int P, int m, int split_rows, const TieOrder tie, int32_t* __restrict__ tags,
                        int32_t* __restrict__ votes, int32_t* __restrict__ show, int32_t* __restrict__ unlabelled) {
    __shared__ uint32_t hist[LABEL_MAX_P];
    __shared__ unsigned long long red[4];
    __shared__ unsigned long long show_key[LABEL_MAX_M];
    __shared__ int32_t sel[LABEL_MAX_M];
    __shared__ int unl_s;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int b = goff[g], e = goff[g + 1];
    if (e - b > split_rows) return;                          // block-uniform
    for (int j = tid; j < P; j += 256) hist[j] = 0u;
    if (tid < LABEL_MAX_M) { show_key[tid] = ~0ull; sel[tid] = -1; }
    if (tid == 0) unl_s = 0;
    __syncthreads();
    int unl = 0;
    for (int i = b + tid; i < e; i += 256) {
        const int L = lab[grows[i]];
        if (L >= 0) atomicAdd(&hist[L], 1u);
        else ++unl;
    }
    if (unl) atomicAdd(&unl_s, unl);
    __syncthreads();
    if (tid == 0) unlabelled[g] = unl_s;
    const size_t o = (size_t)g * m;
    const int chosen = label_select_rounds(hist, P, m, red, sel, tags + o, votes + o, show + o);
    label_show_sweep(grows, b, e, lab, best, tie, sel, chosen, show_key);
    __syncthreads();
    if (tid < chosen) show[o + tid] = tie_row(tie, (uint32_t)show_key[tid]);
}

// ---- the split form: a group of more than split_rows rows is cut into pieces of piece_rows consecutive entries of its row
// list (host-built lists: LabelPieces).  Four launches for all long groups of a call; nothing waits on another workgroup. ----
struct LabelPieces {
    const int32_t* piece_long;   // [np] the piece's long group, as an index into long_group
    const int32_t* piece_b;      // [np] its entries grows[piece_b .. piece_e)
    const int32_t* piece_e;
    const int32_t* long_group;   // [nl] the group's label
    const int32_t* long_poff;    // [nl + 1] its pieces
    uint32_t* phist;             // [np][P] the pieces' histograms
    int32_t* punl;               // [np] the pieces' unlabelled rows
    int32_t* lsel;               // [nl][LABEL_MAX_M] the group's chosen labels (-1 unused)
    unsigned long long* pshow;   // [np][LABEL_MAX_M] the pieces' show keys
};

// 1. one workgroup per piece: its histogram (through LDS) and unlabelled count
__global__ __launch_bounds__(256)
void label_piece_hist_kernel(const int32_t* __restrict__ grows, const int32_t* __restrict__ lab, int P, const LabelPieces w) {
    __shared__ uint32_t hist[LABEL_MAX_P];
    __shared__ int unl_s;
    const int p = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < P; j += 256) hist[j] = 0u;
    if (tid == 0) unl_s = 0;
    __syncthreads();
    int unl = 0;
    for (int i = w.piece_b[p] + tid; i < w.piece_e[p]; i += 256) {
        const int L = lab[grows[i]];
        if (L >= 0) atomicAdd(&hist[L], 1u);
        else ++unl;
    }
    if (unl) atomicAdd(&unl_s, unl);
    __syncthreads();
    for (int j = tid; j < P; j += 256) w.phist[(size_t)p * P + j] = hist[j];
    if (tid == 0) w.punl[p] = unl_s;
}

// 2. one workgroup per long group: the pieces' histograms added in piece order, then the selection rounds
__global__ __launch_bounds__(256)
void label_long_select_kernel(int P, int m, const LabelPieces w, int32_t* __restrict__ tags, int32_t* __restrict__ votes,
                              int32_t* __restrict__ show, int32_t* __restrict__ unlabelled) {
    __shared__ uint32_t hist[LABEL_MAX_P];
    __shared__ unsigned long long red[4];
    __shared__ int32_t sel[LABEL_MAX_M];
    const int l = blockIdx.x, tid = threadIdx.x;
    const int g = w.long_group[l], p0 = w.long_poff[l], p1 = w.long_poff[l + 1];
    for (int j = tid; j < P; j += 256) {
        uint32_t v = 0u;
        for (int p = p0; p < p1; ++p) v += w.phist[(size_t)p * P + j];
        hist[j] = v;
    }
    if (tid < LABEL_MAX_M) sel[tid] = -1;
    if (tid == 0) {
        int unl = 0;
        for (int p = p0; p < p1; ++p) unl += w.punl[p];
        unlabelled[g] = unl;
    }
    __syncthreads();
    const size_t o = (size_t)g * m;
    label_select_rounds(hist, P, m, red, sel, tags + o, votes + o, show + o);
    if (tid < LABEL_MAX_M) w.lsel[l * LABEL_MAX_M + tid] = sel[tid];
}

// 3. one workgroup per piece: the piece's show keys for its group's chosen labels
__global__ __launch_bounds__(256)
void label_piece_show_kernel(const int32_t* __restrict__ grows, const int32_t* __restrict__ lab, const float* __restrict__ best,
                             const TieOrder tie, const LabelPieces w) {
    __shared__ unsigned long long show_key[LABEL_MAX_M];
    __shared__ int32_t sel[LABEL_MAX_M];
    __shared__ int chosen_s;
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid < LABEL_MAX_M) { show_key[tid] = ~0ull; sel[tid] = w.lsel[w.piece_long[p] * LABEL_MAX_M + tid]; }
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        while (c < LABEL_MAX_M && sel[c] >= 0) ++c;
        chosen_s = c;
    }
    __syncthreads();
    label_show_sweep(grows, w.piece_b[p], w.piece_e[p], lab, best, tie, sel, chosen_s, show_key);
    __syncthreads();
    if (tid < LABEL_MAX_M) w.pshow[(size_t)p * LABEL_MAX_M + tid] = show_key[tid];
}

// 4. thread (long group, tag): the pieces' show keys in piece order -> show
__global__ __launch_bounds__(256)
void label_long_show_kernel(int n_long, int m, const TieOrder tie, const LabelPieces w, int32_t* __restrict__ show) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int l = i / LABEL_MAX_M, t = i - l * LABEL_MAX_M;
    if (l >= n_long || t >= m || w.lsel[l * LABEL_MAX_M + t] < 0) return;
    unsigned long long key = ~0ull;
    for (int p = w.long_poff[l]; p < w.long_poff[l + 1]; ++p) {
        const unsigned long long k = w.pshow[(size_t)p * LABEL_MAX_M + t];
        key = k < key ? k : key;
    }
    show[(size_t)w.long_group[l] * m + t] = tie_row(tie, (uint32_t)key);
}

#endif  // __HIPCC__

}  // namespace vq
