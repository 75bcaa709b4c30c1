// Library neighbours (vq_index_neighbors): for every asked row of the matrix its k nearest rows among the rows that are not
// "the same" as it — not the row itself (exclude = 0) or not of the row's own group (exclude = 1).  include/vq_amd.h has the
// definition; DESIGN.md §4 "Library neighbours".  The one n x n operation of the library: the queries are rows of the matrix.
//
//   plan_neighbors            host only: which path a call takes, the chunk of asked rows, the key scratch, the re-score kind
//   neighbors_prepare_kernel  per chunk: the asked rows' tags; for a row list also their fp16 copies and fp32 masters, gathered
//   neighbors_tile_kernel     pass 1: 256 asked rows x up to 2,048 matrix rows per workgroup, per (row, 128-row stream) the two
//                             largest fp16 keys over the ELIGIBLE rows of the stream
//   (pass 2: rescore_verify_kernel_t<4, .., EligTag, NB_RESCAN>, knn_scan_f16.h; pass 3: exact_fallback_kernel<false, EligTag>, knn_fallback.h)
//   neighbors_strike_kernel   exact path: +inf over the ineligible entries of a chunk's distance table
//   neighbors_fix_kernel      exact path: a selected slot whose distance is +inf held a struck entry -> the empty slot (-1, +inf)
//   neighbors_stats_kernel    adds a chunk's outcome counters to the call's
//
// Tags.  A pair (asked row, matrix row) is struck when their tags are equal: the tag of a row is its row number (exclude = 0)
// or its group label (exclude = 1), so eligibility is ONE integer compare.  Rows that do not exist — the pad rows of a ragged
// last tile, on the resident side and on the streamed side — carry NB_PAD_TAG, which strikes every pair they are in.
//
// Pass 1 is the batch scan's job (knn_scan_fold.h) with the matrix on both sides, on the streamed 256 x 256 mainloop
// (scan_stream256.h): the resident tile is 256 asked rows (for "every row": 256 rows of the fp16 scan copy itself, nothing is
// copied), the streamed tiles are the up to eight 256-row tiles of one 2,048-row range.  Wave (wr, wc) owns resident rows
// 128 wr .. +127 and streamed rows 64 wc .. +63 of every tile; a lane holds, for each of its 8 resident rows, 16 scores per
// tile: its own 128-row stream (range, wc, lane group), the batch scans' stream — rows range * 2048 + t * 256 + wc * 64 +
// ni * 16 + 4 g + r, local index t * 16 + ni * 4 + r, scan2_row_of.  Per resident row the lane keeps the stream's (best, second)
// keys in registers; a key is the fp32 score with the local index in its low 7 mantissa bits, compared as a float, exactly the
// batch scans' key, and the keys go out in their layout (batch_key_index, layout 2), so the re-score kernels read them as they
// read scan5's.  Before a score enters the fold it is replaced by the finite sentinel NB_MASKED when its pair is struck.
// The tags sit in the 9 KiB of LDS behind the mainloop's buffers: the resident rows' 256 and the range's 2,048, fetched once
// per workgroup with 16-byte loads before the K loop starts; the fold reads them with two 16-byte and four 4-byte LDS loads
// per quadrant.  The fold obeys scan_stream256.h: no barrier, accumulators left cleared.
//
// Proof.  Every key is a key over eligible rows, every bound the re-score takes (a stream's second key, a share's floor, the
// (C+1)-th kept key) is therefore a bound over eligible rows, and the unfiltered argument of knn_scan_f16.h holds unchanged
// with "row" read as "eligible row".  E = scan_eps_unit(dim) * max|row| * |q|, and q is a stored row.  A struck score's key
// decodes to about -3e38: it loses to every real score and closes every bound it is part of.  A row with fewer than k
// eligible rows among its candidates (a small library, or nearly all of it in the row's own group) is flagged and answered by
// pass 3, whose lists never take a struck row: its unused slots come out as (-1, +inf).
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "scan_stream256.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "scan_plan.h"

#include <algorithm>

namespace vq {

constexpr int NB_ROW_TILE = 256;                     // asked rows per workgroup
constexpr int NB_RANGE = SCAN2_RANGE;                // matrix rows per workgroup: eight streamed tiles
constexpr int NB_RANGE_TILES = NB_RANGE / 256;
constexpr int NB_K_EXACT_MAX = 1024;                 // mode 1
constexpr int64_t NB_FP16_MIN_ROWS = 16384;          // mode 0 takes the tile path from this many stored rows (the plain search's bound) ...
constexpr int64_t NB_AUTO_MIN_M = 64;                // ... and asked rows: the smallest list measured, already 2 x ahead of the exact path (profiles/neighbors/probe.txt)
constexpr int64_t NB_DIST_WORDS = (int64_t)128 << 20;    // exact path: 512 MiB of fp32 distances per chunk
constexpr float NB_MASKED = -3.0e38f;                // finite (knn_scan_fold.h says why), below every score
constexpr int32_t NB_PAD_TAG = INT32_MIN;            // no label and no row number
// The re-score (knn_scan_f16.h) with more stream rescans than the searches' 4.  A library's neighbours come in runs: a frame's
// best matches in another video are a handful of ADJACENT frames, four consecutive rows share a 128-row stream, so the rows a
// stream hides behind its second key matter for nearly every asked row, and with 4 rescans a quarter of the rows (every row
// but itself: 19 in 20) went to the exact redo, which then took 96 % of the call (profiles/neighbors/probe.txt).  Eight
// rescans cover them; the pool's LDS (128 rows each) allows that at four rows per workgroup, six with 128 candidates.
constexpr int NB_RESCORE_QPW = 4;
constexpr int NB_RESCAN = 8, NB_RESCAN_XL = 6;
constexpr int NB_LDS_BYTES = G2_LDS_BYTES + (NB_ROW_TILE + NB_RANGE) * 4;
static_assert(NB_RANGE_TILES * 16 <= 128, "the lane-local row index fits 7 bits");
static_assert(NB_RANGE == SP_BATCH_RANGE && NB_ROW_TILE == SP_BATCH_QT, "the batch scans' geometry: key layout 2");

struct NeighborsPlan {
    int fp16;              // 1: the tile path answers the call
    int64_t chunk_rows;    // asked rows per chunk: whole 256-row tiles (tile path), the distance table's budget (exact path)
    int64_t chunks;
    int64_t key_bytes;     // tile path: the chunk's keys
    int64_t streams;       // 128-row streams of the matrix
    int ranges;
    int rescore;           // RescoreKind (scan_plan.h) of the tile path
    int rescore_qpw;
    float eps;             // unit rows: k-th and (k+1)-th eligible scores more than 4 eps apart are proven without a rescan
};

// near_unit: the index's rows are.  chunk_override: $VQ_AMD_NEIGHBORS_CHUNK (tests), 0 = none.  Mode 2 is refused by the caller
// when !fp16 below.
inline NeighborsPlan plan_neighbors(int64_t n, int dim, int64_t m, int k, int mode, bool near_unit, int64_t chunk_override) {
    NeighborsPlan p;
    const bool ok = scan_fp16_dim(dim) && near_unit && n >= 1 && k <= RV_K_MAX;
    p.fp16 = (mode == 2 && ok) || (mode == 0 && ok && n >= NB_FP16_MIN_ROWS && m >= NB_AUTO_MIN_M) ? 1 : 0;
    const int64_t n_pad = round_up(std::max<int64_t>(n, 1), NB_RANGE);
    p.streams = n_pad / SP_STREAM_ROWS;
    p.ranges = (int)(n_pad / NB_RANGE);
    const int64_t m_pad = round_up(std::max<int64_t>(m, 1), NB_ROW_TILE);
    if (p.fp16) {
        p.chunk_rows = std::min<int64_t>(std::max<int64_t>(NB_ROW_TILE, SP_KEY_BUDGET / p.streams / NB_ROW_TILE * NB_ROW_TILE), m_pad);   // plan_scan's q_chunk
    } else {
        const int64_t ld = round_up(std::max<int64_t>(n, 1), 64);
        p.chunk_rows = std::min<int64_t>(std::max<int64_t>(NB_ROW_TILE, NB_DIST_WORDS / ld / NB_ROW_TILE * NB_ROW_TILE), m_pad);
    }
    if (chunk_override > 0) p.chunk_rows = std::min<int64_t>(round_up(chunk_override, NB_ROW_TILE), m_pad);
    p.chunks = (std::max<int64_t>(m, 1) + p.chunk_rows - 1) / p.chunk_rows;
    p.key_bytes = p.fp16 ? p.streams * p.chunk_rows * 8 : 0;
    p.rescore = k > SP_K_MID ? RESCORE_XLARGE4 : k > SP_K_SMALL ? RESCORE_LARGE4 : RESCORE_BATCH8;      // the candidate pool: 128, 80, 32
    p.rescore_qpw = NB_RESCORE_QPW;
    p.eps = scan_fp16_dim(dim) ? scan_eps_unit(dim) * 1.0001f * 1.0001f : 0.f;
    return p;
}

#ifdef __HIPCC__

// ---- per chunk: asked rows q0 .. q0 + cur - 1 of the call.  list: the call's row list (null = every row: asked row i is row i).
// qtag [q_pad] <- the asked rows' tags (group_of null: the row number), NB_PAD_TAG behind cur.  With a list also q32 [cur][dim] <-
// the fp32 masters and q16 [q_pad][dim] <- the fp16 copies, zero rows behind cur.  One wave per asked row. ----
__global__ __launch_bounds__(256)
void neighbors_prepare_kernel(const int32_t* __restrict__ list, int64_t q0, int cur, int64_t q_pad, const int32_t* __restrict__ group_of,
                              const float* __restrict__ rows, const uint16_t* __restrict__ rows16, int dim,
                              int32_t* __restrict__ qtag, float* __restrict__ q32, uint16_t* __restrict__ q16) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < q_pad; i += (int64_t)gridDim.x * 4) {      // wave-uniform
        const bool live = i < cur;
        const int64_t r = !live ? 0 : list ? (int64_t)list[q0 + i] : q0 + i;
        if (lane == 0) qtag[i] = !live ? NB_PAD_TAG : group_of ? group_of[r] : (int32_t)r;
        if (!list) continue;
        if (q16)                                                  // the tile path only: dim is 256, 512 or 768
            for (int c = lane * 8; c < dim; c += 512) {
                uint4 h = uint4{0u, 0u, 0u, 0u};
                if (live) h = *(const uint4*)(rows16 + (size_t)r * dim + c);
                *(uint4*)(q16 + (size_t)i * dim + c) = h;
            }
        if (live)
            for (int c = lane * 4; c < dim; c += 256) *(float4*)(q32 + (size_t)i * dim + c) = *(const float4*)(rows + (size_t)r * dim + c);
    }
}

// ---- pass 1.  A16 [q_tiles * 256][dim]: the chunk's q_valid asked rows (fp16), qtag [q_tiles * 256] their tags; X16: the matrix's fp16
// copy, whole 2,048-row ranges allocated; rtag [n] the matrix rows' labels, or null: a row's tag is its number.  Grid and the
// workgroup -> (range, resident tile) blocking inside an XCD are scan5_f16_top2_kernel's (knn_scan_fold.h): 32 consecutive
// workgroups = 2^rb_log2 ranges x 32 / 2^rb_log2 resident tiles.  keys: batch_key_index over n_ranges * 16 streams. ----
__global__ __launch_bounds__(G2_THREADS, 2)
void neighbors_tile_kernel(const uint16_t* __restrict__ A16, const int32_t* __restrict__ qtag, const uint16_t* __restrict__ X16,
                           const int32_t* __restrict__ rtag, int dim, int64_t n_valid, int q_valid, int q_tiles, int n_ranges,
                           int range_groups, uint32_t* __restrict__ keys, int rb_log2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const Stream256Lane ln = stream256_lane();
    const int wr = ln.wr, wc = ln.wc, frow = ln.frow, fgrp = ln.fgrp;

    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int blk = wg >> 5, inner = wg & 31;
    const int rg = blk % range_groups, qg = blk / range_groups;
    const int qb_log2 = 5 - rb_log2;
    const int range = (rg << rb_log2) + (inner >> qb_log2);
    const int qtile = (qg << qb_log2) + (inner & ((1 << qb_log2) - 1));
    if (range >= n_ranges || qtile >= q_tiles) return;   // whole workgroup leaves before any barrier
    const int m0 = qtile * NB_ROW_TILE;
    const int64_t n0 = (int64_t)range * NB_RANGE;
    const int rows_here = (int)min((int64_t)NB_RANGE, n_valid - n0);       // >= 1: ranges = cdiv(n, 2048)
    const int nt = (rows_here + 255) >> 8;                                 // streamed tiles that hold a row

    // ---- tags -> LDS behind the mainloop's buffers: qt_s [256], st_s [2048]; one 16-byte load each per thread ----
    int32_t* const qt_s = (int32_t*)(smem + G2_LDS_BYTES);
    int32_t* const st_s = qt_s + NB_ROW_TILE;
    {
        const int c4 = tid * 4;                                            // streamed rows c4 .. c4 + 3 of the range
        int4 tg = int4{NB_PAD_TAG, NB_PAD_TAG, NB_PAD_TAG, NB_PAD_TAG};
        if (rtag) {
            if (c4 + 3 < rows_here) tg = *(const int4*)(rtag + n0 + c4);   // n0 + c4 is a multiple of 4
            else {
                if (c4 < rows_here) tg.x = rtag[n0 + c4];
                if (c4 + 1 < rows_here) tg.y = rtag[n0 + c4 + 1];
                if (c4 + 2 < rows_here) tg.z = rtag[n0 + c4 + 2];
            }
        } else {
            const int32_t b = (int32_t)n0 + c4;
            if (c4 < rows_here) tg.x = b;
            if (c4 + 1 < rows_here) tg.y = b + 1;
            if (c4 + 2 < rows_here) tg.z = b + 2;
            if (c4 + 3 < rows_here) tg.w = b + 3;
        }
        *(int4*)(st_s + c4) = tg;
        if (tid < NB_ROW_TILE / 4) *(int4*)(qt_s + tid * 4) = *(const int4*)(qtag + m0 + tid * 4);
    }
    __syncthreads();                                     // before the mainloop: no DMA is in flight yet
    // pad rows on either side: only the chunk's last resident tile and the matrix's last range (workgroup-uniform)
    const bool pads = rows_here < nt * 256 || m0 + NB_ROW_TILE > q_valid;

    const float NEG = -__builtin_inff();
    float m1[8], m2[8];                                  // per resident row block mi: the stream's (best, second) keys so far
#pragma unroll
    for (int i = 0; i < 8; ++i) { m1[i] = NEG; m2[i] = NEG; }
    // first-key update as med3(first, key, BIG): a max the compiler cannot turn into the canonicalising fmaxf form (knn_scan_fold.h)
    float BIG = 3.0e38f;
    asm volatile("" : "+v"(BIG));

    // Fold quadrant (hm, hn) of streamed tile t into the resident rows' running keys and clear it.
    auto fold = [&](f32x4 (&acc)[8][4], int hm, int hn, int t) __attribute__((always_inline)) {
        int4 st[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) st[j] = *(const int4*)(st_s + t * 256 + wc * 64 + (hn * 2 + j) * 16 + 4 * fgrp);
        int32_t qt[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qt[i] = qt_s[wr * 128 + (hm * 4 + i) * 16 + frow];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mi = hm * 4 + i;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ni = hn * 2 + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int32_t s = r == 0 ? st[j].x : r == 1 ? st[j].y : r == 2 ? st[j].z : st[j].w;
                    bool struck = s == qt[i];
                    if (pads) struck = struck || s == NB_PAD_TAG || qt[i] == NB_PAD_TAG;
                    const float v = struck ? NB_MASKED : acc[mi][ni][r];
                    const float kf = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, v) & ~127u) | (uint32_t)(t * 16 + ni * 4 + r));
                    m2[mi] = __builtin_amdgcn_fmed3f(m1[mi], m2[mi], kf);
                    m1[mi] = __builtin_amdgcn_fmed3f(m1[mi], kf, BIG);
                }
                acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    stream256_run(smem, ln, A16 + (size_t)m0 * dim, X16 + (size_t)n0 * dim, dim, nt, fold);

    const int64_t stream = (int64_t)range * 16 + wc * 4 + fgrp;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        const int q = m0 + wr * 128 + mi * 16 + frow;
        *(uint2*)(keys + batch_key_index(stream, q, (int64_t)n_ranges * 16)) = uint2{__builtin_bit_cast(uint32_t, m1[mi]), __builtin_bit_cast(uint32_t, m2[mi])};
    }
}

// ---- exact path: dist [cur][ld] of asked rows q0 .. (tags qtag + q0) against every row; one workgroup per asked row strikes
// its ineligible entries: entry qtag (exclude = 0: goff null), or the by-group row list of group qtag ----
__global__ __launch_bounds__(256)
void neighbors_strike_kernel(float* __restrict__ dist, int64_t ld, const int32_t* __restrict__ qtag, const int32_t* __restrict__ goff,
                             const int32_t* __restrict__ grows) {
    const int q = blockIdx.x;
    const int32_t tag = qtag[q];
    float* d = dist + (int64_t)q * ld;
    if (!goff) { if (threadIdx.x == 0) d[tag] = __builtin_inff(); return; }
    for (int i = goff[tag] + threadIdx.x; i < goff[tag + 1]; i += 256) d[grows[i]] = __builtin_inff();
}

// a struck entry the selection emitted (fewer eligible rows than k) becomes the empty slot; stored rows are finite, and a
// finite row's distance is finite
__global__ __launch_bounds__(256)
void neighbors_fix_kernel(int32_t* __restrict__ ids, const float* __restrict__ dist, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
        if (dist[i] == __builtin_inff()) ids[i] = -1;
}

// counters {flagged, proven at once, proven after rescans, fallback} of one chunk (collect_flags_kernel) -> the call's
// total {proven, of those after rescans, exact}
__global__ void neighbors_stats_kernel(const int32_t* __restrict__ counters, unsigned long long* __restrict__ total) {
    if (threadIdx.x == 0) {
        total[0] += (unsigned long long)(counters[1] + counters[2]);
        total[1] += (unsigned long long)counters[2];
        total[2] += (unsigned long long)counters[3];
    }
}

#endif  // __HIPCC__

}  // namespace vq
