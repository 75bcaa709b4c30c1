// Diverse search (vq_index_search_diverse): the k best rows of the plain search's exhaustive (distance, tie) list L such that no
// two kept rows lie closer than min_dist to each other — greedy over L in embedding space (include/vq_amd.h has the definition;
// DESIGN.md §4 "Diverse search").
//
//   plan_diverse                 host only: the prefix depth D, the producer of the prefix, the bit matrix's bytes, the redo's
//                                slices, the launches queued
//   diverse_pair_kernel          per query, the pairs i < j of its D prefix entries: is d(r_i, r_j) < min_dist?  The tile and the
//                                index-order fp64 chain of exact_dist_kernel, the rows gathered by id; one wave ballot per
//                                (entry i, 64 entries j) word of the bit matrix [nq][D][ceil(D / 64)]
//   diverse_walk_kernel          one wave per query walks the prefix in order with the "suppressed" words across its lanes, ORs
//                                in the matrix row of every entry it keeps, writes the k results and files the query for the
//                                redo when fewer than k rows were kept and L goes on behind the prefix
//   (distinct_dist_kernel of knn_distinct.h: the filed queries' exact distances [slots][n], once per slice)
//   diverse_pick_chunk_kernel    round t, level one: each chunk's smallest live (distance, tie) key per filed slot
//   diverse_pick_kernel          round t, level two: the slot's smallest key -> result t of its query and the picked row
//   diverse_suppress_kernel      round t: the exact-distance tile with the picked rows gathered as its "queries"; +inf to every
//                                live row with d < min_dist and to the picked row itself.  No distance table is stored
//   diverse_suppress_rows_kernel the same round when at most DIV_ROW_SLOTS slots of the slice are filed (the usual single query):
//                                one thread per live row, the keyframe summary's chain against the picked row in LDS; the
//                                filed count decides on the device which of the two does the work, the other leaves at once
//
// Two facts make both paths exact.  PREFIX (knn_distinct.h): a row's fate depends only on rows before it in L, so greedy over
// the first D entries keeps exactly the kept rows among them; k kept rows, or D = the index size, is the whole answer.  REDO:
// a live row is one that no kept row suppresses, so the smallest live (distance, tie) is the next row of L the walk would keep.
//
// d(a, b) is symmetric bit for bit: the products of two floats are exact in fp64 and commute, and both orders add them in
// index order.  Every redo workgroup reads the filed count first and leaves at once when its slot is not filed; the launches
// queued depend on the shapes and k only; stream order is the only synchronisation between them.  No global atomics beyond the
// walk's three counters (those of the distinct search).
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"
#include "knn_distinct.h"
#include "knn_summary.h"

#include <algorithm>

namespace vq {

constexpr int DIV_MAX_K = 256;               // results per query
constexpr int DIV_MIN_DEPTH = 256;           // the depth rule (DESIGN.md §4 "Diverse search" has the measurement that chose it)
constexpr int DIV_DEPTH_PER_K = 8;
constexpr int DIV_PICK_CHUNK = 8192;         // rows per level-one workgroup of the pick
constexpr int DIV_ROW_SLOTS = 4;             // filed slots of a slice up to which a round suppresses row by row, not by tiles

struct DiversePlan {
    int64_t depth;       // D: prefix entries fetched per query
    int producer;        // 0: exact distances + selection, 1: fp16 scan with proof
    int64_t pair_bytes;  // the bit matrix [nq][D][ceil(D / 64)] of 64-bit words (0: no pair pass runs)
    int64_t slice_q;     // filed queries per redo slice
    int slices;          // redo slices queued (0: no query can be filed)
    int launches;        // kernels queued behind the plain search's own
};

// The depth rule (include/vq_amd.h states it): D = max(256, 8 k), capped by the index size and by the producer's k limit; k
// alone when nothing can be suppressed before the k-th kept row (min_dist = 0, k = 1).  depth_override > 0 (tests) replaces the
// rule and is capped the same way.
inline DiversePlan plan_diverse(int64_t n, int nq, int k, float min_dist, int mode, int64_t depth_override) {
    DiversePlan p;
    p.producer = (mode == 2 || (mode == 0 && n >= DST_FP16_MIN_ROWS)) ? 1 : 0;
    const int64_t limit = std::min<int64_t>(n, p.producer ? DST_FP16_MAX_K : DST_MAX_DEPTH);
    const bool plain = !(min_dist > 0.0f) || k == 1;            // the first k rows of L are the answer
    int64_t d = plain ? k : std::max<int64_t>(DIV_MIN_DEPTH, (int64_t)DIV_DEPTH_PER_K * k);
    if (depth_override > 0) d = depth_override;
    p.depth = std::max<int64_t>(1, std::min(d, limit));
    const bool pairs = min_dist > 0.0f && p.depth > 1;
    p.pair_bytes = pairs ? (int64_t)nq * p.depth * ((p.depth + 63) / 64) * 8 : 0;
    const int64_t ld = round_up(n, 64);
    p.slice_q = std::max<int64_t>(1, std::min<int64_t>(nq, DST_DIST_BUDGET / ld));
    // a query is filed only when its prefix keeps fewer than k rows and L goes on behind it
    const bool can_file = p.depth < n && k > 1 && !(plain && p.depth >= k);
    p.slices = can_file ? (int)((nq + p.slice_q - 1) / p.slice_q) : 0;
    // the pair pass, the walk; per slice: the distances, k picks of two levels, k - 1 suppressions of two forms
    p.launches = (pairs ? 1 : 0) + 1 + p.slices * (1 + 2 * k + 2 * (k - 1));
    return p;
}

#ifdef __HIPCC__

// Grid (ceil(D / 64) column tiles x ceil(D / 32) entry tiles, nq).  Tile: 64 entries j (thread r = tid & 63) x 32 entries i
// (thread g = tid >> 6 owns 8g .. 8g + 7), exactly exact_dist_kernel's with the rows of both sides gathered through the
// prefix's ids.  Word (i, jw) of the matrix holds bit j - 64 jw for every j > i with d(r_i, r_j) < min_dist; a tile with no
// j > i writes zeros and leaves (pairs that cannot matter: the walk asks only about entries behind a kept one).
__global__ __launch_bounds__(256)
void diverse_pair_kernel(const float* __restrict__ rows, int64_t n, int dim, const int32_t* __restrict__ pre_ids, int D, int W,
                         float min_dist, uint64_t* __restrict__ bits) {
    __shared__ float xs[64][65];
    __shared__ double qs[32][64];
    __shared__ int32_t rj[64], ri[32];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int jw = blockIdx.x % W, it = blockIdx.x / W;
    const int64_t q = blockIdx.y;
    const int j0 = jw * 64, i0 = it * 32;
    uint64_t* out = bits + (q * D) * W + jw;                     // word (i, jw) at out [i * W]
    if (j0 + 63 <= i0) {                                         // every j of the tile is <= every i
        if (tid < 32 && i0 + tid < D) out[(int64_t)(i0 + tid) * W] = 0ull;
        return;
    }
    const int32_t* pi = pre_ids + q * D;
    if (tid < 64) { const int32_t v = j0 + tid < D ? pi[j0 + tid] : -1; rj[tid] = (v >= 0 && v < n) ? v : -1; }
    else if (tid < 96) { const int t = tid - 64; const int32_t v = i0 + t < D ? pi[i0 + t] : -1; ri[t] = (v >= 0 && v < n) ? v : -1; }
    __syncthreads();
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    for (int d0 = 0; d0 < dim; d0 += 64) {
        for (int i = tid; i < 64 * 64; i += 256) {
            const int rr = i >> 6, cc = i & 63;
            xs[rr][cc] = (rj[rr] >= 0 && d0 + cc < dim) ? rows[(int64_t)rj[rr] * dim + d0 + cc] : 0.f;
        }
        for (int i = tid; i < 32 * 64; i += 256) {
            const int qq = i >> 6, cc = i & 63;
            qs[qq][cc] = (ri[qq] >= 0 && d0 + cc < dim) ? (double)rows[(int64_t)ri[qq] * dim + d0 + cc] : 0.0;
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
    const bool jok = rj[r] >= 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int il = g * 8 + j, i = i0 + il;                   // wave-uniform: a wave shares g
        const bool close = jok && ri[il] >= 0 && j0 + r > i && 1.0f - (float)acc[j] < min_dist;
        const uint64_t word = __ballot(close);
        if (r == 0 && i < D) out[(int64_t)i * W] = word;
    }
}

// One wave per query.  pre_ids / pre_dist [nq][D]: the plain search's answer at depth D (sorted; -1 ends a list).  bits: the pair
// pass's matrix, or null when nothing suppresses (min_dist = 0, or one entry).  Lane l < W holds word l of the suppressed set
// (W <= DST_MAX_DEPTH / 64 = 16).
__global__ __launch_bounds__(64)
void diverse_walk_kernel(const int32_t* __restrict__ pre_ids, const float* __restrict__ pre_dist, int D, int W, int64_t n, int k,
                         const uint64_t* __restrict__ bits, int32_t* __restrict__ ids, float* __restrict__ dist,
                         int32_t* __restrict__ slots, unsigned long long* __restrict__ counters) {
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t* pi = pre_ids + q * D;
    const float* pd = pre_dist + q * D;
    const uint64_t* m = bits ? bits + q * D * W : nullptr;
    int32_t* oi = ids + q * k;
    float* od = dist + q * k;
    uint64_t sup = 0ull;
    int c = 0, i = 0;
    bool ended = D >= n;                                          // the prefix is all of L
    for (int base = 0; base < D && c < k; base += 64) {
        const int32_t mine = base + lane < D ? pi[base + lane] : -1;      // 64 entries per load
        const uint64_t valid = __ballot(mine >= 0 && mine < n);
        const int lim = min(64, D - base);
        int b = 0;
        for (; b < lim && c < k; ++b) {
            if (!((valid >> b) & 1ull)) { ended = true; break; }  // the list ended
            const uint64_t word = __shfl(sup, base >> 6);         // wave-uniform
            if ((word >> b) & 1ull) continue;
            if (lane == 0) { oi[c] = pi[base + b]; od[c] = pd[base + b]; }
            ++c;
            if (m && lane < W) sup |= m[(int64_t)(base + b) * W + lane];
        }
        i = base + b;
        if (ended) break;
    }
    for (int j = c + lane; j < k; j += 64) { oi[j] = -1; od[j] = __builtin_inff(); }
    if (lane == 0) {
        atomicAdd(counters + DST_WALKED, (unsigned long long)i);
        if (c < k && !ended) slots[atomicAdd(counters + DST_FILED, 1ull)] = (int32_t)q;
        else atomicAdd(counters + DST_PROVEN, 1ull);
    }
}

// ---- the redo's rounds.  dist [slot_cap][ld]: row s = filed slot slot_base + s (distinct_dist_kernel); +inf = not live ----

// Grid (chunks, slot_cap): the chunk's smallest live key -> part [s][chunk] (~0: none)
__global__ __launch_bounds__(256)
void diverse_pick_chunk_kernel(const float* __restrict__ dist, int64_t ld, int64_t n, const TieOrder tie, int nchunks,
                               uint64_t* __restrict__ part, const unsigned long long* __restrict__ counters, int slot_base, int slot_cap) {
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int s = blockIdx.y;
    if (s >= count) return;
    __shared__ uint64_t red[4];
    const int tid = threadIdx.x;
    const float* d = dist + (int64_t)s * ld;
    const int64_t r0 = (int64_t)blockIdx.x * DIV_PICK_CHUNK, r1 = min(n, r0 + DIV_PICK_CHUNK);
    const float inf = __builtin_inff();
    uint64_t best = ~0ull;
    for (int64_t r = r0 + tid; r < r1; r += 256) {
        const float v = d[r];
        if (v == inf) continue;
        const uint64_t key = dist_key(v, tie_of(tie, r));
        best = key < best ? key : best;
    }
    best = block_min_u64(best, red, tid);
    if (tid == 0) part[(int64_t)s * nchunks + blockIdx.x] = best;
}

// Grid (slot_cap): the slot's smallest key over its chunks -> result t of the slot's query, the picked row (-1: no live row)
__global__ __launch_bounds__(256)
void diverse_pick_kernel(const uint64_t* __restrict__ part, int nchunks, const TieOrder tie, int t, int k, const int32_t* __restrict__ slots,
                         const unsigned long long* __restrict__ counters, int slot_base, int slot_cap, int32_t* __restrict__ picked,
                         int32_t* __restrict__ ids, float* __restrict__ dist_out) {
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int s = blockIdx.x;
    if (s >= count) return;
    __shared__ uint64_t red[4];
    const int tid = threadIdx.x;
    uint64_t best = ~0ull;
    for (int c = tid; c < nchunks; c += 256) {
        const uint64_t key = part[(int64_t)s * nchunks + c];
        best = key < best ? key : best;
    }
    best = block_min_u64(best, red, tid);
    if (tid == 0) {
        const int64_t o = (int64_t)slots[slot_base + s] * k + t;
        const int32_t row = best == ~0ull ? -1 : tie_row(tie, (uint32_t)best);
        picked[s] = row;
        ids[o] = row;
        dist_out[o] = best == ~0ull ? __builtin_inff() : key_dist(best);
    }
}

// Grid (row tiles, capped at DST_DIST_GRID and strided; slots / 32): exact_dist_kernel's tile with the slots' picked rows as
// the queries.  A live row r of slot s gets +inf when d(r, picked [s]) < min_dist (min_dist > 0) or r is the picked row.  A wave
// whose eight slots are not filed only helps staging the tile.
__global__ __launch_bounds__(256)
void diverse_suppress_kernel(const float* __restrict__ rows, int64_t n, int dim, const int32_t* __restrict__ picked, float min_dist,
                             const unsigned long long* __restrict__ counters, int slot_base, int slot_cap, float* __restrict__ dist, int64_t ld) {
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int q0 = blockIdx.y * 32;
    if (q0 >= count || count <= DIV_ROW_SLOTS) return;           // (few slots: diverse_suppress_rows_kernel's)
    __shared__ float xs[64][65];
    __shared__ double qs[32][64];
    __shared__ int32_t qn[32];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    if (tid < 32) { const int32_t v = q0 + tid < count ? picked[q0 + tid] : -1; qn[tid] = (v >= 0 && v < n) ? v : -1; }
    __syncthreads();
    const float inf = __builtin_inff();
    const bool wave_live = q0 + g * 8 < count;                   // filed slots are contiguous: the usual one or two keep one wave busy
    for (int64_t row0 = (int64_t)blockIdx.x * 64; row0 < n; row0 += (int64_t)gridDim.x * 64) {
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
                qs[qq][cc] = (qn[qq] >= 0 && d0 + cc < dim) ? (double)rows[(int64_t)qn[qq] * dim + d0 + cc] : 0.0;
            }
            __syncthreads();
            if (wave_live) {
#pragma unroll 8
                for (int c = 0; c < 64; ++c) {
                    const double xv = (double)xs[r][c];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] += xv * qs[g * 8 + j][c];   // product exact in fp64
                }
            }
            __syncthreads();
        }
        const int64_t gr = row0 + r;
        if (gr < n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int sl = g * 8 + j;
                const int32_t pk = qn[sl];
                if (pk < 0) continue;                             // not filed, or the slot has no live row left
                const bool close = min_dist > 0.0f && 1.0f - (float)acc[j] < min_dist;
                if (close || gr == pk) dist[(int64_t)(q0 + sl) * ld + gr] = inf;      // (+inf over +inf: a dead row stays dead)
            }
        }
    }
}

// Grid (row blocks, capped at DST_DIST_GRID and strided; DIV_ROW_SLOTS), dynamic LDS dim * 8: the same round for a slice with at
// most DIV_ROW_SLOTS filed slots.  The tile above runs at a quarter of the memory rate with one live slot; here a thread owns a
// row and runs the keyframe summary's chain (exact_dot_chain_pf / exact_dot_chain: the same additions in the same order, the
// picked row widened to fp64 in LDS once), and a row that is already dead is not read at all.
__global__ __launch_bounds__(SUM_THREADS)
void diverse_suppress_rows_kernel(const float* __restrict__ rows, int64_t n, int dim, const int32_t* __restrict__ picked, float min_dist,
                                  const unsigned long long* __restrict__ counters, int slot_base, int slot_cap, float* __restrict__ dist, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) char div_smem[];
    const int count = min((int)counters[DST_FILED] - slot_base, slot_cap);
    const int s = blockIdx.y, tid = threadIdx.x;
    if (count > DIV_ROW_SLOTS || s >= count) return;
    const int32_t pk = picked[s];
    if (pk < 0 || pk >= n) return;                                // the slot has no live row left
    double* cq = (double*)div_smem;
    sum_stage_centre(rows, dim, pk, cq, tid);
    __syncthreads();
    float* d = dist + (int64_t)s * ld;
    const float inf = __builtin_inff();
    const bool pf = (dim & 31) == 0;
    for (int64_t r = (int64_t)blockIdx.x * SUM_THREADS + tid; r < n; r += (int64_t)gridDim.x * SUM_THREADS) {
        if (d[r] == inf) continue;
        const float* x = rows + r * dim;
        const float dot = pf ? exact_dot_chain_pf(x, cq, dim) : exact_dot_chain(x, cq, dim);
        if ((min_dist > 0.0f && 1.0f - dot < min_dist) || r == pk) d[r] = inf;
    }
}

#endif  // __HIPCC__

}  // namespace vq
