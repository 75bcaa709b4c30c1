// Chapter segmentation (vq_index_segment_groups): the optimal cut of each listed group (video), walked in (position, tie) order,
// into at most k contiguous runs.  include/vq_amd.h has the definition, the ORDER of every floating-point operation included;
// DESIGN.md §4 "Chapter segmentation".
//
//   plan_segment             host only: the group batches, table bytes, the DP's LDS row limit and bytes, the launches
//   seg_prefix_kernel        one workgroup per listed group: P [L + 1][dim] fp64, one chain per column along the order
//   seg_pair_kernel          one workgroup per 64 x 64 tile of (a, b) pairs of the band b - a <= W: cost[b - 1][b - a - 1] fp64
//   seg_dp_kernel            one workgroup per listed group: E_c(b) for c = 1 .. K over the band table, back-pointers, the number
//                            of chapters, the walk back; two E arrays in LDS, or in global memory above the row limit
//   seg_show_kernel          one workgroup per (listed group, chapter slot): the chapter's row most like the chapter's own direction
//   seg_stats_kernel         the call's counters
//
// The pair kernel.  A workgroup of 256 threads owns the pairs a in [64 i, 64 i + 64), b - 1 in [64 j, 64 j + 64) of one group;
// the grid runs over every listed group's (j, j - i) rectangle, so one long video spreads over the machine (a tile with i < 0
// leaves at once).  The 128 prefix rows go through LDS 32 columns at a time, TRANSPOSED: image [column][row] of fp64.  A lane
// stages one row (16 B global loads, the next chunk's issued before this chunk's arithmetic), so the 64 lanes of a wave write 64
// adjacent 8-byte words of one column: no bank conflict.  A thread owns a 4 x 4 block of pairs — rows {2 t, 2 t + 1, 32 + 2 t,
// 33 + 2 t} of either side — so each side's four values of a column are two 16-byte LDS reads; the 16 lanes that differ in
// their a rows read 256 adjacent bytes (all 64 banks once), the b rows are the same address in those lanes (a broadcast).  16
// fp64 accumulators (32 VGPRs) and 8 staged values leave the kernel far below 128 VGPRs: two workgroups a CU, one hiding the
// other's barriers.  Each pair's chain over the columns belongs to one thread and runs in column order whatever the tiling.
//
// The DP.  Costs E are kept as the sequence search's 64-bit order-preserving keys (seq_key; SEQ_UNDEF: no such split), so the
// minimum over a is an integer minimum of (key, a): a wave takes one b, its lanes the admissible a (the table row of b is read
// contiguously), and reduces by shuffles; the waves of the workgroup share the b of a step c and meet at one barrier per c.
// The last step needs E_K(L) only.
//
// Contraction.  The library is built with -ffp-contract=on.  The kernels hold additions and subtractions, one square root and
// one division per cost or spread, and products of two fp32 values widened to fp64 (u * u, x * u, c * penalty): those products
// are exact, so fma(u, u, V) and the rounded product added to V are the same number (the argument at the head of
// knn_cluster.h).  Nothing else can be contracted.
//
// Stores are plain vector stores; no floating-point atomics, no global atomics at all, no workgroup waits for another: stream
// order between launches, barriers inside.  The launches queued depend on the group sizes (known on the host) only.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "knn_sequence.h"

#include <algorithm>
#include <vector>

namespace vq {

constexpr int SEG_MAX_K = 64;                                 // chapters per group
constexpr int64_t SEG_MAX_PAIRS = (int64_t)1 << 26;           // L * W of one group
constexpr int64_t SEG_COST_BYTES = (int64_t)512 << 20;        // band tables (and, apart, prefix rows) of one batch of groups
constexpr int SEG_TILE = 64;                                  // pairs per side of a pair-kernel tile
constexpr int SEG_CHUNK = 32;                                 // columns staged at a time
constexpr int SEG_PAIR_THREADS = 256;
constexpr int SEG_LDS_ROWS = 4096;                            // longest group of the DP's LDS form
constexpr int SEG_DP_THREADS = 1024;
constexpr int SEG_SHOW_THREADS = 256;

// One listed group of a batch (host-built, uploaded with the call).  The entry behind the batch's last holds tile0 = all tiles.
struct SegEntry {
    int64_t toff;        // its band table in the batch's, in pairs
    int64_t bpoff;       // its back-pointers [K][L + 1] in the batch's
    int64_t eoff;        // its two E arrays [2][L + 1] in the batch's (global form)
    int32_t group, L, W; // label, rows, longest run
    int32_t slot;        // index into the call's outputs
    int32_t prow;        // its first prefix row in the batch's
    int32_t tile0;       // its first tile in the pair kernel's grid
    int32_t band;        // tiles per b-tile: j - i = 0 .. band - 1
    int32_t pad_;
};
static_assert(sizeof(SegEntry) == 56, "SegEntry: 14 words");
constexpr int SEG_ENTRY_WORDS = (int)(sizeof(SegEntry) / 4);

inline int64_t seg_run_limit(int64_t L, int64_t max_len) { return max_len <= 0 ? L : std::min(L, max_len); }
inline int64_t seg_pairs(int64_t L, int64_t W) { return W * L - W * (W - 1) / 2; }            // 0 <= a < b <= L, b - a <= W
inline int seg_tiles_b(int64_t L) { return (int)((L + SEG_TILE - 1) / SEG_TILE); }
inline int seg_band(int64_t L, int64_t W) { return (int)std::min<int64_t>(seg_tiles_b(L) - 1, (W + SEG_TILE - 2) / SEG_TILE) + 1; }

struct SegmentPlan {
    std::vector<int32_t> batch_end;   // listed groups [batch_end[i - 1], batch_end[i]) make batch i
    int batches;
    int64_t table_bytes;              // the largest batch's band tables
    int64_t prefix_rows;              // the largest batch's prefix rows
    int64_t bp_words, e_words;        // the largest batch's back-pointers; its global-form E keys
    int64_t tiles;                    // the largest pair grid
    int64_t pairs;                    // pairs costed by the call
    int lds_rows;                     // groups of at most this many rows keep E in LDS
    int64_t lds_bytes;                // the DP's dynamic LDS
    int global_form;                  // 1: the longest listed group keeps E in global memory
    int launches;
};

// lengths [n_sel]: rows of each listed group, in list order.  cost_bytes_override / lds_rows_override > 0 (tests) replace the
// budget and lower the row limit.  A batch is the longest run of listed groups whose tables AND whose prefix rows each stay
// within the budget; a group that exceeds it alone is a batch of its own.
inline SegmentPlan plan_segment(const int64_t* lengths, int32_t n_sel, int dim, int k, int64_t max_len, bool show,
                                int64_t cost_bytes_override, int64_t lds_rows_override) {
    SegmentPlan p;
    const int64_t budget = cost_bytes_override > 0 ? cost_bytes_override : SEG_COST_BYTES;
    p.lds_rows = (int)(lds_rows_override > 0 ? std::min<int64_t>(lds_rows_override, SEG_LDS_ROWS) : SEG_LDS_ROWS);
    p.table_bytes = p.prefix_rows = p.bp_words = p.e_words = p.tiles = p.pairs = 0;
    int64_t tb = 0, pr = 0, bp = 0, ew = 0, tl = 0, longest = 0, lds_longest = 0;
    auto close = [&](int32_t end) {
        p.batch_end.push_back(end);
        p.table_bytes = std::max(p.table_bytes, tb); p.prefix_rows = std::max(p.prefix_rows, pr);
        p.bp_words = std::max(p.bp_words, bp); p.e_words = std::max(p.e_words, ew); p.tiles = std::max(p.tiles, tl);
        tb = pr = bp = ew = tl = 0;
    };
    for (int32_t i = 0; i < n_sel; ++i) {
        const int64_t L = lengths[i], W = seg_run_limit(L, max_len);
        const int64_t t = L * W * 8, r = L + 1;
        if (pr > 0 && (tb + t > budget || (pr + r) * dim * 8 > budget)) close(i);      // (pr > 0: the batch holds a group)
        tb += t; pr += r;
        bp += std::min<int64_t>(k, L) * (L + 1);
        if (L > p.lds_rows) ew += 2 * (L + 1); else lds_longest = std::max(lds_longest, L);
        tl += L ? (int64_t)seg_tiles_b(L) * seg_band(L, W) : 0;
        p.pairs += seg_pairs(L, W);
        longest = std::max(longest, L);
    }
    close(n_sel);
    p.batches = (int)p.batch_end.size();
    p.lds_bytes = 2 * round_up(lds_longest + 1, 64) * 8;
    p.global_form = longest > p.lds_rows ? 1 : 0;
    p.launches = p.batches * (show ? 4 : 3) + 1;
    return p;
}

#ifdef __HIPCC__

// ---- grid = the batch's entries; thread t owns columns 4 t .. 4 t + 3.  P [rows of the batch][dim] ----
__global__ __launch_bounds__(1024)
void seg_prefix_kernel(const float* __restrict__ rows, int dim, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                       const SegEntry* __restrict__ ent, double* __restrict__ P) {
    const SegEntry en = ent[blockIdx.x];
    const int c0 = threadIdx.x * 4;
    if (c0 >= dim) return;
    const int32_t* so = sorder + goff[en.group];
    const float* base = rows + c0;
    double* out = P + (size_t)en.prow * dim + c0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    *(double2*)out = double2{s0, s1};
    *(double2*)(out + 2) = double2{s2, s3};
    const int L = en.L;
    int t = 0;
    for (; t + 8 <= L; t += 8) {                                         // eight rows' loads in flight before the dependent adds
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *(const float4*)(base + (size_t)so[t + u] * dim);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s0 += (double)v[u].x; s1 += (double)v[u].y; s2 += (double)v[u].z; s3 += (double)v[u].w;
            out += dim;
            *(double2*)out = double2{s0, s1};
            *(double2*)(out + 2) = double2{s2, s3};
        }
    }
    for (; t < L; ++t) {
        const float4 v = *(const float4*)(base + (size_t)so[t] * dim);
        s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        out += dim;
        *(double2*)out = double2{s0, s1};
        *(double2*)(out + 2) = double2{s2, s3};
    }
}

// the entry of tile t: the last e with ent[e].tile0 <= t (tile0 ascending, ent[n_ent].tile0 > t)
__device__ __forceinline__ int seg_entry_of_tile(const SegEntry* __restrict__ ent, int n_ent, int t) {
    int lo = 0, hi = n_ent;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ent[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- grid = the batch's tiles.  tab: the batch's band tables ----
__global__ __launch_bounds__(SEG_PAIR_THREADS)
void seg_pair_kernel(const SegEntry* __restrict__ ent, int n_ent, const double* __restrict__ P, int dim, double* __restrict__ tab) {
    __shared__ __attribute__((aligned(16))) double img[2][SEG_CHUNK][SEG_TILE];      // [side][column][row]: 32 KiB
    const int tid = threadIdx.x;
    const SegEntry en = ent[seg_entry_of_tile(ent, n_ent, blockIdx.x)];
    const int local = (int)blockIdx.x - en.tile0;
    const int j = local / en.band, i = j - local % en.band;
    if (i < 0) return;                                                   // block-uniform, before any barrier
    const int L = en.L, W = en.W;
    const int a0 = i * SEG_TILE, b0 = j * SEG_TILE;                      // b0: the tile's first b - 1
    // staging: this lane's row of one side, column pairs sp, sp + 2, ...
    const int side = (tid >> 6) & 1, sr = tid & 63, sp = tid >> 7;
    const int prow = side ? b0 + sr + 1 : a0 + sr;                       // prefix row: a, or b = (b - 1) + 1
    const bool live = (side ? b0 + sr : a0 + sr) < L;
    const double* src = P + ((size_t)en.prow + (live ? prow : 0)) * dim;
    double2 st[SEG_CHUNK / 4];
    auto fetch = [&](int c0) {
        const int cn = min(SEG_CHUNK, dim - c0);
#pragma unroll
        for (int it = 0; it < SEG_CHUNK / 4; ++it) {
            const int c = 2 * (sp + 2 * it);
            st[it] = (live && c < cn) ? *(const double2*)(src + c0 + c) : double2{0.0, 0.0};
        }
    };
    const int ta = tid & 15, tb = tid >> 4;
    double V[4][4];
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) V[y][x] = 0.0;
    fetch(0);
    for (int c0 = 0; c0 < dim; c0 += SEG_CHUNK) {
        const int cn = min(SEG_CHUNK, dim - c0);
        __syncthreads();                                                 // the chunk before has been read
#pragma unroll
        for (int it = 0; it < SEG_CHUNK / 4; ++it) {
            const int c = 2 * (sp + 2 * it);
            img[side][c][sr] = st[it].x;
            img[side][c + 1][sr] = st[it].y;
        }
        __syncthreads();
        if (c0 + SEG_CHUNK < dim) fetch(c0 + SEG_CHUNK);
#pragma unroll 2
        for (int c = 0; c < cn; ++c) {
            const double2 a01 = *(const double2*)&img[0][c][2 * ta], a23 = *(const double2*)&img[0][c][32 + 2 * ta];
            const double2 b01 = *(const double2*)&img[1][c][2 * tb], b23 = *(const double2*)&img[1][c][32 + 2 * tb];
            const double av[4] = {a01.x, a01.y, a23.x, a23.y}, bv[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float u = (float)(bv[y] - av[x]);
                    V[y][x] += (double)u * (double)u;                    // exact product: contraction cannot change the sum
                }
        }
    }
    double* out = tab + en.toff;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        const int b1 = b0 + (y >> 1) * 32 + 2 * tb + (y & 1);           // b - 1
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int a = a0 + (x >> 1) * 32 + 2 * ta + (x & 1);
            const int d = b1 - a;                                        // b - a - 1
            if (b1 < L && d >= 0 && d < W) out[(size_t)b1 * W + d] = (double)(d + 1) - __builtin_sqrt(V[y][x]);
        }
    }
}

// One group: E over prev / cur [L + 1] (LDS or global), back-pointers bp [K][L + 1], EL [K] = the keys of E_c(L).
__device__ __forceinline__ void seg_dp_group(uint64_t* prev, uint64_t* cur, const double* __restrict__ tab, int32_t* __restrict__ bp, int L, int W,
                                             int K, uint64_t* EL) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WAVES = SEG_DP_THREADS / 64;
    for (int b = tid; b <= L; b += SEG_DP_THREADS) prev[b] = b == 0 ? seq_key(0.0) : SEQ_UNDEF;
    __syncthreads();
    for (int c = 1; c <= K; ++c) {
        const int from = c == K ? L : c;                                 // the last step: E_K(L) only
        for (int b = tid; b < from; b += SEG_DP_THREADS) cur[b] = SEQ_UNDEF;
        for (int b = from + wave; b <= L; b += WAVES) {
            const int lo = max(c - 1, b - W), nd = b - lo;               // a = b - 1 - d, d = 0 .. nd - 1
            const double* row = tab + (size_t)(b - 1) * W;
            uint64_t key = SEQ_UNDEF, at = ~0ull;
#pragma unroll 4
            for (int d = lane; d < nd; d += 64) {
                const int a = b - 1 - d;
                const uint64_t e = prev[a];
                const double cost = row[d];
                if (e != SEQ_UNDEF) {
                    const uint64_t s = seq_key(seq_cost(e) + cost);
                    if (s < key || (s == key && (uint64_t)a < at)) { key = s; at = (uint64_t)a; }
                }
            }
            seq_wave_min(key, at);
            if (lane == 0) {
                cur[b] = key;
                bp[(size_t)(c - 1) * (L + 1) + b] = key == SEQ_UNDEF ? -1 : (int32_t)at;
            }
        }
        __syncthreads();
        if (tid == 0) EL[c - 1] = cur[L];
        uint64_t* t = prev; prev = cur; cur = t;
    }
    __syncthreads();
}

// ---- grid = the batch's entries.  dynamic LDS: 2 * round_up(longest LDS-form group + 1, 64) keys.  cuts [n_sel][k][2]: each
// chapter's (a, b), for seg_show_kernel ----
__global__ __launch_bounds__(SEG_DP_THREADS)
void seg_dp_kernel(const SegEntry* __restrict__ ent, const double* __restrict__ tab_all, int32_t* __restrict__ bp_all, uint64_t* __restrict__ e_all,
                   const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder, int k, float penalty, int lds_rows, int lds_alloc,
                   int32_t* __restrict__ count_out, int32_t* __restrict__ first_out, int32_t* __restrict__ last_out, int32_t* __restrict__ len_out,
                   float* __restrict__ spread_out, float* __restrict__ mean_out, int32_t* __restrict__ cuts) {
    extern __shared__ __attribute__((aligned(16))) char seg_smem[];
    __shared__ uint64_t EL[SEG_MAX_K];
    __shared__ int kappa_s;
    const SegEntry en = ent[blockIdx.x];
    const int tid = threadIdx.x, L = en.L, W = en.W, K = min(k, L);
    const size_t o = (size_t)en.slot * k;
    const double* tab = tab_all + en.toff;
    int32_t* bp = bp_all + en.bpoff;
    if (L > 0) {                                                         // block-uniform
        if (L <= lds_rows) seg_dp_group((uint64_t*)seg_smem, (uint64_t*)seg_smem + lds_alloc, tab, bp, L, W, K, EL);
        else seg_dp_group(e_all + en.eoff, e_all + en.eoff + (L + 1), tab, bp, L, W, K, EL);
    }
    if (tid == 0) {
        int kappa = 0;
        double best = 0.0;
        for (int c = 1; c <= K; ++c) {
            if (EL[c - 1] == SEQ_UNDEF) continue;
            const double F = seq_cost(EL[c - 1]) + (double)c * (double)penalty;
            if (kappa == 0 || F < best) { kappa = c; best = F; }
        }
        const int32_t* so = sorder + goff[en.group];
        int b = L;
        for (int c = kappa; c >= 1; --c) {
            int a = bp[(size_t)(c - 1) * (L + 1) + b];
            a = min(max(a, max(c - 1, b - W)), b - 1);                   // (a* is admissible; non-finite rows must not lead outside the table)
            const int t = c - 1, len = b - a;
            first_out[o + t] = so[a]; last_out[o + t] = so[b - 1]; len_out[o + t] = len;
            spread_out[o + t] = (float)(tab[(size_t)(b - 1) * W + (len - 1)] / (double)len);
            cuts[2 * (o + t)] = a; cuts[2 * (o + t) + 1] = b;
            b = a;
        }
        count_out[en.slot] = kappa;
        if (mean_out) mean_out[en.slot] = kappa ? (float)(seq_cost(EL[kappa - 1]) / (double)L) : __builtin_inff();
        kappa_s = kappa;
    }
    __syncthreads();
    for (int t = kappa_s + tid; t < k; t += SEG_DP_THREADS) {
        first_out[o + t] = -1; last_out[o + t] = -1; len_out[o + t] = 0; spread_out[o + t] = __builtin_inff();
        cuts[2 * (o + t)] = -1; cuts[2 * (o + t) + 1] = -1;
    }
}

// ---- grid = the batch's entries x k: show_out[slot][t] = the row of chapter t with the smallest (1 - x . u, tie) ----
__global__ __launch_bounds__(SEG_SHOW_THREADS)
void seg_show_kernel(const float* __restrict__ rows, int dim, const int32_t* __restrict__ goff, const int32_t* __restrict__ sorder,
                     const SegEntry* __restrict__ ent, const double* __restrict__ P, const int32_t* __restrict__ cuts, int k, const TieOrder tie,
                     int32_t* __restrict__ show_out) {
    __shared__ __attribute__((aligned(16))) float u[4096];               // dim <= 4096 (vq_index_create)
    __shared__ uint64_t red[SEG_SHOW_THREADS / 64];
    const SegEntry en = ent[blockIdx.x / k];
    const int t = blockIdx.x % k, tid = threadIdx.x;
    const size_t o = (size_t)en.slot * k + t;
    const int a = cuts[2 * o], b = cuts[2 * o + 1];
    if (a < 0) {                                                         // block-uniform: an unused slot
        if (tid == 0) show_out[o] = -1;
        return;
    }
    const double* Pa = P + ((size_t)en.prow + a) * dim;
    const double* Pb = P + ((size_t)en.prow + b) * dim;
    for (int i = tid; i < dim; i += SEG_SHOW_THREADS) u[i] = (float)(Pb[i] - Pa[i]);
    __syncthreads();
    const int32_t* so = sorder + goff[en.group];
    uint64_t key = ~0ull;
    for (int p = a + tid; p < b; p += SEG_SHOW_THREADS) {
        const int r = so[p];
        const float* x = rows + (size_t)r * dim;
        const float d = exact_row_dist(x, u, dim);
        const uint64_t kk = dist_key(d, tie_of(tie, r));
        key = kk < key ? kk : key;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t other = __shfl_xor(key, s);
        key = other < key ? other : key;
    }
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < SEG_SHOW_THREADS / 64; ++w) key = red[w] < key ? red[w] : key;
        show_out[o] = tie_row(tie, (uint32_t)key);
    }
}

// ---- the call's counters: groups that got chapters, and the two figures the host knows ----
__global__ __launch_bounds__(256)
void seg_stats_kernel(const int32_t* __restrict__ count, int n_sel, unsigned long long pairs, unsigned long long batches,
                      unsigned long long* __restrict__ counters) {
    __shared__ int red[4];
    const int tid = threadIdx.x;
    int c = 0;
    for (int i = tid; i < n_sel; i += 256) c += count[i] > 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        counters[0] = (unsigned long long)(red[0] + red[1] + red[2] + red[3]);
        counters[1] = pairs;
        counters[2] = batches;
    }
}

#endif  // __HIPCC__

}  // namespace vq
