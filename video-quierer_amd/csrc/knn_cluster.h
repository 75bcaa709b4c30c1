// Library clustering (vq_index_cluster): exact spherical k-means over the stored rows.  include/vq_amd.h has the definition,
// the ORDER of every floating-point operation included; DESIGN.md §4 "Library clustering".  The assignment step of an iteration
// is vq_index_label_rows with the centroids as prompts (knn_label.h, unchanged); this file is the other half, the centroid
// update over the fp32 master, and what surrounds the loop.
//
//   plan_cluster               host only: the piece length, the most pieces a call can have, scratch, launches per iteration
//   cluster_gather_kernel      C_1[j] = stored row init_rows[j]
//   cluster_hist_kernel        per block of 1,024 rows the histogram of their labels; rows whose label changed are counted
//   cluster_prefix_kernel      per label the blocks' counts -> exclusive prefix over the blocks, and the label's total
//   cluster_scan_kernel        one workgroup: counts -> list offsets and piece offsets; the changed count goes to its slot
//   cluster_scatter_kernel     the by-label row list, ascending row within a label (a stable counting sort)
//   cluster_piece_kernel       one workgroup per piece of <= 1,024 list entries: the fp64 column sums of its rows, in list order
//   cluster_finish_kernel      one workgroup per cluster: pieces in order, mean, |mean|^2 chain, square root, division
//   cluster_show_kernel / cluster_show_rows_kernel   per cluster the row with the smallest (best, tie)
//
// The list.  Integers only, so any correct stable method gives the same list; this one is the counting sort the remove path
// and the label call's per-piece histograms already use in parts: a [blocks][P] table of per-block label counts (4 B x P per
// 1,024 rows), turned per label into exclusive prefixes over the blocks, then every block places its rows at
// off[label] + prefix[block][label] + (the number of earlier rows of the block with the same label).  That last term is counted
// against the block's labels in LDS, every lane reading the same four words (a broadcast, no bank conflict).
//
// The sums.  A floating-point sum is defined by its order, and the order is the definition's: a cluster's rows in ascending row
// number, cut into pieces of 1,024; within a piece one fp64 chain per column, the pieces' sums added in piece order.  So no
// floating-point atomics and no tree anywhere.  The pieces are what makes the pass parallel whatever P is: n / 1,024 + P
// workgroups at most, also for P = 1.  A thread owns four adjacent columns (one 16-byte load per row and lane, a wave reads
// 1 KiB of a row contiguously) and runs their four chains; eight rows' loads are issued before the eight dependent adds.  The
// grid is the plan's bound (the device form reads nothing back); a workgroup beyond the call's pieces leaves at once.
//
// Contraction.  The library is built with -ffp-contract=on.  The piece and finish kernels hold additions, one division, one
// square root and the products m[i] * m[i] of two fp32 values widened to fp64: those products are exact (48 significant bits),
// so fma(m, m, s) and the rounded product added to s are the same number.  Nothing else can be contracted.
//
// Stores are plain vector stores; global atomics (integer): the changed count, the clusters' show keys.
#pragma once
#include "vq_common.h"
#include "knn_kernels.h"

#include <algorithm>

namespace vq {

constexpr int CL_MAX_P = 4096;                       // clusters per call (= vq_index_label_rows' prompts)
constexpr int CL_MAX_ITER = 1000;
constexpr int CL_PIECE = 1024;                       // list entries per piece of the sum (part of the definition)
constexpr int CL_BLOCK_ROWS = 1024;                  // rows per block of the counting sort
constexpr int CL_UNROLL = 8;                         // rows in flight per lane of the piece kernel
constexpr int CL_LAUNCHES = 6;                       // hist, prefix, scan, scatter, piece, finish
constexpr int CL_CTL_WORDS = 16;                     // ctl[0] changed rows (accumulator), ctl[1] pieces of this list

struct ClusterPlan {
    int piece_rows;
    int64_t max_pieces;       // the piece kernel's grid: floor(n / 1,024) + min(P, n) bounds sum_j ceil(cnt_j / 1,024)
    int64_t blocks;           // blocks of the counting sort
    int64_t table_bytes;      // [blocks][P] counts
    int64_t sum_bytes;        // [max_pieces][dim] fp64
    int64_t scratch_bytes;    // both, and the words (previous labels, labels, distances, list, counts, offsets, show keys)
    int piece_threads;        // dim / 4 rounded up to whole waves
    int launches;             // per iteration, the assignment aside
};

inline ClusterPlan plan_cluster(int64_t n, int dim, int P) {
    ClusterPlan p;
    p.piece_rows = CL_PIECE;
    p.max_pieces = n / CL_PIECE + std::min<int64_t>(P, n);
    p.blocks = (n + CL_BLOCK_ROWS - 1) / CL_BLOCK_ROWS;
    p.table_bytes = p.blocks * P * 4;
    p.sum_bytes = p.max_pieces * dim * 8;
    p.scratch_bytes = p.table_bytes + p.sum_bytes + 4 * (CL_CTL_WORDS + 4 * round_up(n, 4) + 5 * round_up((int64_t)P + 1, 4)) + 8 * (int64_t)P;
    p.piece_threads = (int)round_up(dim / 4, 64);
    p.launches = CL_LAUNCHES;
    return p;
}

#ifdef __HIPCC__

// ---- C_1[j] = row init_rows[j] (an entry outside [0, n) is the caller's error; it is clamped so that nothing is read out of bounds) ----
__global__ __launch_bounds__(256)
void cluster_gather_kernel(const float* __restrict__ rows, int64_t n, int dim, const int32_t* __restrict__ init_rows, float* __restrict__ C) {
    const int j = blockIdx.x;
    int64_t r = init_rows[j];
    r = r < 0 ? 0 : (r >= n ? n - 1 : r);
    const float4* src = (const float4*)(rows + (size_t)r * dim);
    float4* dst = (float4*)(C + (size_t)j * dim);
    for (int i = threadIdx.x; i < dim / 4; i += 256) dst[i] = src[i];
}

// ---- block b: table[b][j] = its rows with label j; ctl[0] += its rows with lab != prev (first: all of them); prev = lab.
// A label outside [0, P) is counted nowhere (the label call writes none; the debug hook checks its input). ----
__global__ __launch_bounds__(256)
void cluster_hist_kernel(const int32_t* __restrict__ lab, int32_t* __restrict__ prev, int64_t n, int P, int first,
                         uint32_t* __restrict__ table, int32_t* __restrict__ ctl) {
    __shared__ uint32_t hist[CL_MAX_P];
    __shared__ int changed_s;
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * CL_BLOCK_ROWS;
    for (int j = tid; j < P; j += 256) hist[j] = 0u;
    if (tid == 0) changed_s = 0;
    __syncthreads();
    int changed = 0;
#pragma unroll
    for (int k = 0; k < CL_BLOCK_ROWS / 256; ++k) {
        const int64_t r = r0 + k * 256 + tid;
        if (r < n) {
            const int32_t L = lab[r];
            if ((uint32_t)L < (uint32_t)P) atomicAdd(&hist[L], 1u);
            changed += (first || prev[r] != L) ? 1 : 0;
            prev[r] = L;
        }
    }
    if (changed) atomicAdd(&changed_s, changed);
    __syncthreads();
    uint32_t* out = table + (size_t)blockIdx.x * P;
    for (int j = tid; j < P; j += 256) out[j] = hist[j];
    if (tid == 0 && changed_s) atomicAdd(ctl, changed_s);
}

// ---- thread j: table[b][j] -> the count of label j in the blocks before b; cnt[j] = its total ----
__global__ __launch_bounds__(256)
void cluster_prefix_kernel(uint32_t* __restrict__ table, int64_t blocks, int P, int32_t* __restrict__ cnt) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    uint32_t run = 0u;
    uint32_t* at = table + j;
    int64_t b = 0;
    for (; b + 8 <= blocks; b += 8, at += (size_t)8 * P) {               // eight loads in flight before the dependent stores
        uint32_t c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = at[(size_t)u * P];
#pragma unroll
        for (int u = 0; u < 8; ++u) { at[(size_t)u * P] = run; run += c[u]; }
    }
    for (; b < blocks; ++b, at += P) {
        const uint32_t c = *at;
        *at = run;
        run += c;
    }
    cnt[j] = (int32_t)run;
}

// ---- one workgroup of 1,024 threads: off[j] = rows of the labels below j, poff[j] = their pieces (both [P + 1]); skey[j] = "no
// row"; counts_out (or null) = cnt; ctl[1] = pieces; the changed count moves from ctl[0] to *changed_out (or nowhere) ----
__global__ __launch_bounds__(1024)
void cluster_scan_kernel(const int32_t* __restrict__ cnt, int P, int32_t* __restrict__ off, int32_t* __restrict__ poff,
                         unsigned long long* __restrict__ skey, int32_t* __restrict__ counts_out, int32_t* __restrict__ ctl,
                         int32_t* __restrict__ changed_out) {
    __shared__ int32_t part_rows[1024], part_pieces[1024];
    const int tid = threadIdx.x;
    const int j0 = tid * 4;
    int32_t c[4], rows = 0, pieces = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c[e] = j0 + e < P ? cnt[j0 + e] : 0;
        rows += c[e];
        pieces += (c[e] + CL_PIECE - 1) / CL_PIECE;
    }
    part_rows[tid] = rows; part_pieces[tid] = pieces;
    __syncthreads();
    if (tid == 0) {
        int32_t rr = 0, pp = 0;
        const int used = (P + 3) / 4;
        for (int t = 0; t < used; ++t) {
            const int32_t a = part_rows[t], b = part_pieces[t];
            part_rows[t] = rr; part_pieces[t] = pp;
            rr += a; pp += b;
        }
        off[P] = rr; poff[P] = pp;
        ctl[1] = pp;
        if (changed_out) *changed_out = ctl[0];
        ctl[0] = 0;
    }
    __syncthreads();
    rows = part_rows[tid]; pieces = part_pieces[tid];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (j0 + e < P) {
            off[j0 + e] = rows; poff[j0 + e] = pieces;
            skey[j0 + e] = ~0ull;
            if (counts_out) counts_out[j0 + e] = c[e];
        }
        rows += c[e];
        pieces += (c[e] + CL_PIECE - 1) / CL_PIECE;
    }
}

// ---- block b places its rows: list[off[L] + table[b][L] + earlier rows of the block with label L] = row ----
__global__ __launch_bounds__(256)
void cluster_scatter_kernel(const int32_t* __restrict__ lab, int64_t n, int P, const uint32_t* __restrict__ table,
                            const int32_t* __restrict__ off, int32_t* __restrict__ list) {
    __shared__ __attribute__((aligned(16))) int32_t labs[CL_BLOCK_ROWS];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * CL_BLOCK_ROWS;
    const int here = (int)min((int64_t)CL_BLOCK_ROWS, n - r0);          // rows of this block (>= 1)
    int32_t mine[CL_BLOCK_ROWS / 256];
#pragma unroll
    for (int k = 0; k < CL_BLOCK_ROWS / 256; ++k) {
        const int i = k * 256 + tid;
        mine[k] = i < here ? lab[r0 + i] : -1;
        labs[i] = mine[k];
    }
    __syncthreads();
    int rank[CL_BLOCK_ROWS / 256];
#pragma unroll
    for (int k = 0; k < CL_BLOCK_ROWS / 256; ++k) {                      // row k * 256 + tid against the rows before it
        const int me = k * 256 + tid, L = mine[k];                       // (words past `here` hold -1: never a placed row's label)
        int r = 0;
        for (int i = 0; i < k * 256; i += 4) {                           // whole chunks before this row's: every lane reads the same four words
            const int4 v = *(const int4*)(labs + i);
            r += (v.x == L ? 1 : 0) + (v.y == L ? 1 : 0) + (v.z == L ? 1 : 0) + (v.w == L ? 1 : 0);
        }
        for (int i = k * 256; i < (k + 1) * 256; i += 4) {               // its own chunk: only the rows before it
            const int4 v = *(const int4*)(labs + i);
            r += (v.x == L && i < me ? 1 : 0) + (v.y == L && i + 1 < me ? 1 : 0) + (v.z == L && i + 2 < me ? 1 : 0) + (v.w == L && i + 3 < me ? 1 : 0);
        }
        rank[k] = r;
    }
    const uint32_t* pre = table + (size_t)blockIdx.x * P;
#pragma unroll
    for (int k = 0; k < CL_BLOCK_ROWS / 256; ++k) {
        const int i = k * 256 + tid;
        if (i < here && (uint32_t)mine[k] < (uint32_t)P) list[(int64_t)off[mine[k]] + pre[mine[k]] + rank[k]] = (int32_t)(r0 + i);
    }
}

// the cluster of piece p: the last j with poff[j] <= p (poff [P + 1] ascending, poff[P] > p)
__device__ __forceinline__ int cluster_of_piece(const int32_t* __restrict__ poff, int P, int p) {
    int lo = 0, hi = P;                                                  // poff[lo] <= p < poff[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (poff[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- one workgroup per piece; thread t owns columns 4 t .. 4 t + 3.  psum [pieces][dim] ----
__global__ __launch_bounds__(1024)
void cluster_piece_kernel(const float* __restrict__ rows, int dim, int P, const int32_t* __restrict__ list, const int32_t* __restrict__ off,
                          const int32_t* __restrict__ poff, const int32_t* __restrict__ ctl, double* __restrict__ psum) {
    const int p = blockIdx.x;
    if (p >= ctl[1]) return;                                             // block-uniform: beyond this list's pieces
    const int j = cluster_of_piece(poff, P, p);
    const int64_t b = (int64_t)off[j] + (int64_t)(p - poff[j]) * CL_PIECE;
    const int64_t e = min(b + CL_PIECE, (int64_t)off[j + 1]);
    const int c0 = threadIdx.x * 4;
    if (c0 >= dim) return;
    const float* base = rows + c0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t i = b;
    for (; i + CL_UNROLL <= e; i += CL_UNROLL) {
        float4 v[CL_UNROLL];
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) v[u] = *(const float4*)(base + (size_t)list[i + u] * dim);
#pragma unroll
        for (int u = 0; u < CL_UNROLL; ++u) { s0 += (double)v[u].x; s1 += (double)v[u].y; s2 += (double)v[u].z; s3 += (double)v[u].w; }
    }
    for (; i < e; ++i) {
        const float4 v = *(const float4*)(base + (size_t)list[i] * dim);
        s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
    }
    double* out = psum + (size_t)p * dim + c0;
    *(double2*)out = double2{s0, s1};
    *(double2*)(out + 2) = double2{s2, s3};
}

// ---- one workgroup per cluster: C[j] <- normalised mean of its rows, or untouched (no row / a zero mean).  In place: cluster
// j's workgroup is the only reader and writer of C[j]. ----
__global__ __launch_bounds__(256)
void cluster_finish_kernel(const double* __restrict__ psum, int dim, const int32_t* __restrict__ off, const int32_t* __restrict__ poff,
                           float* __restrict__ C) {
    __shared__ float m[4096];                                            // dim <= 4096 (vq_index_create)
    const int j = blockIdx.x, tid = threadIdx.x;
    const int cnt = off[j + 1] - off[j];
    if (cnt == 0) return;                                                // block-uniform
    const int p0 = poff[j], p1 = poff[j + 1];
    const double denom = (double)cnt;
    for (int i = tid; i < dim; i += 256) {
        double s = 0.0;
        for (int p = p0; p < p1; ++p) s += psum[(size_t)p * dim + i];
        m[i] = (float)(s / denom);
    }
    __syncthreads();
    double n2 = 0.0;                                                     // every thread runs the same chain: no broadcast needed
    for (int i = 0; i < dim; ++i) {
        const double v = (double)m[i];
        n2 += v * v;                                                     // exact product: contraction cannot change the sum
    }
    if (n2 == 0.0) return;
    const double len = __builtin_sqrt(n2);
    float* out = C + (size_t)j * dim;
    for (int i = tid; i < dim; i += 256) out[i] = (float)((double)m[i] / len);
}

// ---- one workgroup per piece: skey[cluster] = min(skey[cluster], smallest (best, tie) key of the piece's rows) ----
__global__ __launch_bounds__(256)
void cluster_show_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ off, const int32_t* __restrict__ poff, int P,
                         const int32_t* __restrict__ ctl, const float* __restrict__ best, const TieOrder tie,
                         unsigned long long* __restrict__ skey) {
    __shared__ unsigned long long red[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (p >= ctl[1]) return;
    const int j = cluster_of_piece(poff, P, p);
    const int64_t b = (int64_t)off[j] + (int64_t)(p - poff[j]) * CL_PIECE;
    const int64_t e = min(b + CL_PIECE, (int64_t)off[j + 1]);
    unsigned long long key = ~0ull;
    for (int64_t i = b + tid; i < e; i += 256) {
        const int r = list[i];
        const unsigned long long k = dist_key(best[r], tie_of(tie, r));
        key = k < key ? k : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) atomicMin(&skey[j], min(min(red[0], red[1]), min(red[2], red[3])));
}

__global__ __launch_bounds__(256)
void cluster_show_rows_kernel(const unsigned long long* __restrict__ skey, int P, const TieOrder tie, int32_t* __restrict__ show) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P) return;
    const unsigned long long k = skey[j];
    show[j] = k == ~0ull ? -1 : tie_row(tie, (uint32_t)k);
}

#endif  // __HIPCC__

}  // namespace vq
