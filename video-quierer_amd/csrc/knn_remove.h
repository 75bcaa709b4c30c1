// vq_index_remove_rows (vq_index.hip): stable compaction of the index after rows are taken out.
//
// The host hands over the removed row numbers sorted and unique, rm[0..m).  Row r survives unless it is in rm; its new number
// is newrow[r] = r - (removed rows below r).  Every kernel here is one of three kinds:
//   - maps: newrow[] for every old row, src_of[] (the old row of every new row that moves);
//   - a three-pass exclusive prefix sum over int32 flags (tile sums -> one-workgroup carry -> tile scan), used for the two stable
//     compactions that are not row moves: the rank order (rank_inv) and the by-group row list (grows);
//   - gathers / scatters through those maps into scratch, which the host then copies back over the live arrays.
// Row moves go through bounded scratch (remove_gather_rows_kernel, remove_store_rows_kernel): every row moves DOWN, so an in-place
// pass would read rows another workgroup has already overwritten.  Plain vector memory ops only: no atomics are needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vq {

constexpr int RM_SCAN_TILE = 2048;            // elements per prefix-sum workgroup (256 threads x 8 consecutive)

// number of entries of the sorted list a[0..m) that are < v
__device__ __forceinline__ int64_t rm_lower_bound(const int64_t* __restrict__ a, int64_t m, int64_t v) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// newrow[r] for every old row (-1 = removed); src_of[d - r0] = r for every survivor that moves (new number d >= r0 = rm[0]).
__global__ __launch_bounds__(256)
void remove_row_map_kernel(const int64_t* __restrict__ rm, int64_t m, int64_t n, int64_t r0, int32_t* __restrict__ newrow,
                           int32_t* __restrict__ src_of) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        if (r < r0) { newrow[r] = (int32_t)r; continue; }
        const int64_t j = rm_lower_bound(rm, m, r);
        const bool gone = j < m && rm[j] == r;
        newrow[r] = gone ? -1 : (int32_t)(r - j);
        if (!gone) src_of[r - j - r0] = (int32_t)r;
    }
}

// scratch[i] = rows[src_of[d0 + i]] for the cnt moved rows of one chunk (fp32 master only: the fp16 copy is re-derived from it by
// remove_store_rows_kernel).  One thread per float4.
__global__ __launch_bounds__(256)
void remove_gather_rows_kernel(const float* __restrict__ rows, int dim, const int32_t* __restrict__ src_of, int64_t cnt,
                               float* __restrict__ scratch) {
    const int per_row = dim >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt * per_row; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = i / per_row;
        const int c = (int)(i - d * per_row) * 4;
        *(float4*)(scratch + d * dim + c) = *(const float4*)(rows + (int64_t)src_of[d] * dim + c);
    }
}

// A chunk of gathered rows back into place: fp32 master and its fp16 scan copy, the conversion of rows_to_f16_kernel (so the
// result is bit-identical to what vq_index_add of the survivors stores).  8 floats per thread: two 16-byte loads, two 16-byte
// fp32 stores and one 16-byte fp16 store.  count8 = floats / 8; the host takes this kernel when dim % 8 == 0 (every row then
// starts 16-byte aligned in both copies).
__global__ __launch_bounds__(256)
void remove_store_rows_kernel(const float* __restrict__ src, int64_t count8, float* __restrict__ rows, uint16_t* __restrict__ rows16) {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count8; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = *(const float4*)(src + i * 8), b = *(const float4*)(src + i * 8 + 4);
        *(float4*)(rows + i * 8) = a;
        *(float4*)(rows + i * 8 + 4) = b;
        const h4 ha = {(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w};
        const h4 hb = {(_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
        const uint2 ua = __builtin_bit_cast(uint2, ha), ub = __builtin_bit_cast(uint2, hb);
        *(uint4*)(rows16 + i * 8) = make_uint4(ua.x, ua.y, ub.x, ub.y);
    }
}

// ---- exclusive prefix sum of int32 (in place; out[n] = total) ----
// Exclusive scan of one value per thread over a 256-thread workgroup; *total = the workgroup's sum.
__device__ __forceinline__ int32_t rm_block_excl_scan(int32_t v, int32_t* total) {
    __shared__ int32_t wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int32_t before = 0;
    for (int i = 0; i < w; ++i) before += wsum[i];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();                                  // wsum is reused by the next call
    return before + inc - v;
}

__global__ __launch_bounds__(256)
void rm_scan_tile_sum_kernel(const int32_t* __restrict__ v, int64_t n, int32_t* __restrict__ tile_sum) {
    const int64_t base = (int64_t)blockIdx.x * RM_SCAN_TILE + threadIdx.x * 8;
    int32_t s = 0;
    for (int j = 0; j < 8; ++j)
        if (base + j < n) s += v[base + j];
    int32_t total;
    (void)rm_block_excl_scan(s, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// tile_sum[0..ntiles) -> exclusive prefix, tile_sum[ntiles] = total.  One workgroup, 256 tiles per step.
__global__ __launch_bounds__(256)
void rm_scan_carry_kernel(int32_t* __restrict__ tile_sum, int64_t ntiles) {
    int32_t carry = 0;
    for (int64_t b = 0; b < ntiles; b += 256) {
        const int64_t i = b + threadIdx.x;
        const int32_t v = i < ntiles ? tile_sum[i] : 0;
        int32_t total;
        const int32_t ex = rm_block_excl_scan(v, &total);
        if (i < ntiles) tile_sum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sum[ntiles] = carry;
}

__global__ __launch_bounds__(256)
void rm_scan_apply_kernel(int32_t* __restrict__ v, int64_t n, const int32_t* __restrict__ tile_sum, int64_t ntiles) {
    const int64_t base = (int64_t)blockIdx.x * RM_SCAN_TILE + threadIdx.x * 8;
    int32_t x[8], s = 0;
    for (int j = 0; j < 8; ++j) { x[j] = base + j < n ? v[base + j] : 0; s += x[j]; }
    int32_t total;
    int32_t run = tile_sum[blockIdx.x] + rm_block_excl_scan(s, &total);
    for (int j = 0; j < 8; ++j)
        if (base + j < n) { v[base + j] = run; run += x[j]; }
    if (blockIdx.x == 0 && threadIdx.x == 0) v[n] = tile_sum[ntiles];
}

// f[i] = 1 when the old row a[i] survives (a = rank_inv or grows: lists of old row numbers)
__global__ __launch_bounds__(256)
void remove_survivor_flags_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ newrow, int64_t n, int32_t* __restrict__ f) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        f[i] = newrow[a[i]] >= 0 ? 1 : 0;
}

// Ranks: S = exclusive scan of the survivor flags over the rank order, so a survivor's new rank is S[t] (its old rank t minus the
// removed ranks below it).  rank [new n] is written in place (this kernel reads rank_inv only); rank_inv_new goes to scratch.
__global__ __launch_bounds__(256)
void remove_renumber_ranks_kernel(const int32_t* __restrict__ rank_inv, const int32_t* __restrict__ newrow, const int32_t* __restrict__ S,
                                  int64_t n, int32_t* __restrict__ rank, int32_t* __restrict__ rank_inv_new) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t nr = newrow[rank_inv[t]];
        if (nr < 0) continue;
        rank[nr] = S[t];
        rank_inv_new[S[t]] = nr;
    }
}

// Groups: S = exclusive scan of the survivor flags over grows (S[n] = new n).  keep[g] = the group still holds a row.
__global__ __launch_bounds__(256)
void remove_group_keep_kernel(const int32_t* __restrict__ goff, const int32_t* __restrict__ S, int32_t G, int32_t* __restrict__ keep) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x)
        keep[g] = S[goff[g + 1]] > S[goff[g]] ? 1 : 0;
}

// The new label block in vq_index_set_groups' layout: labels [n_pad'] (-1 past n') | goff [G' + 1] | grows [n'].  K = exclusive
// scan of keep (K[g] = the new number of a kept group g, K[G] = G').  Filtering grows keeps its (group, row) order: the group and
// row renumberings are both monotone.
__global__ __launch_bounds__(256)
void remove_rebuild_groups_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                                  const int32_t* __restrict__ newrow, const int32_t* __restrict__ S, const int32_t* __restrict__ K,
                                  int64_t n, int32_t G, int64_t n_new, int64_t n_pad_new, int32_t* __restrict__ lab_new,
                                  int32_t* __restrict__ goff_new, int32_t* __restrict__ grows_new) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t r = t0; r < n; r += stride) {
        const int32_t nr = newrow[r];
        if (nr >= 0) lab_new[nr] = K[lab[r]];
        if (S[r + 1] > S[r]) grows_new[S[r]] = newrow[grows[r]];
    }
    for (int64_t r = n_new + t0; r < n_pad_new; r += stride) lab_new[r] = -1;
    for (int64_t g = t0; g < G; g += stride)
        if (K[g + 1] > K[g]) goff_new[K[g]] = S[goff[g]];
    if (t0 == 0) goff_new[K[G]] = (int32_t)n_new;
}

// Per 128-row stream the label all its rows share, or -1 (vq_index_set_groups' d_sgroup, read by scan3_group_max_kernel).
__global__ __launch_bounds__(256)
void remove_stream_labels_kernel(const int32_t* __restrict__ lab, int64_t streams, int32_t* __restrict__ sg) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < streams; s += (int64_t)gridDim.x * blockDim.x) {
        const int32_t* l = lab + s * 128;
        const int32_t g = l[0];
        bool same = g >= 0;
        for (int i = 1; i < 128 && same; ++i) same = l[i] == g;
        sg[s] = same ? g : -1;
    }
}

}  // namespace vq
