// Frame preprocessing upstream of the encoder: Pillow's separable 8-bit resample
// (src/libImaging/Resample.c) as two integer passes, and the frame-quality statistics of
// reference src/core/frame_extractor.py:301-316.  Byte/integer work, HBM-bound: a source frame is read once
// (staged through LDS row by row), the uint8 intermediate is the only extra traffic.
#pragma once
#include "vq_common.h"

namespace vq {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;       // Resample.c PRECISION_BITS: 22-bit fixed-point weights
constexpr int RS_THREADS = 256;

__device__ __forceinline__ uint8_t rs_clip8(int v) {
    v >>= RS_PRECISION_BITS;                          // arithmetic shift, as clip8() does
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// Horizontal pass (ImagingResampleHorizontal_8bpc, 3 bands).
// A workgroup (4 waves) owns RSH_ROWS = 64 source rows x one segment of `oc` output columns.  It stages the
// source bytes those columns touch into LDS, one dword-aligned row per LDS row (row pitch an odd number of
// dwords), then LANE = ROW: a wave takes output columns of the segment in turn, so the tap window and the
// weights are wave-uniform (the weights sit in LDS, read as broadcasts) and every lane streams consecutive dwords of its own row,
// bank-conflict free.  Four taps = 12 bytes = three dwords, realigned with v_alignbyte by the row's byte
// offset; each byte costs one extract and one multiply-add.  Results go through an LDS tile so the global
// stores are row-contiguous.
//   src  [n][h][w][3]; the pass covers source rows [row_first, row_first + rows_needed) of every frame
//   tmp  [n][rows_needed][out_cols][3] for output columns [col_first, col_first + out_cols)
//   kk rows are `ksize` ints, ksize a multiple of 4, zero beyond the tap count
// oc, pitch_dw, tile_pitch, the LDS bytes and the grid are plan_resample's (preproc_plan.h, which computes with RP_ROWS = RSH_ROWS)
constexpr int RSH_ROWS = 64;
typedef __attribute__((address_space(3))) void rs_lds_t;
typedef const __attribute__((address_space(1))) void rs_gbl_t;

template <bool DWORD_STORE>
__global__ __launch_bounds__(RS_THREADS)
void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp,
                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                       int h, int w, int row_first, int rows_needed, int col_first, int out_cols,
                       int oc, int pitch_dw, int tile_pitch) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
    uint8_t* tile = (uint8_t*)(lds32 + RSH_ROWS * pitch_dw);        // [64][tile_pitch] bytes
    int* kl = (int*)(tile + RSH_ROWS * tile_pitch);                  // [oc][ksize] weights of this segment's columns
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int img = blockIdx.z, r0 = blockIdx.y * RSH_ROWS;
    const int xo0 = blockIdx.x * oc, ncol = min(oc, out_cols - xo0);
    const int xx0 = col_first + xo0;
    const int sx0 = bounds[2 * xx0];                                 // first source pixel the segment touches
    const int sx1 = bounds[2 * (xx0 + ncol - 1)] + bounds[2 * (xx0 + ncol - 1) + 1];
    const int span_bytes = (sx1 - sx0) * 3;
    const size_t pitch = (size_t)w * 3;
    const uint8_t* seg0 = src + ((size_t)img * h + row_first) * pitch + (size_t)sx0 * 3;

    // ---- stage: wave w copies rows w, w+4, ... with LDS-DMA dword loads (64 lanes -> 64 consecutive LDS dwords,
    // no VGPR round trip).  A row starts at the aligned dword that holds its first byte; an aligned dword that
    // contains a valid byte never leaves that byte's page, so the up-to-3 bytes read before / after the span
    // are harmless. ----
    for (int rr = wave; rr < RSH_ROWS; rr += 4) {
        const int row = min(r0 + rr, rows_needed - 1);               // rows past the end repeat the last one, never stored
        const uint8_t* g = seg0 + (size_t)row * pitch;
        const int a = (int)((uintptr_t)g & 3);
        const uint8_t* ga = g - a;
        const int nd = (a + span_bytes + 3) >> 2;
        for (int j0 = 0; j0 < nd; j0 += 64)
            if (j0 + lane < nd)
                __builtin_amdgcn_global_load_lds((rs_gbl_t*)(ga + 4 * (size_t)(j0 + lane)),
                                                 (rs_lds_t*)(lds32 + rr * pitch_dw + j0), 4, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int i = threadIdx.x; i < ncol * ksize; i += RS_THREADS) kl[i] = kk[(size_t)xx0 * ksize + i];
    __syncthreads();

    // ---- compute: lane = row ----
    const int my_row = min(r0 + lane, rows_needed - 1);
    const int a = (int)((uintptr_t)(seg0 + (size_t)my_row * pitch) & 3);
    const uint32_t* rowp = lds32 + lane * pitch_dw;
    for (int c = wave; c < ncol; c += 4) {
        const int xx = xx0 + c;
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const int4* k = (const int4*)(kl + c * ksize);              // wave-uniform address: an LDS broadcast read
        const int off = a + (xmin - sx0) * 3;
        int di = off >> 2;
        const int sh = off & 3;
        int s0 = 1 << (RS_PRECISION_BITS - 1), s1 = s0, s2 = s0;
        uint32_t d0 = rowp[di];
        const int nchunk = (cnt + 3) >> 2;
        for (int q = 0; q < nchunk; ++q) {
            const uint32_t d1 = rowp[di + 1], d2 = rowp[di + 2], d3 = rowp[di + 3];
            const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
            const uint32_t e1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
            const uint32_t e2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
            const int4 kq = k[q];
            const int k0 = kq.x, k1 = kq.y, k2 = kq.z, k3 = kq.w;
            // weights are 23-bit signed, pixels 8-bit: v_mad_i32_i24 (full rate) instead of a 32-bit multiply
            s0 += __mul24((int)(e0 & 255), k0);         s1 += __mul24((int)((e0 >> 8) & 255), k0);  s2 += __mul24((int)((e0 >> 16) & 255), k0);
            s0 += __mul24((int)(e0 >> 24), k1);         s1 += __mul24((int)(e1 & 255), k1);         s2 += __mul24((int)((e1 >> 8) & 255), k1);
            s0 += __mul24((int)((e1 >> 16) & 255), k2); s1 += __mul24((int)(e1 >> 24), k2);         s2 += __mul24((int)(e2 & 255), k2);
            s0 += __mul24((int)((e2 >> 8) & 255), k3);  s1 += __mul24((int)((e2 >> 16) & 255), k3); s2 += __mul24((int)(e2 >> 24), k3);
            d0 = d3;
            di += 3;
        }
        uint8_t* o = tile + lane * tile_pitch + c * 3;
        o[0] = rs_clip8(s0); o[1] = rs_clip8(s1); o[2] = rs_clip8(s2);
    }
    __syncthreads();

    // ---- store the 64 x ncol tile, row-contiguous ----
    const int rows = min(RSH_ROWS, rows_needed - r0);
    uint8_t* out0 = tmp + (((size_t)img * rows_needed + r0) * out_cols + xo0) * 3;
    const size_t out_pitch = (size_t)out_cols * 3;
    if constexpr (DWORD_STORE) {
        const int nd = (ncol * 3) >> 2;                              // <= 24 dwords: half a wave per row
        const int j = lane & 31;
        for (int r = wave * 2 + (lane >> 5); r < rows; r += 8)
            if (j < nd) *(uint32_t*)(out0 + r * out_pitch + 4 * j) = *(const uint32_t*)(tile + r * tile_pitch + 4 * j);
    } else {
        const int nb = ncol * 3;
        for (int r = wave; r < rows; r += 4)
            for (int j = lane; j < nb; j += 64) out0[r * out_pitch + j] = tile[r * tile_pitch + j];
    }
}

// Horizontal pass, row-block-major form.  Measured on resample_h_kernel with s_memtime stamps (1080p -> 224, 64 frames):
// of a workgroup's 23-26k cycles, 11-14k go to ISSUING its 48 LDS-DMA requests per wave — the requests queue behind a
// memory system that serves this pattern (a ~570-byte piece of each of 64 rows 5,760 bytes apart, per workgroup, with
// the pieces of one row spread over workgroups on different XCDs) at ~2 TB/s — and 6.8k to the multiply-adds.  Here a
// workgroup keeps its RSH_ROWS rows and walks `spw` consecutive column segments left to right: what it asks for next
// continues where its last request ended (the halo lines of a segment boundary are in its XCD's L2), a row's span is
// ONE wave-wide request of aligned 16-byte loads held in registers, and the next segment's pixels and weights are in
// flight while the current one is multiplied.  Same LDS image, lane = row compute loop and tile store as above.
template <bool DWORD_STORE>
__global__ __launch_bounds__(RS_THREADS)
void resample_hx_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ tmp,
                        const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                        int h, int w, int row_first, int rows_needed, int col_first, int out_cols,
                        int oc, int pitch_dw, int tile_pitch, int spw /* segments per workgroup */) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds32[];
    uint8_t* tile = (uint8_t*)(lds32 + RSH_ROWS * pitch_dw);        // [64][tile_pitch] bytes
    int* kl = (int*)(tile + RSH_ROWS * tile_pitch);                  // [oc][ksize] weights of the current segment's columns
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int img = blockIdx.z, r0 = blockIdx.y * RSH_ROWS;
    const int nseg = (out_cols + oc - 1) / oc;
    const int s_begin = blockIdx.x * spw, s_end = min(nseg, s_begin + spw);
    const size_t pitch = (size_t)w * 3;
    const uint8_t* frame = src + ((size_t)img * h + row_first) * pitch;

    uint4 v[RSH_ROWS / 4];
    int kw[4];                                                       // plan_resample: oc * ksize <= RP_HX_KW * RS_THREADS
    auto issue = [&](int sg) {                                       // segment sg: pixels of rows w, w+4, ... and its weights -> registers
        const int xo0 = sg * oc, ncol = min(oc, out_cols - xo0), xx0 = col_first + xo0;
        const int sx0 = bounds[2 * xx0];
        const int span_bytes = (bounds[2 * (xx0 + ncol - 1)] + bounds[2 * (xx0 + ncol - 1) + 1] - sx0) * 3;
#pragma unroll
        for (int i = 0; i < RSH_ROWS / 4; ++i) {
            const int row = min(r0 + wave + 4 * i, rows_needed - 1);     // rows past the end repeat the last one, never stored
            const uint8_t* g = frame + (size_t)row * pitch + (size_t)sx0 * 3;
            const int a = (int)((uintptr_t)g & 15);
            v[i] = uint4{0u, 0u, 0u, 0u};
            // an aligned 16-byte chunk that holds a valid byte never leaves that byte's page
            if (lane < ((a + span_bytes + 15) >> 4)) v[i] = *(const uint4*)(g - a + 16 * (size_t)lane);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = (int)threadIdx.x + RS_THREADS * u;
            kw[u] = idx < ncol * ksize ? kk[(size_t)xx0 * ksize + idx] : 0;
        }
    };
    if (s_begin < s_end) issue(s_begin);
    for (int sg = s_begin; sg < s_end; ++sg) {
        const int xo0 = sg * oc, ncol = min(oc, out_cols - xo0), xx0 = col_first + xo0;
        const int sx0 = bounds[2 * xx0];
        if (4 * lane < pitch_dw - 3) {
#pragma unroll
            for (int i = 0; i < RSH_ROWS / 4; ++i) {
                uint32_t* d = lds32 + (wave + 4 * i) * pitch_dw + 4 * lane;
                d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = (int)threadIdx.x + RS_THREADS * u;
            if (idx < oc * ksize) kl[idx] = kw[u];
        }
        __syncthreads();                                             // segment staged; every wave is done with the previous tile
        if (sg + 1 < s_end) issue(sg + 1);

        // ---- compute: lane = row ----
        const int my_row = min(r0 + lane, rows_needed - 1);
        const int a = (int)((uintptr_t)(frame + (size_t)my_row * pitch + (size_t)sx0 * 3) & 15);
        const uint32_t* rowp = lds32 + lane * pitch_dw;
        for (int c = wave; c < ncol; c += 4) {
            const int xx = xx0 + c;
            const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
            const int4* k = (const int4*)(kl + c * ksize);          // wave-uniform address: an LDS broadcast read
            const int off = a + (xmin - sx0) * 3;
            int di = off >> 2;
            const int sh = off & 3;
            int s0 = 1 << (RS_PRECISION_BITS - 1), s1 = s0, s2 = s0;
            uint32_t d0 = rowp[di];
            const int nchunk = (cnt + 3) >> 2;
            for (int q = 0; q < nchunk; ++q) {
                const uint32_t d1 = rowp[di + 1], d2 = rowp[di + 2], d3 = rowp[di + 3];
                const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
                const uint32_t e1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
                const uint32_t e2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
                const int4 kq = k[q];
                const int k0 = kq.x, k1 = kq.y, k2 = kq.z, k3 = kq.w;
                s0 += __mul24((int)(e0 & 255), k0);         s1 += __mul24((int)((e0 >> 8) & 255), k0);  s2 += __mul24((int)((e0 >> 16) & 255), k0);
                s0 += __mul24((int)(e0 >> 24), k1);         s1 += __mul24((int)(e1 & 255), k1);         s2 += __mul24((int)((e1 >> 8) & 255), k1);
                s0 += __mul24((int)((e1 >> 16) & 255), k2); s1 += __mul24((int)(e1 >> 24), k2);         s2 += __mul24((int)(e2 & 255), k2);
                s0 += __mul24((int)((e2 >> 8) & 255), k3);  s1 += __mul24((int)((e2 >> 16) & 255), k3); s2 += __mul24((int)(e2 >> 24), k3);
                d0 = d3;
                di += 3;
            }
            uint8_t* o = tile + lane * tile_pitch + c * 3;
            o[0] = rs_clip8(s0); o[1] = rs_clip8(s1); o[2] = rs_clip8(s2);
        }
        __syncthreads();

        // ---- store the 64 x ncol tile, row-contiguous ----
        const int rows = min(RSH_ROWS, rows_needed - r0);
        uint8_t* out0 = tmp + (((size_t)img * rows_needed + r0) * out_cols + xo0) * 3;
        const size_t out_pitch = (size_t)out_cols * 3;
        if constexpr (DWORD_STORE) {
            const int nd = (ncol * 3) >> 2;                          // <= 24 dwords: half a wave per row
            const int j = lane & 31;
            for (int r = wave * 2 + (lane >> 5); r < rows; r += 8)
                if (j < nd) *(uint32_t*)(out0 + r * out_pitch + 4 * j) = *(const uint32_t*)(tile + r * tile_pitch + 4 * j);
        } else {
            const int nb = ncol * 3;
            for (int r = wave; r < rows; r += 4)
                for (int j = lane; j < nb; j += 64) out0[r * out_pitch + j] = tile[r * tile_pitch + j];
        }
    }
}

// Vertical pass (ImagingResampleVertical_8bpc).  A thread produces VEC consecutive bytes of one output row: 16 when
// rows are 16-byte aligned (one wide load per tap, all taps independent: the pass is latency-bound on its ~11 taps),
// else 4 or 1.  tmp [n][rows_in][row_bytes], dst [n][out_rows][row_bytes] for output rows [row_first, row_first +
// out_rows); `row_shift` is the source row that tmp row 0 corresponds to.
// Each clipped byte goes through an opaque register move before packing: ROCm 7.2's backend otherwise folds
// clamp(x >> 22) pairs into v_ashr_pk_u8_i32, whose upper destination half it does not clear (bytes 2-3 of the
// packed dword came out as stale register contents on gfx950).
__device__ __forceinline__ uint32_t rs_pack4(int s0, int s1, int s2, int s3) {
    uint32_t b0 = rs_clip8(s0), b1 = rs_clip8(s1), b2 = rs_clip8(s2), b3 = rs_clip8(s3);
    asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

template <int VEC>
__global__ __launch_bounds__(RS_THREADS)
void resample_v_kernel(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ dst,
                       const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                       int rows_in, int row_bytes, int row_first, int out_rows, int row_shift) {
    const int img = blockIdx.z;
    int j, yo;
    if constexpr (VEC == 16) {                                      // threads cover (output row, 16-byte chunk) pairs
        const int per_row = row_bytes >> 4;
        const int idx = blockIdx.x * RS_THREADS + threadIdx.x;
        yo = idx / per_row;
        j = (idx - yo * per_row) << 4;
        if (yo >= out_rows) return;
    } else {
        j = (blockIdx.x * RS_THREADS + threadIdx.x) * VEC;
        yo = blockIdx.y;
        if (j >= row_bytes) return;
    }
    const int yy = row_first + yo;
    const int ymin = bounds[2 * yy] - row_shift, cnt = bounds[2 * yy + 1];
    const int* k = kk + (size_t)yy * ksize;
    const uint8_t* p = tmp + ((size_t)img * rows_in + ymin) * row_bytes + j;
    uint8_t* o = dst + ((size_t)img * out_rows + yo) * row_bytes + j;
    if constexpr (VEC == 16) {
        int s[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) {
            const uint4 v = *(const uint4*)(p + (size_t)t * row_bytes);
            const int c = k[t];
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                s[4 * d] += __mul24((int)(w4[d] & 255), c);             s[4 * d + 1] += __mul24((int)((w4[d] >> 8) & 255), c);
                s[4 * d + 2] += __mul24((int)((w4[d] >> 16) & 255), c); s[4 * d + 3] += __mul24((int)(w4[d] >> 24), c);
            }
        }
        *(uint4*)o = uint4{rs_pack4(s[0], s[1], s[2], s[3]), rs_pack4(s[4], s[5], s[6], s[7]),
                           rs_pack4(s[8], s[9], s[10], s[11]), rs_pack4(s[12], s[13], s[14], s[15])};
    } else if constexpr (VEC == 4) {
        int s0 = 1 << (RS_PRECISION_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
        for (int t = 0; t < cnt; ++t) {
            const uint32_t v = *(const uint32_t*)(p + (size_t)t * row_bytes);
            const int c = k[t];
            s0 += __mul24((int)(v & 255), c); s1 += __mul24((int)((v >> 8) & 255), c); s2 += __mul24((int)((v >> 16) & 255), c); s3 += __mul24((int)(v >> 24), c);
        }
        *(uint32_t*)o = rs_pack4(s0, s1, s2, s3);
    } else {
        int s = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) s += __mul24((int)p[(size_t)t * row_bytes], k[t]);
        *o = rs_clip8(s);
    }
}

// ---- cv2.resize(frame, (w, h)), INTER_LINEAR, 8-bit (reference frame_extractor.py:283-284) --------------
// OpenCV's two-tap fixed-point bilinear: 11-bit weights, 32-bit horizontal sums, the VResizeLinear<uchar>
// rounding.  No antialiasing, so a thread reads 4 source pixels per output pixel: one thread per output byte.
//   xofs/yofs: first tap per output column / row; wx, wy: the two short weights per column / row
//   out [n][crop_h][crop_w][3] = window (crop_top, crop_left) of the resized frame
__global__ __launch_bounds__(RS_THREADS)
void cv_resize_linear_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                             const int* __restrict__ xofs, const int* __restrict__ wx,
                             const int* __restrict__ yofs, const int* __restrict__ wy,
                             int h, int w, int crop_top, int crop_left, int crop_h, int crop_w) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;            // byte inside the output row
    const int yo = blockIdx.y, img = blockIdx.z;
    if (j >= crop_w * 3) return;
    const int xo = j / 3, c = j - xo * 3;
    const int dx = crop_left + xo, dy = crop_top + yo;
    const int sx = xofs[dx], sx1 = min(sx + 1, w - 1);
    const int a0 = wx[2 * dx], a1 = wx[2 * dx + 1];
    const int sy = yofs[dy];
    const int y0 = min(max(sy, 0), h - 1), y1 = min(max(sy + 1, 0), h - 1);
    const int b0 = wy[2 * dy], b1 = wy[2 * dy + 1];
    const uint8_t* f = src + (size_t)img * h * w * 3;
    const uint8_t* r0 = f + (size_t)y0 * w * 3;
    const uint8_t* r1 = f + (size_t)y1 * w * 3;
    const int d0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
    const int d1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
    const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
    dst[((size_t)img * crop_h + yo) * crop_w * 3 + j] = (uint8_t)v;
}

// exact 2x2 down-scale: cv2 routes INTER_LINEAR to INTER_AREA's fast path, (a + b + c + d + 2) >> 2
__global__ __launch_bounds__(RS_THREADS)
void cv_resize_half_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                           int h, int w, int crop_top, int crop_left, int crop_h, int crop_w) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    const int yo = blockIdx.y, img = blockIdx.z;
    if (j >= crop_w * 3) return;
    const int xo = j / 3, c = j - xo * 3;
    const uint8_t* p = src + (((size_t)img * h + 2 * (crop_top + yo)) * w + 2 * (crop_left + xo)) * 3 + c;
    const size_t pitch = (size_t)w * 3;
    dst[((size_t)img * crop_h + yo) * crop_w * 3 + j] = (uint8_t)((p[0] + p[3] + p[pitch] + p[pitch + 3] + 2) >> 2);
}

// ---- frame quality (reference frame_extractor.py:301-316) ------------------------------------------------
// per frame: sum of all bytes (np.mean(frame)), and over the grey image g = BGR2GRAY(frame) the sums of
// L and L^2 where L = cv2.Laplacian(g, CV_64F) (aperture 1: the 4-neighbour stencil, BORDER_REFLECT_101).
// Grey conversion: OpenCV 4.x fixed point, (B*3735 + G*19235 + R*9798 + 2^14) >> 15.
__device__ __forceinline__ int gray_bgr(int b, int g, int r) {
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15;
}
__device__ __forceinline__ int gray_bgr(const uint8_t* p) { return gray_bgr(p[0], p[1], p[2]); }
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

// acc [n][3] int64: {sum bytes, sum L, sum L^2}; zeroed by the caller.  One thread per pixel.
__global__ __launch_bounds__(RS_THREADS)
void frame_quality_kernel(const uint8_t* __restrict__ frames, long long* __restrict__ acc, int h, int w) {
    const int img = blockIdx.y;
    const uint8_t* f = frames + (size_t)img * h * w * 3;
    long long sb = 0, sl = 0, sl2 = 0;
    const int total = h * w;
    for (int idx = blockIdx.x * RS_THREADS + threadIdx.x; idx < total; idx += gridDim.x * RS_THREADS) {
        const int y = idx / w, x = idx - y * w;
        const uint8_t* p = f + (size_t)idx * 3;
        sb += p[0] + p[1] + p[2];
        const int yu = reflect101(y - 1, h), yd = reflect101(y + 1, h);
        const int xl = reflect101(x - 1, w), xr = reflect101(x + 1, w);
        const int lap = gray_bgr(f + ((size_t)yu * w + x) * 3) + gray_bgr(f + ((size_t)yd * w + x) * 3) +
                        gray_bgr(f + ((size_t)y * w + xl) * 3) + gray_bgr(f + ((size_t)y * w + xr) * 3) - 4 * gray_bgr(p);
        sl += lap; sl2 += (long long)lap * lap;
    }
    // wave reduction, then one atomic per wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sb += __shfl_down(sb, off); sl += __shfl_down(sl, off); sl2 += __shfl_down(sl2, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd((unsigned long long*)&acc[img * 3 + 0], (unsigned long long)sb);
        atomicAdd((unsigned long long*)&acc[img * 3 + 1], (unsigned long long)sl);
        atomicAdd((unsigned long long*)&acc[img * 3 + 2], (unsigned long long)sl2);
    }
}

// ---- fused frame post-processing (reference frame_extractor.py:279-293) -----------------------------------
// OptimizedFrameExtractor.extract_frames per sampled frame: cv2.resize to frame_size, _is_low_quality, keep or drop.
// One device pass instead of resize -> download -> upload -> frame_quality_kernel -> host verdict:
//
// postproc_fused_kernel: grid (bands of output rows, frames).  A workgroup produces its band of the resized frame
// into LDS — the arithmetic of cv_resize_linear_kernel / cv_resize_half_kernel / a copy, byte for byte — plus the two
// halo rows reflect101(y0 - 1, out_h) and reflect101(y1 + 1, out_h) (y0 / y1: its first / last owned row), computed
// like any other row whichever row they turn out to be.  Each pixel is converted to grey once, into an LDS grey plane.
// The owned rows go to global memory from LDS (16-byte stores when the row bytes and the destination allow, else
// 4-byte, else bytes); the sum of the owned bytes and the sums of L and L^2 of the 4-neighbour Laplacian over the
// owned pixels (BORDER_REFLECT_101: the halo rows vertically, reflect101 on the column horizontally) come from LDS.
// They are frame_quality_kernel's three sums, stored per workgroup (no global atomics; integers, so the order of
// the later sum does not matter).
//   LDS: pix [lrows][pitch] bytes (row 0 / rows + 1 the halos, pitch = row bytes rounded up to 16), grey
//   [lrows][gpitch], then PP_RED_BYTES of reduction scratch; lrows = min(band_rows, out_h) + 2.  The host plan
//   (pp_plan) picks band_rows so that all of it stays within PP_LDS_BUDGET.
//   A thread handles at most lrows * (out_w / 256 + 1) <= 64 + 34 pixels (lrows * out_w * 4 <= the budget), so its
//   three sums fit 32 bits: 98 * 1020^2 < 2^27.
//
// postproc_verdict_kernel: one workgroup over n <= 65535 frames sums each frame's partials and decides in integers,
// with N = out_h * out_w, S1 = sum L, S2 = sum L^2:
//   low quality  <=>  sum_bytes < 20 * 3 * N  ||  sum_bytes > 235 * 3 * N  ||  N * S2 - S1^2 < 100 * N^2.
// N <= 2^21 keeps every term inside int64 (N^2 * 1020^2 < 2^63).  These are the verdicts of
// FramePreprocessor.is_low_quality, which compares the rounded quotients sum_bytes / (3 N) and (N S2 - S1^2) / N^2
// with 20, 235 and 100: a quotient that does not equal its threshold lies at least 1 / (3 N) resp. 1 / N^2 >= 2^-42
// away from it — relative to a threshold of at most 235 that is above 2^-50, several ulps of a double — so rounding
// the quotient cannot carry it onto or across the threshold, and a quotient that equals the threshold is exact.
// It then leaves keep[i], the exclusive prefix sum of keep and the total (kept bits in LDS, popcounts).
//
// postproc_gather_kernel: kept frame i -> slot prefix[i] of the result buffer.
constexpr int PP_LDS_BUDGET = 65536;                         // bytes of dynamic LDS a fused workgroup may ask for
constexpr int PP_MAX_BAND_ROWS = 32;                         // 224 x 224: 7 bands of 32 rows, 6 % of halo rows
constexpr int PP_RED_BYTES = 128;                            // 4 waves x 3 int64, rounded up
constexpr int PP_MAX_PIXELS = 1 << 21;                       // out_h * out_w the integer verdict is proven for
constexpr int PP_COPY = 0, PP_HALF = 1, PP_LINEAR = 2;

__host__ __device__ inline int pp_pitch(int out_w) { return (out_w * 3 + 15) & ~15; }
__host__ __device__ inline int pp_gpitch(int out_w) { return (out_w + 15) & ~15; }
// LDS bytes of a fused workgroup whose bands have `rows` rows
__host__ __device__ inline long long pp_lds_bytes(int rows, int out_w) {
    return (long long)(rows + 2) * (pp_pitch(out_w) + pp_gpitch(out_w)) + PP_RED_BYTES;
}
// band_rows: the most rows (at most PP_MAX_BAND_ROWS) whose band fits the budget; fused = 0 when not even one does
inline void pp_plan(int out_h, int out_w, int* band_rows, int* n_bands, int* fused) {
    const long long per_row = pp_pitch(out_w) + pp_gpitch(out_w);
    long long rows = (PP_LDS_BUDGET - PP_RED_BYTES) / per_row - 2;
    if (rows > PP_MAX_BAND_ROWS) rows = PP_MAX_BAND_ROWS;
    *fused = rows >= 1;
    *band_rows = rows >= 1 ? (int)rows : out_h;              // unfused: the whole frame is one "band" (one partial)
    *n_bands = (out_h + *band_rows - 1) / *band_rows;
}

// one output pixel (dy, dx) of the resized frame, exactly as cv_resize_linear_kernel / cv_resize_half_kernel / a copy
template <int MODE>
__device__ __forceinline__ void pp_pixel(const uint8_t* __restrict__ f, const int* __restrict__ xofs, const int* __restrict__ wx,
                                         const int* __restrict__ yofs, const int* __restrict__ wy, int h, int w, int dy, int dx,
                                         int (&v)[3]) {
    const size_t pitch = (size_t)w * 3;
    if constexpr (MODE == PP_COPY) {
        const uint8_t* p = f + (size_t)dy * pitch + (size_t)dx * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
    } else if constexpr (MODE == PP_HALF) {
        const uint8_t* p = f + (size_t)(2 * dy) * pitch + (size_t)(2 * dx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (p[c] + p[3 + c] + p[pitch + c] + p[pitch + 3 + c] + 2) >> 2;
    } else {
        const int sx = xofs[dx], sx1 = min(sx + 1, w - 1);
        const int a0 = wx[2 * dx], a1 = wx[2 * dx + 1];
        const int sy = yofs[dy];
        const int y0 = min(max(sy, 0), h - 1), y1 = min(max(sy + 1, 0), h - 1);
        const int b0 = wy[2 * dy], b1 = wy[2 * dy + 1];
        const uint8_t* r0 = f + (size_t)y0 * pitch;
        const uint8_t* r1 = f + (size_t)y1 * pitch;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
            const int d1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
            v[c] = (int)(uint8_t)((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2);
        }
    }
}

//   src [n][h][w][3]; dst [n][out_h][out_w][3]; partials [n][gridDim.x][3] int64 = {sum bytes, sum L, sum L^2}
//   WIDE_SRC (PP_COPY only): rows are 16-byte aligned multiples of 16 bytes, staged with 16-byte loads
//   store_vec: 16, 4 or 1 bytes per store of the owned rows
template <int MODE, bool WIDE_SRC>
__global__ __launch_bounds__(RS_THREADS)
void postproc_fused_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long* __restrict__ partials,
                           const int* __restrict__ xofs, const int* __restrict__ wx, const int* __restrict__ yofs,
                           const int* __restrict__ wy, int h, int w, int out_h, int out_w, int band_rows, int lrows, int store_vec) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pp_lds[];
    const int pitch = pp_pitch(out_w), gpitch = pp_gpitch(out_w);
    uint8_t* pix = pp_lds;                                           // [lrows][pitch]
    uint8_t* grey = pix + (size_t)lrows * pitch;                     // [lrows][gpitch]
    long long* red = (long long*)(grey + (size_t)lrows * gpitch);    // [4][3]
    const int band = blockIdx.x, img = blockIdx.y;
    const int y0 = band * band_rows, rows = min(band_rows, out_h - y0), y1 = y0 + rows - 1;
    const int row_bytes = out_w * 3;
    const uint8_t* f = src + (size_t)img * h * w * 3;
    auto out_row = [&](int r) { return r == 0 ? reflect101(y0 - 1, out_h) : (r == rows + 1 ? reflect101(y1 + 1, out_h) : y0 + r - 1); };
    int sb = 0;

    // ---- the band and its halo rows -> pix, grey ----
    if constexpr (MODE == PP_COPY && WIDE_SRC) {
        const int cpr = row_bytes >> 4;                              // row_bytes == pitch here
        for (int i = threadIdx.x; i < (rows + 2) * cpr; i += RS_THREADS) {
            const int r = i / cpr, c = i - r * cpr;
            *(uint4*)(pix + (size_t)r * pitch + 16 * c) = *(const uint4*)(f + (size_t)out_row(r) * row_bytes + 16 * c);
        }
        __syncthreads();
        for (int r = 0; r < rows + 2; ++r) {
            const bool owned = r >= 1 && r <= rows;
            for (int x = threadIdx.x; x < out_w; x += RS_THREADS) {
                const uint8_t* p = pix + (size_t)r * pitch + 3 * x;
                const int b = p[0], g = p[1], rr = p[2];
                grey[(size_t)r * gpitch + x] = (uint8_t)gray_bgr(b, g, rr);
                if (owned) sb += b + g + rr;
            }
        }
    } else {
        for (int r = 0; r < rows + 2; ++r) {
            const int dy = out_row(r);
            const bool owned = r >= 1 && r <= rows;
            for (int x = threadIdx.x; x < out_w; x += RS_THREADS) {
                int v[3];
                pp_pixel<MODE>(f, xofs, wx, yofs, wy, h, w, dy, x, v);
                uint8_t* p = pix + (size_t)r * pitch + 3 * x;
                p[0] = (uint8_t)v[0]; p[1] = (uint8_t)v[1]; p[2] = (uint8_t)v[2];
                grey[(size_t)r * gpitch + x] = (uint8_t)gray_bgr(v[0], v[1], v[2]);
                if (owned) sb += v[0] + v[1] + v[2];
            }
        }
    }
    __syncthreads();

    // ---- owned rows -> global: rows y0 .. y1 are contiguous there ----
    uint8_t* o = dst + ((size_t)img * out_h + y0) * row_bytes;
    if (store_vec == 16) {
        const int cpr = row_bytes >> 4;
        for (int i = threadIdx.x; i < rows * cpr; i += RS_THREADS) {
            const int r = i / cpr, c = i - r * cpr;
            *(uint4*)(o + (size_t)r * row_bytes + 16 * c) = *(const uint4*)(pix + (size_t)(r + 1) * pitch + 16 * c);
        }
    } else if (store_vec == 4) {
        const int cpr = row_bytes >> 2;
        for (int i = threadIdx.x; i < rows * cpr; i += RS_THREADS) {
            const int r = i / cpr, c = i - r * cpr;
            *(uint32_t*)(o + (size_t)r * row_bytes + 4 * c) = *(const uint32_t*)(pix + (size_t)(r + 1) * pitch + 4 * c);
        }
    } else {
        for (int r = 0; r < rows; ++r)
            for (int j = threadIdx.x; j < row_bytes; j += RS_THREADS) o[(size_t)r * row_bytes + j] = pix[(size_t)(r + 1) * pitch + j];
    }

    // ---- Laplacian sums over the owned pixels, from the grey plane ----
    int sl = 0, sl2 = 0;
    for (int r = 1; r <= rows; ++r) {
        const uint8_t* g = grey + (size_t)r * gpitch;
        for (int x = threadIdx.x; x < out_w; x += RS_THREADS) {
            const int lap = (int)g[x - gpitch] + (int)g[x + gpitch] + (int)g[reflect101(x - 1, out_w)] + (int)g[reflect101(x + 1, out_w)] -
                            4 * (int)g[x];
            sl += lap; sl2 += lap * lap;
        }
    }
    long long a = sb, b = sl, c = sl2;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); c += __shfl_down(c, off); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave * 3] = a; red[wave * 3 + 1] = b; red[wave * 3 + 2] = c; }
    __syncthreads();
    if (threadIdx.x < 3)
        partials[((size_t)img * gridDim.x + band) * 3 + threadIdx.x] =
            red[threadIdx.x] + red[3 + threadIdx.x] + red[6 + threadIdx.x] + red[9 + threadIdx.x];
}

//   partials [n][nb][3]; res: [0] = frames kept, then sums [n][3]; keep [n] bytes; prefix [n]: kept frames before frame i
//   filter == 0: every frame is kept (the sums are still formed)
__global__ __launch_bounds__(RS_THREADS)
void postproc_verdict_kernel(const long long* __restrict__ partials, int n, int nb, long long N, int filter,
                             long long* __restrict__ res, uint8_t* __restrict__ keep, int* __restrict__ prefix) {
    __shared__ uint32_t bits[2048];                                  // bit i: frame i is kept (n <= 65535)
    __shared__ uint32_t wpre[2048];                                  // kept frames before word j's first frame
    __shared__ uint32_t tsum[RS_THREADS];
    const int t = threadIdx.x;
    for (int i = t; i < 2048; i += RS_THREADS) bits[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += RS_THREADS) {
        const long long* p = partials + (size_t)i * nb * 3;
        long long sb = 0, s1 = 0, s2 = 0;
        for (int b = 0; b < nb; ++b) { sb += p[3 * b]; s1 += p[3 * b + 1]; s2 += p[3 * b + 2]; }
        res[1 + 3 * (size_t)i] = sb; res[2 + 3 * (size_t)i] = s1; res[3 + 3 * (size_t)i] = s2;
        const bool low = filter && (sb < 20 * 3 * N || sb > 235 * 3 * N || N * s2 - s1 * s1 < 100 * N * N);
        keep[i] = low ? 0 : 1;
        if (!low) atomicOr(&bits[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    uint32_t mine = 0;                                               // thread t owns words 8t .. 8t + 7
#pragma unroll
    for (int k = 0; k < 8; ++k) mine += __popc(bits[8 * t + k]);
    tsum[t] = mine;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < RS_THREADS; ++i) { const uint32_t v = tsum[i]; tsum[i] = run; run += v; }
        res[0] = run;
    }
    __syncthreads();
    uint32_t run = tsum[t];
#pragma unroll
    for (int k = 0; k < 8; ++k) { wpre[8 * t + k] = run; run += __popc(bits[8 * t + k]); }
    __syncthreads();
    for (int i = t; i < n; i += RS_THREADS) prefix[i] = (int)(wpre[i >> 5] + __popc(bits[i >> 5] & ((1u << (i & 31)) - 1u)));
}
static_assert(RS_THREADS * 8 * 32 >= 65536, "the verdict's bit set must hold 65535 frames");

// grid (x, n).  WIDE: frame_bytes is a multiple of 16 and both buffers are 16-byte aligned -> 16-byte copies
template <bool WIDE>
__global__ __launch_bounds__(RS_THREADS)
void postproc_gather_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ keep,
                            const int* __restrict__ prefix, size_t frame_bytes) {
    const int i = blockIdx.y;
    if (!keep[i]) return;
    const uint8_t* s = src + (size_t)i * frame_bytes;
    uint8_t* d = dst + (size_t)prefix[i] * frame_bytes;
    const size_t step = (size_t)gridDim.x * RS_THREADS;
    if constexpr (WIDE) {
        const size_t n16 = frame_bytes >> 4;
        for (size_t j = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; j < n16; j += step) ((uint4*)d)[j] = ((const uint4*)s)[j];
    } else {
        for (size_t j = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; j < frame_bytes; j += step) d[j] = s[j];
    }
}

// ---- scene-change score (reference frame_extractor.py:168-186) -------------------------------------------
// AdaptiveFrameSampler._calculate_frame_difference for every consecutive pair (earlier a, later b) of a batch:
//   mse = mean((grey_a - grey_b)^2), chi = cv2.compareHist(hist_a, hist_b, HISTCMP_CHISQR), score = mse + chi * 0.01.
// Two kernels.  scene_partials_kernel streams the frames once and leaves exact integer partials per (frame, pixel
// tile); scene_finalise_kernel sums them and does the few hundred fp64 operations of a pair in a fixed order.
//
// scene_partials_kernel: grid (pixel tiles, frame chunks).  A workgroup owns SC_TILE pixels (SC_PPT per thread) and
// walks SC_CHUNK_FRAMES consecutive frames in order, keeping the previous frame's grey values of its own pixels packed
// four to a register, so the squared difference of a pair needs no second read.  The frame before a chunk's first one
// (the caller's `prev` for chunk 0) is read for its grey values only: a 1/SC_CHUNK_FRAMES share of re-read, and its
// histogram belongs to the chunk before (to chunk 0 for `prev`, which nobody else reads).
// Histogram: one private 256-bin copy per wave in LDS, non-returning ds_add_u32; combined per frame after a barrier and
// stored plainly to hist[slot][tile][256] (slot 0 = prev, slot k + 1 = frame k) — no global atomics: a 1080p frame
// would send its ~250 workgroups to the same 257 words.  1 KiB of partials per 24 KiB of tile read.
// Counts are uint32 (a constant tile puts SC_TILE pixels into one bin); a tile's squared-difference sum is at most
// SC_TILE * 255^2 < 2^32.
constexpr int SC_PPT = 32;                                   // pixels per thread: two groups of 16 (48 bytes = three 16-byte loads)
constexpr int SC_TILE = RS_THREADS * SC_PPT;                 // 8192 pixels per workgroup
constexpr int SC_CHUNK_FRAMES = 8;                           // frames a workgroup walks (plus the one before them, grey only)
static_assert((long long)SC_TILE * 255 * 255 < (1ll << 32), "a tile's squared-difference sum must fit uint32");

// grey values of this thread's SC_PPT pixels of one frame, packed four to a dword.
//   WIDE (frame base and h*w*3 multiples of 16): pixels [first + 16*(tid + 256*j), +16), j = 0, 1; a group of 16 is
//   all inside the frame or all outside it, since h*w is then a multiple of 16.
//   bytes: pixels first + tid + 256*k, k = 0..31 (consecutive lanes on consecutive pixels), each bounds-checked.
// Pixels outside the frame pack as 0 and are skipped by `valid` (bit per pixel, the same for every frame).
template <bool WIDE>
__device__ __forceinline__ void sc_load_grey(const uint8_t* __restrict__ f, int first, int npix, uint32_t (&g)[SC_PPT / 4]) {
    if constexpr (WIDE) {
#pragma unroll
        for (int j = 0; j < SC_PPT / 16; ++j) {
            const int p0 = first + 16 * ((int)threadIdx.x + RS_THREADS * j);
            uint32_t d[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) d[i] = 0;
            if (p0 < npix) {
                const uint4* q = (const uint4*)(f + (size_t)p0 * 3);
                const uint4 a = q[0], b = q[1], c = q[2];
                d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
                d[8] = c.x; d[9] = c.y; d[10] = c.z; d[11] = c.w;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = 3 * i;
                const int bb = (d[k >> 2] >> (8 * (k & 3))) & 255, gg = (d[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 255,
                          rr = (d[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 255;
                const uint32_t v = (uint32_t)gray_bgr(bb, gg, rr);
                if ((i & 3) == 0) g[4 * j + (i >> 2)] = v; else g[4 * j + (i >> 2)] |= v << (8 * (i & 3));
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < SC_PPT; ++k) {
            const int p = first + (int)threadIdx.x + RS_THREADS * k;
            const uint32_t v = p < npix ? (uint32_t)gray_bgr(f + (size_t)p * 3) : 0u;
            if ((k & 3) == 0) g[k >> 2] = v; else g[k >> 2] |= v << (8 * (k & 3));
        }
    }
}

template <bool WIDE>
__device__ __forceinline__ uint32_t sc_valid_mask(int first, int npix) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < SC_PPT; ++k) {
        const int p = WIDE ? first + 16 * ((int)threadIdx.x + RS_THREADS * (k >> 4)) + (k & 15) : first + (int)threadIdx.x + RS_THREADS * k;
        m |= (uint32_t)(p < npix) << k;
    }
    return m;
}

//   frames [m][npix][3]; prev: one frame or null
//   hist   [m + 1][tiles][256] uint32: slot 0 is written only when prev is given
//   ssd    [m][tiles] uint32: pair i = (frame i - 1 or prev, frame i); pair 0 is written only when prev is given
template <bool WIDE>
__global__ __launch_bounds__(RS_THREADS)
void scene_partials_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ prev,
                           uint32_t* __restrict__ hist, uint32_t* __restrict__ ssd, int m, int npix) {
    __shared__ uint32_t lh[4][256];                                  // one histogram copy per wave
    __shared__ uint32_t ls[4];
    const int tile = blockIdx.x, tiles = gridDim.x;
    const int first = tile * SC_TILE;
    const int k0 = blockIdx.y * SC_CHUNK_FRAMES, k1 = min(m, k0 + SC_CHUNK_FRAMES);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t frame_bytes = (size_t)npix * 3;
    const uint32_t valid = sc_valid_mask<WIDE>(first, npix);
#pragma unroll
    for (int c = 0; c < 4; ++c) lh[c][threadIdx.x] = 0;
    __syncthreads();

    uint32_t pg[SC_PPT / 4];
    bool have_pg = false;
    // k = k0 - 1 is the frame before the chunk: grey only, except prev (k = -1), whose histogram is this chunk's too
    for (int k = (k0 > 0 || prev) ? k0 - 1 : k0; k < k1; ++k) {
        const uint8_t* f = k < 0 ? prev : frames + (size_t)k * frame_bytes;
        const bool want_hist = k >= k0 || k < 0;
        uint32_t g[SC_PPT / 4];
        sc_load_grey<WIDE>(f, first, npix, g);
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < SC_PPT / 16; ++j) {
            if (WIDE && !((valid >> (16 * j)) & 1)) continue;        // a wide group is inside the frame or outside it as a whole
            bool add_each = want_hist;
            if constexpr (WIDE) {
                // Flat picture areas (a constant frame, letterbox bars): when all 16 pixels of every active lane hold one grey
                // value, the wave's 1,024 consecutive pixels go to the bin in ONE add.  Lane by lane they would be 64 adds to
                // the same LDS word per instruction, which serialise (measured: constant 1080p frames 3.6x slower than noise).
                if (want_hist) {
                    const uint32_t c = __builtin_amdgcn_readfirstlane(g[4 * j]);
                    const uint32_t odd = (g[4 * j] ^ c) | (g[4 * j + 1] ^ c) | (g[4 * j + 2] ^ c) | (g[4 * j + 3] ^ c);
                    if (c == (c & 255u) * 0x01010101u && __builtin_amdgcn_ballot_w64(odd != 0) == 0) {
                        const unsigned long long active = __builtin_amdgcn_ballot_w64(true);
                        if (lane == __builtin_ctzll(active))
                            __hip_atomic_fetch_add(&lh[wave][c & 255u], 16u * (uint32_t)__builtin_popcountll(active), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                        add_each = false;
                    }
                }
            }
#pragma unroll
            for (int i = 16 * j; i < 16 * j + 16; ++i) {
                if (!WIDE && !((valid >> i) & 1)) continue;
                const int v = (g[i >> 2] >> (8 * (i & 3))) & 255;
                if (add_each) __hip_atomic_fetch_add(&lh[wave][v], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (have_pg) {
                    const int dlt = v - (int)((pg[i >> 2] >> (8 * (i & 3))) & 255);
                    s += (uint32_t)(dlt * dlt);
                }
            }
        }
        if (have_pg) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
            if (lane == 0) ls[wave] = s;
        }
        __syncthreads();                                             // every wave's adds of this frame are in LDS
        if (want_hist) {
            const uint32_t c = lh[0][threadIdx.x] + lh[1][threadIdx.x] + lh[2][threadIdx.x] + lh[3][threadIdx.x];
            hist[((size_t)(k + 1) * tiles + tile) * 256 + threadIdx.x] = c;
#pragma unroll
            for (int w = 0; w < 4; ++w) lh[w][threadIdx.x] = 0;
        }
        if (have_pg && threadIdx.x == 0) ssd[(size_t)k * tiles + tile] = ls[0] + ls[1] + ls[2] + ls[3];
        __syncthreads();                                             // copies are zero and ls is free before the next frame
#pragma unroll
        for (int i = 0; i < SC_PPT / 4; ++i) pg[i] = g[i];
        have_pg = true;
    }
}

// One 256-thread workgroup per pair.  Thread b sums bin b of the earlier (slot pair) and the later (slot pair + 1)
// frame over the tiles, as integers, and forms its chi-square term; the squared-difference partials are summed as
// integers; thread 0 adds the 256 terms in ascending bin order (a bin with H_a == 0 contributes +0.0, which leaves
// the running non-negative sum unchanged, so this is OpenCV's "skip when the denominator is zero").
// Every fp64 step is one correctly rounded operation: no contraction into FMAs here.
//   res [m][3] = {mse, chi, score}; pair 0 without a predecessor is {0, 0, 0}
__global__ __launch_bounds__(256)
void scene_finalise_kernel(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ ssd, double* __restrict__ res,
                           int tiles, int npix, int has_prev) {
#pragma clang fp contract(off)
    __shared__ double term[256];
    __shared__ unsigned long long part[256];
    const int pair = blockIdx.x, b = threadIdx.x;
    if (pair == 0 && !has_prev) {
        if (b < 3) res[b] = 0.0;
        return;
    }
    const uint32_t* ha = hist + (size_t)pair * tiles * 256 + b;
    const uint32_t* hb = ha + (size_t)tiles * 256;
    long long ca = 0, cb = 0;
    unsigned long long s = 0;
    for (int t = 0; t < tiles; ++t) { ca += ha[(size_t)t * 256]; cb += hb[(size_t)t * 256]; }
    for (int t = b; t < tiles; t += 256) s += ssd[(size_t)pair * tiles + t];
    double tm = 0.0;
    if (ca != 0) {
        const double d = (double)(ca - cb);
        const double dd = d * d;
        tm = dd / (double)ca;
    }
    term[b] = tm;
    part[b] = s;
    __syncthreads();
    if (b == 0) {
        double chi = 0.0;
        unsigned long long S = 0;
        for (int i = 0; i < 256; ++i) { chi += term[i]; S += part[i]; }
        const double mse = (double)S / (double)npix;
        const double scaled = chi * 0.01;
        res[(size_t)pair * 3 + 0] = mse;
        res[(size_t)pair * 3 + 1] = chi;
        res[(size_t)pair * 3 + 2] = mse + scaled;
    }
}

}  // namespace vq
