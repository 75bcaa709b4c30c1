// Second-generation batch scan, superseded by scan5_f16_top2_kernel (knn_scan_fold.h) and kept for A/B
// runs behind VQ_AMD_SCAN=2, `make EXPERIMENTS=1` only: the streamed 256x256 four-phase mainloop (scan_stream256.h, shared
// with the product's tile scans) with a top-2 fold.  Geometry, streams and key layout 2: knn_scan_f16.h (SCAN2_QT,
// SCAN2_RANGE, scan2_row_of, batch_key_index).
#pragma once
#include "../vq_common.h"
#include "../gemm_mfma.h"
#include "../scan_stream256.h"
#include "../knn_scan_f16.h"

namespace vq {

__global__ __launch_bounds__(G2_THREADS, 2)
void scan2_f16_top2_kernel(const uint16_t* __restrict__ Q16, const uint16_t* __restrict__ X16,
                           int dim, int64_t n_valid, int q_tiles, int n_ranges, int range_groups, int64_t q_pad,
                           uint32_t* __restrict__ keys /*[streams][q_pad][2]*/) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Stream256Lane ln = stream256_lane();
    const int wr = ln.wr, wc = ln.wc, frow = ln.frow, fgrp = ln.fgrp;

    int range, qtile;                                    // workgroup order and its L2 rationale: scan2_block_tile (knn_scan_f16.h)
    if (!scan2_block_tile(range_groups, n_ranges, q_tiles, range, qtile)) return;   // whole workgroup leaves before any barrier
    const int m0 = qtile * SCAN2_QT;
    const int64_t n0 = (int64_t)range * SCAN2_RANGE;

    const float NEG = -__builtin_inff();
    const float MASKED = -3.0e38f;       // finite: see scan_f16_top2_kernel
    float m1[8], m2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { m1[i] = NEG; m2[i] = NEG; }

    // fold quadrant (hm, hn) of row tile t into the running top-2 and clear it
    auto fold = [&](f32x4 (&acc)[8][4], int hm, int hn, int t) __attribute__((always_inline)) {
        const bool ragged = n0 + (int64_t)(t + 1) * 256 > n_valid;     // wave-uniform
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int mi = hm * 4 + i, ni = hn * 2 + j;
                    float v = acc[mi][ni][r];
                    if (ragged && n0 + t * 256 + wc * 64 + ni * 16 + 4 * fgrp + r >= n_valid) v = MASKED;
                    const uint32_t kb = (__builtin_bit_cast(uint32_t, v) & ~127u) | (uint32_t)(t * 16 + ni * 4 + r);
                    const float kf = __builtin_bit_cast(float, kb);
                    m2[mi] = __builtin_amdgcn_fmed3f(m1[mi], m2[mi], kf);
                    m1[mi] = fmaxf(m1[mi], kf);
                    acc[mi][ni][r] = 0.f;
                }
    };
    stream256_run(smem, ln, Q16 + (size_t)m0 * dim, X16 + (size_t)n0 * dim, dim, 8, fold);

    const int64_t stream = (int64_t)range * 16 + wc * 4 + fgrp;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        const int q = m0 + wr * 128 + mi * 16 + frow;
        *(uint2*)(keys + batch_key_index(stream, q, (int64_t)n_ranges * 16)) =
            uint2{__builtin_bit_cast(uint32_t, m1[mi]), __builtin_bit_cast(uint32_t, m2[mi])};
    }
}

}  // namespace vq
