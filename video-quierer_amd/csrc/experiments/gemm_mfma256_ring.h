// Ring variant of gemm_tn256_kernel (gemm_mfma256.h; kernel id 3, measured and rejected): same 256x256 tile / wave layout, but the K loop advances in 32-wide sub-tiles
// through a 4-slot LDS ring (4 x {A 256 rows x 64 B, W 256 rows x 64 B} = 128 KiB).
//   phase p (one per sub-tile): read half  = 12 ds_read_b128 (8 A + 4 W fragments of slot p%4),
//                                            4 LDS-DMA pieces refilling slot (p-1)%4 with sub-tile p+3,
//                                            s_waitcnt vmcnt(8) (sub-tile p+1 landed; 8 pieces stay in
//                                            flight), s_waitcnt lgkmcnt(0), s_barrier
//                              MFMA half  = 32 MFMAs (the wave's whole 128x64 tile x K=32), s_barrier
// Twice the MFMAs per barrier pair of the 4-phase-per-K-tile kernel of gemm_mfma256.h (measured there with
// s_memtime stamps: ~200 cycles of barrier/restart per half phase against 256 cycles of MFMA), a
// prefetch distance of three sub-tiles, and every DMA wait counted.  The two wave groups run
// staggered by one barrier.  Hazards (b(k) = k-th barrier; group 0 phase p: pre b(2p), close b(2p+1);
// group 1: pre b(2p+1), close b(2p+2)):
//   WAR  slot (p-1)%4 was last read in phase p-1; both groups retire those reads (lgkmcnt(0)) BEFORE
//        their pre-MFMA barrier, i.e. before b(2p-2) / b(2p-1); the earliest refill is issued after b(2p-1).
//   RAW  sub-tile p+1 is retired by every issuer's vmcnt in the read half of phase p (before b(2p) /
//        b(2p+1)); it is first read after b(2p+1) (group 0) / b(2p+2) (group 1).
// 64-byte LDS rows: chunk c of row r is stored at chunk c ^ (2*((r>>3)&1)) — conflict-free for the four
// ds_read_b128 lane groups (brute-forced against the bank model of MI355X_MICROARCH.md §LDS).
#pragma once
#include "../vq_common.h"
#include "../gemm_mfma.h"
#include "../gemm_mfma256.h"

namespace vq {

constexpr int G3_PART = 256 * G3_SUB_K * 2;       // 16 KiB: 256 rows x 64 B (one operand of one sub-tile)
constexpr int G3_SLOT = 2 * G3_PART;              // 32 KiB
constexpr int G3_LDS_BYTES = 4 * G3_SLOT;         // 128 KiB

template <bool IS_F16, class Epi, bool DIAG = false, int NSLOT = 4>
__global__ __launch_bounds__(G2_THREADS, 2)
void gemm_tn256_ring_kernel(const uint16_t* __restrict__ A, int lda,
                            const uint16_t* __restrict__ W, int ldw,
                            int K, int tiles_n, Epi epi, int diag = 0) {
    typedef mfma_op<IS_F16> op;
    typedef typename op::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (wg / tiles_n) * G2_BM;
    const int n0 = (wg % tiles_n) * G2_BN;

    // LDS-DMA: a 1-KiB piece = 16 rows x 64 B; wave w fills pieces 2w, 2w+1 (rows 32w..32w+31) of A and of W
    const int srow = lane >> 2;                                   // row inside the piece
    const int schunk = (lane & 3) ^ (((lane >> 5) & 1) * 2);      // logical chunk stored at physical slot lane&3
    const uint16_t* a_src[2];
    const uint16_t* w_src[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 16 + srow;
        a_src[i] = A + (size_t)(m0 + row) * lda + schunk * 8;
        w_src[i] = W + (size_t)(n0 + row) * ldw + schunk * 8;
    }
    const int piece_off = wave * 2048;

    auto stage = [&](int slot, int sub) {
        char* dst = smem + slot * G3_SLOT + piece_off;
        const int koff = sub * G3_SUB_K;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(a_src[0] + koff), (lds_void_t*)(dst), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(a_src[1] + koff), (lds_void_t*)(dst + 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(w_src[0] + koff), (lds_void_t*)(dst + G3_PART), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(w_src[1] + koff), (lds_void_t*)(dst + G3_PART + 1024), 16, 0, 0);
    };

    const int frow = lane & 15, fgrp = lane >> 4;
    const int pchunk = fgrp ^ (((frow >> 3) & 1) * 2);
    const int a_base = (wr * 128 + frow) * 64 + pchunk * 16;                 // + mi*1024
    const int w_base = G3_PART + (wc * 64 + frow) * 64 + pchunk * 16;        // + ni*1024

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsub = K / G3_SUB_K;
    auto barrier = [&]() {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // NSLOT ring slots (4 = 128 KiB, 5 = 160 KiB): NSLOT-1 sub-tiles in flight while one is consumed.
    // The slot index is wave-uniform run-time state (scalar adds), so the loop needs no unrolling.
    auto phase = [&](int p, int slot, int slot_refill) __attribute__((always_inline)) {
        const char* buf = smem + slot * G3_SLOT;
        frag af[8], wf[4];
        if (DIAG && (diag & 2)) {
#pragma unroll
            for (int i = 0; i < 8; ++i) af[i] = frag{};
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = frag{};
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) af[i] = *(const frag*)(buf + a_base + i * 1024);
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *(const frag*)(buf + w_base + j * 1024);
        }
        if (p + NSLOT - 1 < nsub) {
            if (!(DIAG && (diag & 1))) stage(slot_refill, p + NSLOT - 1);
            if constexpr (NSLOT == 5) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else                      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (!(DIAG && (diag & 8))) barrier();
        if (!(DIAG && (diag & 4))) {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = op::run(wf[j], af[i], acc[i][j]);
            __builtin_amdgcn_s_setprio(0);
        }
        if (!(DIAG && (diag & 8))) barrier();
    };

    // prologue: sub-tiles 0..NSLOT-2 in flight, 0 landed
#pragma unroll
    for (int i = 0; i < NSLOT - 1; ++i) stage(i, i);
    if constexpr (NSLOT == 5) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else                      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    barrier();

    if (wr == 1) barrier();               // stagger: group 1 runs one barrier behind group 0
    int slot = 0, slot_refill = NSLOT - 1;
    for (int p = 0; p < nsub; ++p) {
        phase(p, slot, slot_refill);
        slot_refill = slot;               // the slot just consumed is refilled next phase ... (p-1)%NSLOT
        slot = slot + 1 == NSLOT ? 0 : slot + 1;
    }
    if (wr == 0) barrier();

    barrier();                            // group 1's last fragment reads are retired before anyone reuses LDS
    wave_epilogue<8>(smem + wave * EPI_WAVE_BYTES, acc, m0 + wr * 128, n0 + wc * 64, lane, epi);
}

template <bool IS_F16, class Epi>
static int launch_gemm_tn256_ring(hipStream_t st, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                                  int M, int N, int K, const Epi& epi) {
    VQ_CHECK(M > 0 && M % G2_BM == 0 && N % G2_BN == 0 && K % 128 == 0,
             "gemm_tn256_ring: shape M=%d N=%d K=%d is not tile-aligned (256/256/128)", M, N, K);
    VQ_CHECK(lda % 8 == 0 && ldw % 8 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0,
             "gemm_tn256_ring: operands must be 16-byte aligned with lda/ldw %% 8 == 0");
    static bool attr_set = false;
    if (!attr_set) {
        VQ_HIP(hipFuncSetAttribute((const void*)gemm_tn256_ring_kernel<IS_F16, Epi, false, 5>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 5 * G3_SLOT));
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_tn256_ring_kernel<IS_F16, Epi, false, 5>), dim3((M / G2_BM) * (N / G2_BN)), dim3(G2_THREADS),
                       5 * G3_SLOT, st, A, lda, W, ldw, K, N / G2_BN, epi, 0);
    VQ_HIP(hipGetLastError());
    return 0;
}

template <bool IS_F16, class Epi>
static int launch_gemm_tn256_ring_diag(hipStream_t st, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                                       int M, int N, int K, const Epi& epi, int diag) {
    VQ_CHECK(M % G2_BM == 0 && N % G2_BN == 0 && K % 128 == 0, "gemm_tn256_ring_diag: shape not tile-aligned");
    if (diag & 16) {      // bit4: 5-slot ring
        VQ_HIP(hipFuncSetAttribute((const void*)gemm_tn256_ring_kernel<IS_F16, Epi, true, 5>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 5 * G3_SLOT));
        hipLaunchKernelGGL((gemm_tn256_ring_kernel<IS_F16, Epi, true, 5>), dim3((M / G2_BM) * (N / G2_BN)), dim3(G2_THREADS),
                           5 * G3_SLOT, st, A, lda, W, ldw, K, N / G2_BN, epi, diag);
    } else {
        VQ_HIP(hipFuncSetAttribute((const void*)gemm_tn256_ring_kernel<IS_F16, Epi, true, 4>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 4 * G3_SLOT));
        hipLaunchKernelGGL((gemm_tn256_ring_kernel<IS_F16, Epi, true, 4>), dim3((M / G2_BM) * (N / G2_BN)), dim3(G2_THREADS),
                           4 * G3_SLOT, st, A, lda, W, ldw, K, N / G2_BN, epi, diag);
    }
    VQ_HIP(hipGetLastError());
    return 0;
}

}  // namespace vq
