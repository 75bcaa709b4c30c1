// The streamed 256 x 256 fp16 mainloop of the tile scans: label_tile_kernel (knn_label.h), match_tile_kernel (knn_match.h) and
// the parked scan2_f16_top2_kernel (experiments/knn_scan_phase4.h) call it and differ only in the fold they hand it and in where
// their operands start.  set_group_max_kernel (knn_set.h) runs the same schedule from a copy of its own (its header says why):
// what is argued here holds there, and a change to the schedule is made in both.
//
//   scores[256 resident rows of A][256 nt streamed rows of W] = A x W^T, fp16 operands, fp32 accumulators, never stored:
//   every finished 256 x 256 tile is handed, a quadrant at a time, to the caller's fold.
//
// Geometry, LDS image and swizzle are gemm_tn256_kernel's (gemm_mfma256.h): 512 threads = 8 waves as 2 (wr: A halves) x 4
// (wc: 64 W rows each), a wave owns 128 x 64 scores of every tile = acc[8][4] MFMA 16x16x32 tiles, LDS = 2 K-tile buffers x
// {A half 0, A half 1, W half 0, W half 1} x 16 KiB (G2_LDS_BYTES at the start of smem).  The nt tiles make ONE continuous
// K loop of nt * dim / 64 K-tiles: the resident rows' K-tiles are staged again per streamed tile (from L2), so the DMA ring
// never drains between tiles.  dim % 128 == 0 (a tile never ends on an odd K-tile), nt >= 1, A and W hold whole tiles.
//
// Schedule.  A K-tile is 4 phases; a phase = read half {ds_read the sub-tile it needs, issue ONE half-tile of LDS-DMA
// prefetch} | s_barrier | MFMA half {16 MFMAs: one 64 x 32 quadrant x K = 64} | s_barrier.  Quadrants run in the order (0,0)
// (0,1) (1,1) (1,0), which re-reads one operand sub-tile per phase.  The two wave groups (wr = 0 / 1, which share every SIMD
// pairwise) run STAGGERED by one barrier: one group's read half sits under the other's MFMAs.  K-tile kt + 1 is prefetched
// during K-tile kt (A half 1, W half 0, W half 1 in phases 1-3), its A half 0 already in phase 4 of K-tile kt - 1.
//
// Hazards under the stagger (group 1 is one barrier behind group 0; b(k) = the k-th barrier):
//  RAW  the only VMEM wait of the loop is the COUNTED s_waitcnt vmcnt(2) in the read half of phase 4: it retires K-tile
//       kt + 1 and leaves the half-tile just issued (A half 0 of kt + 2: two DMA instructions) in flight.  It sits before
//       b(2p) for group 0 and b(2p+1) for group 1; K-tile kt + 1 is first read after b(2p+1) (group 0) / b(2p+2) (group 1):
//       every issuer's wait precedes a barrier the reader has passed.
//  WAR  a half-tile is staged again >= 2 phases after its last ds_read (A half 1, the W halves), except A half 0 in phase 4
//       right after its last read in phase 3: A half 0 is read by group 0 only, whose phase-3 reads retire (lgkmcnt(0)) before
//       b(2p-1), and nobody issues the phase-4 DMA before b(2p-1).
//  Barriers are raw s_barrier, never __syncthreads() (which would drain the DMA queue).
//
// The fold.  fold(acc, hm, hn, t) receives quadrant (hm, hn) = acc[4 hm .. + 3][2 hn .. + 1] of streamed tile t complete,
// and must leave those accumulators cleared.  It runs in the read half of the phase AFTER the quadrant's last MFMAs, i.e. under
// the partner group's MFMAs: (0,0), (0,1), (1,1) in phases 2-4 of the tile's last K-tile, (1,0) in phase 1 of the next
// tile's first K-tile, or behind the loop for tile nt - 1.  So per tile the folds arrive in the order (0,0) (0,1) (1,1) (1,0):
// hm != hn marks the second quadrant of its hm.  A fold may issue global loads, stores and atomics: they are older than the
// DMA the counted wait leaves in flight (the phase-4 fold is issued before it), so they only add to what the wait retires,
// never to what it lets pass.  A fold must not contain a barrier; waves need not agree on what they do in it.
// Behind the call every wave has issued its last ds_read and no DMA is in flight (vmcnt(0) in the last K-tile); a caller that
// reuses the LDS puts one more barrier first.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "gemm_mfma256.h"

namespace vq {

// the lane's place in the wave grid and in an MFMA tile: it holds, of acc[mi][ni][r], the score of resident row
// 128 wr + 16 mi + frow and streamed row 64 wc + 16 ni + 4 fgrp + r of the tile
struct Stream256Lane { int wr, wc, frow, fgrp; };
__device__ __forceinline__ Stream256Lane stream256_lane() {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return Stream256Lane{wave >> 2, wave & 3, lane & 15, lane >> 4};
}

// A: the 256 resident rows, W: the first streamed row; both [.][dim] fp16, 16-byte aligned.
template <class Fold>
__device__ __forceinline__ void stream256_run(char* smem, const Stream256Lane ln, const uint16_t* __restrict__ A, const uint16_t* __restrict__ W,
                                              int dim, int nt, Fold&& fold) {
    typedef mfma_op<true> op;
    typedef op::frag frag;
    const int lane = threadIdx.x & 63;
    const int wr = ln.wr, wc = ln.wc, wave = wr * 4 + wc;

    // ---- LDS-DMA source pointers: wave w fills 1-KiB pieces 2w, 2w+1 of a half-tile ----
    const int srow = lane >> 3, sslot = lane & 7;
    const uint16_t* a_src[2];
    const uint16_t* w_src[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + srow;            // row inside the 128-row half-tile
        const int chunk = sslot ^ ((row >> 1) & 7);
        a_src[i] = A + (size_t)row * dim + chunk * 8;
        w_src[i] = W + (size_t)row * dim + chunk * 8;
    }
    const size_t half_rows = (size_t)128 * dim;
    const int piece_off = wave * 2048;
    const int nk = dim / G2_BK;                          // K-tiles per streamed tile (even)
    const int total = nt * nk;                           // flattened K-tiles

    // which: 0/1 = A halves, 2/3 = W halves; kt = flattened K-tile index
    auto stage = [&](int buf, int which, int kt) __attribute__((always_inline)) {
        char* dst = smem + buf * G2_BUF + which * G2_HALF + piece_off;
        const int t = kt / nk, kk = kt - t * nk;
        if (which < 2) {
            const size_t off = (which ? half_rows : 0) + (size_t)kk * G2_BK;
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(a_src[0] + off), (lds_void_t*)(dst), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(a_src[1] + off), (lds_void_t*)(dst + 1024), 16, 0, 0);
        } else {
            const size_t off = (size_t)t * 256 * dim + ((which & 1) ? half_rows : 0) + (size_t)kk * G2_BK;
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(w_src[0] + off), (lds_void_t*)(dst), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(w_src[1] + off), (lds_void_t*)(dst + 1024), 16, 0, 0);
        }
    };

    // ---- fragment read offsets ----
    const int frow = ln.frow, fgrp = ln.fgrp;
    const int fx = (frow >> 1) & 7;
    const int slot[2] = {((0 + fgrp) ^ fx) * 16, ((4 + fgrp) ^ fx) * 16};
    const int a_base = wr * G2_HALF + frow * 128;
    const int w_base = 2 * G2_HALF + (wc >> 1) * G2_HALF + ((wc & 1) * 64 + frow) * 128;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    frag af[4][2], wf[2][2];

    auto load_a = [&](const char* buf, int hm) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                af[i][ks] = *(const frag*)(buf + a_base + (hm * 4 + i) * 2048 + slot[ks]);
    };
    auto load_w = [&](const char* buf, int hn) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                wf[j][ks] = *(const frag*)(buf + w_base + (hn * 2 + j) * 2048 + slot[ks]);
    };
    auto mfma_quadrant = [&](int hm, int hn) __attribute__((always_inline)) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[hm * 4 + i][hn * 2 + j] = op::run(wf[j][ks], af[i][ks], acc[hm * 4 + i][hn * 2 + j]);
        __builtin_amdgcn_s_setprio(0);
    };
    auto barrier = [&]() __attribute__((always_inline)) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // One K-tile.  `last` = final K-tile of streamed tile t; `fold_prev` = first K-tile of a tile behind another.
    auto tile = [&](int kt, int bufi, bool last, bool fold_prev, int t) __attribute__((always_inline)) {
        const char* buf = smem + bufi * G2_BUF;
        const bool next = kt + 1 < total, next2 = kt + 2 < total;
        // phase 1: quadrant (0,0)
        if (fold_prev) fold(acc, 1, 0, t - 1);
        load_a(buf, 0); load_w(buf, 0);
        if (next) stage(bufi ^ 1, 1, kt + 1);
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(0, 0);
        barrier();
        // phase 2: quadrant (0,1)
        if (last) fold(acc, 0, 0, t);
        load_w(buf, 1);
        if (next) stage(bufi ^ 1, 2, kt + 1);
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(0, 1);
        barrier();
        // phase 3: quadrant (1,1)
        if (last) fold(acc, 0, 1, t);
        load_a(buf, 1);
        if (next) stage(bufi ^ 1, 3, kt + 1);
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(1, 1);
        barrier();
        // phase 4: quadrant (1,0); this buffer's A half 0 is dead -> start K-tile kt+2's A half 0, then retire everything
        // older (K-tile kt+1 complete, the fold's own traffic) with that one half-tile left in flight
        if (last) fold(acc, 1, 1, t);
        load_w(buf, 0);
        if (next2) { stage(bufi, 0, kt + 2); asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
        else       { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(1, 0);
        barrier();
    };

    // ---- prologue: K-tile 0 complete, K-tile 1's A half 0 in flight ----
    stage(0, 0, 0); stage(0, 1, 0); stage(0, 2, 0); stage(0, 3, 0);
    if (total > 1) { stage(1, 0, 1); asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
    else           { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    barrier();

    if (wr == 1) barrier();               // stagger: group 1 runs one barrier behind group 0
    int kk = 0, t = 0;
    for (int kt = 0; kt < total; kt += 2) {
        tile(kt, 0, false, kk == 0 && t > 0, t);
        ++kk;
        tile(kt + 1, 1, kk + 1 == nk, false, t);
        if (++kk == nk) { kk = 0; ++t; }
    }
    fold(acc, 1, 0, nt - 1);
    if (wr == 0) barrier();               // every wave executes the same number of barriers
}

}  // namespace vq
