// Clip search: the k GROUPS (videos) most similar to a SET of query frames (vq_index_search_set).
//
// Queries q_0 .. q_{m-1}.  d(i, g) = the smallest distance of q_i to a row of group g (distance = fp32(1 - fp32(dot)) by the
// fixed-order fp64 chain, the row that attains it = the smallest (distance, tie rank) key), D(g) = fp32((d(0,g) + d(1,g) + ...
// in fp64, i ascending) / m), the answer = the first k allowed groups by (D, label).  For near-unit rows and queries every d is
// a multiple of 2^-24 of magnitude <= 2, so the fp64 sum of up to 4,096 of them is exact in any order; the kernels still add
// in the order i = 0 .. m-1 so that un-normalised queries have one answer too.
//
// Exact path (mode 1, and the redo of a call the fp16 proof does not cover), per query chunk in order:
//   exact_dist_kernel -> [chunk][n] distances; set_group_min_kernel<true>: the (distance, tie) minimum per (query, group)
//   over the by-group row list (the reduction of group_block_topk_kernel without its top-k); set_accum_dist_kernel: one thread
//   per group adds (double)d(i, g) for the chunk's i ascending into acc[g] (plain loads and stores).  After the last chunk
//   set_final_exact_kernel turns acc into the order key of (D, label); set_select_block_kernel / set_select_merge_kernel take
//   the k smallest; set_match_rows_kernel recomputes, for the k winners only, the row that attains every d(i, g).
//   The redo computes the distances inside set_group_min_kernel<false> (no [chunk][n] buffer); every redo kernel leaves at once
//   unless the call's flag is 2.
//
// fp16 path (mode 2):
//   1. set_group_max_kernel: gbest[i][g] = the order-preserving key of the largest fp16 score of query i over group g, for a
//      whole tile of 256 queries per pass over the matrix — the streamed 256 x 256 mainloop of scan_stream256.h over
//      2048-row ranges (geometry: knn_scan_f16.h) with a group-max fold.  Wave (wr, wc) owns 64 rows of every 256-row tile,
//      all inside one 128-row stream: when stream_group says those rows share a label, the epilogue is a register maximum per
//      query column and ONE atomicMax per (wave, row tile, query); otherwise it reads the 8 row labels of its quadrant and
//      issues at most one atomicMax per (query, run of equal labels); where a lane's 8 rows hold more than two runs (scattered
//      labels) it first reads the keys those groups hold and skips a run that cannot raise its group's (gbest only grows, so a
//      stale read only lets a needless atomic through).  Chunks of <= 16 queries use scan3_group_max_kernel unchanged.
//   2. set_accum_score_kernel: sum16[g] += (double)gbest[i][g] over the chunk's queries; set_query_norm_kernel: |q_i| and
//      the |q|^2 range test.
//   3. set_threshold_kernel (one workgroup): S16(g) = fp32(sum16 / m), Ebar = the mean of E_i = scan_eps_unit(dim) * max|row|
//      * |q_i|, T = the k'-th largest S16 over allowed groups (k' = min(k, allowed); 8-bit radix select), candidates = allowed
//      groups with S16 >= T - 2 Ebar - SET_SLACK (all of them when k >= allowed).
//   4. set_cand_keys_kernel: for every candidate and every i the exact (distance, tie) key over ALL the candidate's rows;
//      set_cand_sum_kernel: D as above; then the exact path's selection; match rows come from the stored keys.
//   Proof.  Every row's fp16 score is within E_i of its exact score s, so |gbest[i][g] - max_r s(i, r)| <= E_i and, with
//   S(g) = the mean over i of max_r s(i, r), |mean_i gbest[i][g] - S(g)| <= Ebar.  The computed S16 is that mean rounded once
//   to fp32 (the fp64 sum of <= 4,096 fp32 values carries an error far below it): dS <= 2^-23 for |S16| < 4.  A reported
//   distance is d = 1 - s up to the fp32 roundings of the dot (|dot| < 4: <= 2^-23) and of the subtraction (<= 2^-23), the
//   minimum over rows keeps that bound, and the final fp32 rounding of D adds <= 2^-23: |D(g) - (1 - S(g))| <= dD = 2^-22 + 2^-23.
//   The k' groups with S16 >= T have S >= T - Ebar - dS, hence D <= 1 - T + Ebar + dS + dD, so the k'-th smallest D is at most
//   that.  A winner w has D(w) <= it, so S(w) >= T - Ebar - dS - 2 dD and S16(w) >= S(w) - Ebar - dS >= T - 2 Ebar - 2 dS - 2 dD.
//   The threshold (T - 2 Ebar) - slack is evaluated in fp32 with two roundings of <= 2^-23 each.  In all the slack has to cover
//   2 dS + 2 dD + 2^-22 = 2^-22 + (2^-21 + 2^-22) + 2^-22 = 5 * 2^-22; SET_SLACK = 2^-19 does.  (Ebar's own fp32 evaluation is
//   inside the 2 % scan_eps_unit carries for that purpose.)  Every winner is therefore a candidate, every candidate gets its
//   exact D, and groups that are not candidates cannot displace a winner.  Comparisons are inclusive.
//   Not provable -> the whole call is redone by the exact path on the device: a query with |q|^2 outside [0.25, 4] or not
//   finite, or more than SET_KEY_BUDGET candidate (group, query) keys.  One flag per call (0 proven path, 2 redo).
//
// Bounded scratch: gbest [chunk][G] <= 256 MiB, exact distances [chunk][n] <= 512 MiB, group minima [chunk][G] <= 256 MiB,
// candidate keys <= SET_KEY_BUDGET * 8 B = 128 MiB; per-group arrays are 40 B per group.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "gemm_mfma256.h"
#include "scan_stream256.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "knn_grouped.h"

namespace vq {

constexpr int SET_MAX_M = 4096;                       // query frames per call
constexpr int64_t SET_KEY_BUDGET = (int64_t)16 << 20; // candidate (group, query) keys on the fp16 path (more: exact redo)
constexpr float SET_SLACK = 1.0f / 524288;            // 2^-19 >= 5 * 2^-22 (derivation above)

// ---- fp16 pass 1: group-max over a 256-query tile.  A workgroup covers 256 queries x 2048 rows (SCAN2_QT, SCAN2_RANGE: 8 row
// tiles, one continuous K loop); a finished quadrant (4 query blocks x 2 row blocks of 16) is folded into group maxima.
// The K loop is stream256_run's (scan_stream256.h: staging, phases, waits and the hazard argument are written there), kept here
// as the kernel's OWN COPY: called through stream256_run, with the row tile's label handed over by a per-tile hook, the kernel
// kept its instruction counts and registers but ran 0.1-0.8 % slower than this copy at m = 64 and 256, repeatably and outside
// the copy's run-to-run spread (profiles/stream256_mainloop/ab.txt), and the margin was not found.  A change to the schedule
// is made in scan_stream256.h first and repeated here.  stream_group / group_of cover `streams` = cdiv(n, 128) streams; row
// tiles past them score nothing.  MASK: disallowed groups never reach gbest. ----
template <bool MASK>
__global__ __launch_bounds__(G2_THREADS, 2)
void set_group_max_kernel(const uint16_t* __restrict__ Q16, const uint16_t* __restrict__ X16, int dim, int64_t streams,
                          int q_tiles, int n_ranges, int range_groups, const int32_t* __restrict__ group_of,
                          const int32_t* __restrict__ stream_group, int nq_real, int n_groups,
                          uint32_t* __restrict__ gbest /*[nq_real][n_groups]*/, const uint32_t* __restrict__ allow) {
    typedef mfma_op<true> op;
    typedef op::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    int range, qtile;
    if (!scan2_block_tile(range_groups, n_ranges, q_tiles, range, qtile)) return;   // whole workgroup leaves before any barrier
    const int m0 = qtile * SCAN2_QT;
    const int64_t n0 = (int64_t)range * SCAN2_RANGE;

    const int srow = lane >> 3, sslot = lane & 7;
    const uint16_t* a_src[2];
    const uint16_t* w_src[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + srow;
        const int chunk = sslot ^ ((row >> 1) & 7);
        a_src[i] = Q16 + (size_t)(m0 + row) * dim + chunk * 8;
        w_src[i] = X16 + (size_t)(n0 + row) * dim + chunk * 8;
    }
    const size_t half_rows = (size_t)128 * dim;
    const int piece_off = wave * 2048;
    const int nk = dim / G2_BK;                          // K-tiles per row tile (even: dim % 128 == 0)
    const int total = 8 * nk;                            // flattened K-tiles

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

    const int frow = lane & 15, fgrp = lane >> 4;
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
    const float NEG = -__builtin_inff();
    const int qbase = m0 + wr * 128 + frow;              // the lane's query of block mi: qbase + 16 mi
    uint32_t* const gb0 = gbest + (size_t)qbase * n_groups; // (never dereferenced for a query past nq_real)
    float tm[8];                                         // uniform row tile: running maximum per query block
#pragma unroll
    for (int i = 0; i < 8; ++i) tm[i] = NEG;

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
    // label of the wave's 64 rows of row tile t: >= 0 shared by all of them, -1 mixed, -2 nothing to score (past the labelled
    // streams, or a disallowed video).  Wave-uniform: a scalar load.
    auto tile_label = [&](int t) __attribute__((always_inline)) -> int {
        const int64_t s = ((n0 + (int64_t)t * 256) >> 7) + (wc >> 1);
        if (s >= streams) return -2;
        const int sg = __builtin_amdgcn_readfirstlane(stream_group[s]);
        if constexpr (MASK)
            if (sg >= 0 && !group_allowed(allow, sg)) return -2;
        return sg;
    };
    // Fold quadrant (hm, hn) of row tile t (label sg) and clear it.  Quadrants of one hm finish in the order hn = 0, 1 for
    // hm = 0 and hn = 1, 0 for hm = 1: `flush` marks the second, where a uniform tile's maxima go out.
    auto fold = [&](int hm, int hn, int t, int sg, bool flush) __attribute__((always_inline)) {
        if (sg >= 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mi = hm * 4 + i;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ni = hn * 2 + j;
#pragma unroll
                    for (int r = 0; r < 4; ++r) tm[mi] = fmaxf(tm[mi], acc[mi][ni][r]);
                    acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                if (flush) {
                    const float v = rows4_max(tm[mi]);                 // over the four lane groups = the wave's 64 rows
                    // one per-lane base + a wave-uniform offset kept in scalar registers (the empty asm pins it there): hoisted
                    // out of the loop, the eight 64-bit row pointers this adds up to do not fit the vector registers
                    size_t uo = (size_t)(mi * 16) * n_groups + sg;
                    asm volatile("" : "+s"(uo));
                    if (fgrp == 0 && qbase + mi * 16 < nq_real) atomicMax(gb0 + uo, score_key(v));
                    tm[mi] = NEG;
                }
            }
        } else if (sg == -1) {
            // rows n0 + t*256 + wc*64 + ni*16 + 4*fgrp + r, ni = 2 hn, 2 hn + 1: two aligned int4 of labels (-1 past the end)
            const int32_t* lp = group_of + (n0 + (int64_t)t * 256 + wc * 64 + hn * 32 + 4 * fgrp);
            const int4 la = *(const int4*)lp, lb = *(const int4*)(lp + 16);
            int L[8] = {la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w};
            if constexpr (MASK) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (!group_allowed(allow, L[e])) L[e] = -1;
            }
            int runs = 0, last = -1;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (L[e] >= 0 && L[e] != last) { ++runs; last = L[e]; }
            const bool many = __builtin_amdgcn_ballot_w64(runs > 2) != 0;   // wave-uniform
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mi = hm * 4 + i;
                const bool qlive = qbase + mi * 16 < nq_real;
                size_t uo = (size_t)(mi * 16) * n_groups;
                asm volatile("" : "+s"(uo));
                uint32_t* gb = qlive ? gb0 + uo : gbest;               // always inside gbest: the loads below are unconditional
                // Many runs (scattered labels: every row its own run): read the keys the eight rows' groups hold now.  gbest only
                // grows, so a key at or below a value read here (however stale) cannot raise it and its atomic is skipped; only
                // the few rows that beat their group's running maximum still pay one.  Few runs (a video boundary inside the
                // stream): the reads would only stall the pipeline, the one or two atomics go out unconditionally.
                uint32_t seen[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                if (many) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) seen[e] = gb[L[e] < 0 ? 0 : L[e]];
                }
                int cur = -1;
                uint32_t cur_seen = 0;
                float m = NEG;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = acc[mi][hn * 2 + (e >> 2)][e & 3];
                    if (L[e] < 0) continue;
                    if (L[e] != cur) {                                 // a run ends: at most one atomic for it
                        if (cur >= 0 && qlive && score_key(m) > cur_seen) atomicMax(gb + cur, score_key(m));
                        cur = L[e]; cur_seen = seen[e]; m = v;
                    } else {
                        m = fmaxf(m, v);
                    }
                }
                if (cur >= 0 && qlive && score_key(m) > cur_seen) atomicMax(gb + cur, score_key(m));
                acc[mi][hn * 2] = f32x4{0.f, 0.f, 0.f, 0.f};
                acc[mi][hn * 2 + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[hm * 4 + i][hn * 2] = f32x4{0.f, 0.f, 0.f, 0.f};
                acc[hm * 4 + i][hn * 2 + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    auto barrier = [&]() __attribute__((always_inline)) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    int sg_cur = -2, sg_prev = -2;
    // One K-tile of stream256_run's schedule (scan_stream256.h has the phases, hazards and waits), with the row tile's label
    // handed to its folds: `last` = final K-tile of a row tile, the fourth quadrant's fold lands in phase 1 of the next
    // K-tile (`fold_prev`).
    auto tile = [&](int kt, int bufi, bool last, bool fold_prev, int t) __attribute__((always_inline)) {
        const char* buf = smem + bufi * G2_BUF;
        const bool next = kt + 1 < total, next2 = kt + 2 < total;
        if (fold_prev) fold(1, 0, t - 1, sg_prev, true);
        load_a(buf, 0); load_w(buf, 0);
        if (next) stage(bufi ^ 1, 1, kt + 1);
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(0, 0);
        barrier();
        if (last) fold(0, 0, t, sg_cur, false);
        load_w(buf, 1);
        if (next) stage(bufi ^ 1, 2, kt + 1);
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(0, 1);
        barrier();
        if (last) fold(0, 1, t, sg_cur, true);
        load_a(buf, 1);
        if (next) stage(bufi ^ 1, 3, kt + 1);
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(1, 1);
        barrier();
        if (last) fold(1, 1, t, sg_cur, false);
        load_w(buf, 0);
        if (next2) { stage(bufi, 0, kt + 2); asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
        else       { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mfma_quadrant(1, 0);
        barrier();
    };

    stage(0, 0, 0); stage(0, 1, 0); stage(0, 2, 0); stage(0, 3, 0);
    if (total > 1) { stage(1, 0, 1); asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
    else           { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    barrier();

    if (wr == 1) barrier();
    int kk = 0, t = 0;
    for (int kt = 0; kt < total; kt += 2) {
        if (kk == 0) { sg_prev = sg_cur; sg_cur = tile_label(t); }     // fetched a whole row tile before its first use
        tile(kt, 0, false, kk == 0 && t > 0, t);
        ++kk;
        tile(kt + 1, 1, kk + 1 == nk, false, t);
        if (++kk == nk) { kk = 0; ++t; }
    }
    fold(1, 0, 7, sg_cur, true);
    if (wr == 0) barrier();
}

// ---- |q_i| and the |q|^2 range test: one wave per query ----
__global__ __launch_bounds__(64)
void set_query_norm_kernel(const float* __restrict__ queries, int dim, float* __restrict__ qn /*[m]*/, int32_t* __restrict__ flag) {
    const int q = blockIdx.x;
    wave_query_norm2(queries + (size_t)q * dim, dim, [&](float s2, bool covered) {
        qn[q] = sqrtf(s2);
        if (!covered) *flag = 2;
    });
}

// ---- sum16[g] (+)= the chunk's fp16 group maxima, i ascending; a group no row reached (key 0: disallowed) adds nothing ----
__global__ __launch_bounds__(256)
void set_accum_score_kernel(const uint32_t* __restrict__ gbest, int cur, int n_groups, int first, double* __restrict__ sum16) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    double s = first ? 0.0 : sum16[g];
    for (int i = 0; i < cur; ++i) {
        const uint32_t key = gbest[(size_t)i * n_groups + g];
        if (key) s += (double)key_score(key);
    }
    sum16[g] = s;
}

// ---- fp16 pass 2: threshold and candidate groups, one workgroup for the call ----
__global__ __launch_bounds__(256)
void set_threshold_kernel(const double* __restrict__ sum16, int n_groups, int m, int k_sel, int n_allowed,
                          const uint32_t* __restrict__ allow, const float* __restrict__ qn, float eps_rows,
                          const int32_t* __restrict__ goff, uint32_t* __restrict__ skey /*[G] scratch*/, int32_t* __restrict__ cand /*[G]*/,
                          int32_t* __restrict__ candpos /*[G]*/, int32_t* __restrict__ cand_n, uint64_t* __restrict__ ekey /*[G]*/,
                          int32_t* __restrict__ flag, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t hist[256];
    __shared__ double red[4];
    __shared__ uint32_t prefix_s;
    __shared__ int kr_s, cnt_s;
    __shared__ unsigned long long rows_s;
    const int tid = threadIdx.x;
    if (*flag != 0) {                                       // a query outside the bound's range: exact redo
        if (tid == 0) *cand_n = 0;
        return;
    }
    double es = 0.0;
    for (int i = tid; i < m; i += 256) es += (double)qn[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) es += __shfl_xor(es, o);
    if ((tid & 63) == 0) red[tid >> 6] = es;
    if (tid == 0) { cnt_s = 0; rows_s = 0ull; }
    __syncthreads();
    const float Ebar = (float)((double)eps_rows * ((red[0] + red[1]) + (red[2] + red[3])) / (double)m);
    for (int g = tid; g < n_groups; g += 256) {
        const bool ok = allow ? group_allowed(allow, g) : true;
        skey[g] = ok ? score_key((float)(sum16[g] / (double)m)) : 0u;
        candpos[g] = -1;
        ekey[g] = ~0ull;
    }
    __syncthreads();
    const bool all = k_sel >= n_allowed;
    float thr = -__builtin_inff();
    if (!all) {                                             // T = the k_sel-th largest key: radix select, 8 bits at a time
        uint32_t prefix = 0, mask = 0;
        int kr = k_sel;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n_groups; i += 256) {
                const uint32_t v = skey[i];
                if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0;
                for (int b = 255; b >= 0; --b) {
                    const int h = (int)hist[b];
                    if (cum + h >= kr) { prefix_s = prefix | ((uint32_t)b << shift); kr_s = kr - cum; break; }
                    cum += h;
                }
            }
            __syncthreads();
            prefix = prefix_s; kr = kr_s; mask |= 255u << shift;
        }
        thr = (key_score(prefix) - 2.0f * Ebar) - SET_SLACK;
    }
    unsigned long long rows = 0;
    for (int g = tid; g < n_groups; g += 256) {
        const uint32_t v = skey[g];
        if (v != 0u && (all || key_score(v) >= thr)) {
            const int pos = atomicAdd(&cnt_s, 1);           // pos < n_groups: cand holds every group
            cand[pos] = g; candpos[g] = pos;
            rows += (unsigned long long)(goff[g + 1] - goff[g]);
        }
    }
    if (rows) atomicAdd(&rows_s, rows);
    __syncthreads();
    if (tid == 0) {
        const int c = cnt_s;
        if ((int64_t)c * m > SET_KEY_BUDGET) { *flag = 2; *cand_n = 0; }       // more keys than the buffer holds: exact redo
        else { *cand_n = c; counters[1] = rows_s * (unsigned long long)m; }
    }
}

// ---- fp16 pass 3a: exact (distance, tie) minimum of every (candidate, query) over all the candidate's rows.  Workgroup =
// (slice of candidates, query); lpg lanes share a candidate and stride its rows. ----
__global__ __launch_bounds__(256)
void set_cand_keys_kernel(const float* __restrict__ rows, int dim, const float* __restrict__ queries, int m,
                          const int32_t* __restrict__ goff, const int32_t* __restrict__ grows, const int32_t* __restrict__ cand,
                          const int32_t* __restrict__ cand_n, int lpg, uint64_t* __restrict__ ckeys /*[cand][m]*/,
                          const int32_t* __restrict__ flag, const TieOrder tie) {
    if (*flag != 0) return;
    const int cn = *cand_n, tid = threadIdx.x, q = blockIdx.y;
    const int sub = tid / lpg, ls = tid - sub * lpg, nsub = 256 / lpg;
    const float* qv = queries + (size_t)q * dim;
    for (int base = blockIdx.x * nsub; base < cn; base += gridDim.x * nsub) {      // block-uniform trip count
        const int c = base + sub;
        uint64_t best = ~0ull;
        if (c < cn) {
            const int g = cand[c], e = goff[g + 1];
            for (int i = goff[g] + ls; i < e; i += lpg) {
                const int r = grows[i];
                const float d = exact_row_dist(rows + (size_t)r * dim, qv, dim);
                const uint64_t key = dist_key(d, tie_of(tie, r));
                best = key < best ? key : best;
            }
        }
        for (int o = lpg >> 1; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor(best, o, lpg);
            best = other < best ? other : best;
        }
        if (ls == 0 && c < cn) ckeys[(size_t)c * m + q] = best;
    }
}

// ---- fp16 pass 3b: D of every candidate, i ascending in fp64 -> the order key of (D, label) ----
__global__ __launch_bounds__(256)
void set_cand_sum_kernel(const uint64_t* __restrict__ ckeys, int m, const int32_t* __restrict__ cand, const int32_t* __restrict__ cand_n,
                         uint64_t* __restrict__ ekey, const int32_t* __restrict__ flag) {
    if (*flag != 0) return;
    const int cn = *cand_n;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < cn; c += gridDim.x * 256) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += (double)key_dist(ckeys[(size_t)c * m + i]);
        ekey[cand[c]] = dist_key((float)(s / (double)m), (uint32_t)cand[c]);
    }
}

// ---- exact path: the (distance, tie) minimum per (query, group); the reduction of group_block_topk_kernel.  flag != null:
// only a call flagged 2 does anything. ----
template <bool FROM_DIST, bool MASK>
__global__ __launch_bounds__(256)
void set_group_min_kernel(const float* __restrict__ dist, int64_t ld, const float* __restrict__ rows, int dim,
                          const float* __restrict__ queries, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                          int n_groups, int lpg, uint64_t* __restrict__ gmin /*[chunk][n_groups]*/, const int32_t* __restrict__ flag,
                          const TieOrder tie, const uint32_t* __restrict__ allow) {
    if (flag && *flag != 2) return;
    const int q = blockIdx.y, tid = threadIdx.x;
    const int g0 = blockIdx.x * GRP_BLOCK;
    const int sub = tid / lpg, ls = tid - sub * lpg, nsub = 256 / lpg;
    const float* qv = queries + (size_t)q * dim;
    for (int gl = sub; gl < GRP_BLOCK; gl += nsub) {
        const int g = g0 + gl;
        uint64_t best = ~0ull;
        bool live = g < n_groups;
        if constexpr (MASK) live = live && group_allowed(allow, g);
        if (live) {
            const int e = goff[g + 1];
            for (int i = goff[g] + ls; i < e; i += lpg) {
                const int r = grows[i];
                float d;
                if constexpr (FROM_DIST) d = dist[(int64_t)q * ld + r];
                else d = exact_row_dist(rows + (size_t)r * dim, qv, dim);
                const uint64_t key = dist_key(d, tie_of(tie, r));
                best = key < best ? key : best;
            }
        }
        for (int o = lpg >> 1; o > 0; o >>= 1) {
            const uint64_t other = __shfl_xor(best, o, lpg);
            best = other < best ? other : best;
        }
        if (ls == 0 && g < n_groups) gmin[(size_t)q * n_groups + g] = best;
    }
}

// ---- exact path: acc[g] (+)= (double)d(i, g) for the chunk's i ascending; plain loads and stores ----
__global__ __launch_bounds__(256)
void set_accum_dist_kernel(const uint64_t* __restrict__ gmin, int cur, int n_groups, int first, double* __restrict__ acc,
                           const int32_t* __restrict__ flag) {
    if (flag && *flag != 2) return;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    double s = first ? 0.0 : acc[g];
    for (int i = 0; i < cur; ++i) {
        const uint64_t key = gmin[(size_t)i * n_groups + g];
        if (key != ~0ull) s += (double)key_dist(key);
    }
    acc[g] = s;
}

__global__ __launch_bounds__(256)
void set_final_exact_kernel(const double* __restrict__ acc, int n_groups, int m, const uint32_t* __restrict__ allow,
                            uint64_t* __restrict__ ekey, const int32_t* __restrict__ flag) {
    if (flag && *flag != 2) return;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const bool ok = allow ? group_allowed(allow, g) : true;
    ekey[g] = ok ? dist_key((float)(acc[g] / (double)m), (uint32_t)g) : ~0ull;
}

// ---- selection: each block of 256 groups ranks its keys by counting (they are distinct: the low word is the label) and
// lists its k_local smallest; one workgroup then takes the k smallest of the lists by k rounds of "smallest above the
// previous one" (group_merge_kernel's selection). ----
__global__ __launch_bounds__(256)
void set_select_block_kernel(const uint64_t* __restrict__ ekey, int n_groups, int k_local, uint64_t* __restrict__ partial /*[blocks][k_local]*/) {
    __shared__ uint64_t gk[256];
    const int tid = threadIdx.x, g = blockIdx.x * 256 + tid;
    const uint64_t mine = g < n_groups ? ekey[g] : ~0ull;
    gk[tid] = mine;
    __syncthreads();
    int valid = 0, rank = 0;
    for (int j = 0; j < 256; ++j) { const uint64_t o = gk[j]; valid += o != ~0ull; rank += o < mine; }
    uint64_t* out = partial + (size_t)blockIdx.x * k_local;
    if (mine != ~0ull && rank < k_local) out[rank] = mine;
    for (int j = valid + tid; j < k_local; j += 256) out[j] = ~0ull;
}

__global__ __launch_bounds__(256)
void set_select_merge_kernel(const uint64_t* __restrict__ partial, int64_t total, int k, int32_t* __restrict__ groups_out,
                             float* __restrict__ dist_out, const int32_t* __restrict__ flag, unsigned long long* __restrict__ counters) {
    __shared__ uint64_t red[4];
    const int tid = threadIdx.x;
    if (tid == 0 && counters) {
        if (*flag == 0) { counters[0] = 1ull; counters[2] = 0ull; }
        else { counters[0] = 0ull; counters[1] = 0ull; counters[2] = 1ull; }
    }
    uint64_t prev = 0;
    for (int j = 0; j < k; ++j) {
        uint64_t best = ~0ull;
        for (int64_t i = tid; i < total; i += 256) {
            const uint64_t key = partial[i];
            if ((j == 0 || key > prev) && key < best) best = key;
        }
        best = block_min_u64(best, red, tid);
        if (best == ~0ull) {                                  // block-uniform
            for (int jj = j + tid; jj < k; jj += 256) { groups_out[jj] = -1; dist_out[jj] = __builtin_inff(); }
            break;
        }
        if (tid == 0) { groups_out[j] = (int32_t)(uint32_t)best; dist_out[j] = key_dist(best); }
        prev = best;
    }
}

// ---- match_rows[j][i] = the row of result group j that attains d(i, group j).  The proven fp16 path reads the candidate's
// stored keys; the exact path (flag null or 2) recomputes the minimum, one wave per (winner, query). ----
__global__ __launch_bounds__(256)
void set_match_rows_kernel(const int32_t* __restrict__ groups_out, int m, const float* __restrict__ rows, int dim,
                           const float* __restrict__ queries, const int32_t* __restrict__ goff, const int32_t* __restrict__ grows,
                           const int32_t* __restrict__ candpos, const uint64_t* __restrict__ ckeys, const int32_t* __restrict__ flag,
                           int32_t* __restrict__ match /*[k][m]*/, const TieOrder tie) {
    const int j = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = groups_out[j];
    const bool stored = flag && *flag == 0;
    for (int i = blockIdx.y * 4 + wave; i < m; i += gridDim.y * 4) {       // wave-uniform
        int32_t r_out = -1;
        if (g >= 0 && stored) {
            r_out = tie_row(tie, (uint32_t)ckeys[(size_t)candpos[g] * m + i]);
        } else if (g >= 0) {
            const float* qv = queries + (size_t)i * dim;
            uint64_t best = ~0ull;
            const int e = goff[g + 1];
            for (int p = goff[g] + lane; p < e; p += 64) {
                const int r = grows[p];
                const float d = exact_row_dist(rows + (size_t)r * dim, qv, dim);
                const uint64_t key = dist_key(d, tie_of(tie, r));
                best = key < best ? key : best;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t other = __shfl_xor(best, o);
                best = other < best ? other : best;
            }
            r_out = tie_row(tie, (uint32_t)best);
        }
        if (lane == 0) match[(size_t)j * m + i] = r_out;
    }
}

}  // namespace vq
