// What an fp16 search (search_fp16 in vq_index.hip) launches: plan, then launch.
//
//   scan_switches_from_env()   the five A/B switches, read once per handle at vq_index_create.
//   plan_scan(...)             pure host arithmetic: (dim, rows, queries, k, switches, build kind) -> which scan and which
//                              re-score kernel run and the geometry that follows from the choice, or an error for a kind
//                              this build does not carry.  No HIP here; vq_debug_scan_plan returns it on a machine without a GPU
//                              (tests/test_scan_plan_cpu.py).
//   q_pad / q_tiles / scan_grid / rescore_grid   the per-chunk values.
// launch_scan and launch_rescore (vq_index.hip) are one switch each over the plan's kinds.
//
// The geometry constants are the kernels' (knn_scan_f16.h, knn_scan_small.h, knn_scan_fold.h, gemm_mfma256.h); vq_index.hip
// asserts that the two sets agree.
#pragma once
#include "../../include/vq_amd.h"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace vq {

// The values of $VQ_AMD_SCAN (SCAN_STREAM excepted: batches of <= SP_STREAM_MAX_Q queries take it whatever the switch says).
enum ScanKind : int {
    SCAN_TILE128 = 1,            // 128 queries x 1024 rows per workgroup (scan_f16_top2_kernel): any dim % 64 == 0, key layout 1
    SCAN_PHASE4 = 2,             // experiment: 256 x 2048, four-phase mainloop (experiments/knn_scan_phase4.h)
    SCAN_STREAM = 3,             // small batches: the HBM-bound streaming scan (knn_scan_small.h), key layout 3
    SCAN_DEEP = 4,               // experiment: 256 x 2048, deep prefetch, fold at the row-tile boundary (experiments/knn_scan_deep.h)
    SCAN_FOLD = 5,               // 256 x 2048, deep prefetch, fold spread behind the MFMA clusters (knn_scan_fold.h): the default, dim % 128 == 0
    SCAN_FOLD_NONE = 51,         // diagnostic builds: scan5 without fold (keys invalid)
    SCAN_FOLD_AFTER = 52,        //                    ... fold not interleaved
    SCAN_FOLD_CLEAR = 53,        //                    ... the fold clears its accumulators (no C = 0 MFMAs)
};

enum RescoreKind : int {
    RESCORE_BATCH8 = 0,          // rescore_verify_kernel: 8 queries per workgroup, k <= 20
    RESCORE_LARGE4,              // rescore_verify_large_kernel: 4 queries per workgroup, k in (20, 64]
    RESCORE_XLARGE4,             // rescore_verify_xlarge_kernel: 4 queries per workgroup, k in (64, 100]
    RESCORE_LARGE1,              // rescore_verify_large1_kernel: the streaming scan's keys, one query per workgroup, k in (20, 64]
    RESCORE_XLARGE1,             // rescore_verify_xlarge1_kernel: ... k in (64, 100]
    RESCORE_SMALL32,             // rescore_verify_small_kernel: the streaming scan's keys, one query per workgroup, 32 candidates, k <= 20
    RESCORE_SMALL64,             // rescore_verify_small64_kernel: ... 64 candidates, k in (20, 40]
};

constexpr int SP_STREAM_ROWS = 128;                               // rows per lane stream, every scan
constexpr int SP_TILE128_QT = 128, SP_TILE128_RANGE = 1024;       // queries / rows per workgroup
constexpr int SP_BATCH_QT = 256, SP_BATCH_RANGE = 2048;           // ... of the 256 x 2048 scans
constexpr int SP_STREAM_QB = 16, SP_STREAM_FUSED_MAX_Q = 4, SP_STREAM_MAX_Q = 96;
constexpr int SP_PHASE4_LDS = 128 << 10, SP_FOLD_LDS = 160 << 10; // two K-tile buffers; + the running keys: the whole LDS of a CU
constexpr int SP_K_SMALL = 20, SP_K_SMALL64 = 40, SP_K_MID = 64;
constexpr int SP_BATCH8_QPW = 8, SP_LARGE_QPW = 4;
constexpr int SP_SMALL32_C = 32, SP_SMALL64_C = 64;               // candidate rows the one-query kernels stage in LDS
constexpr int64_t SP_KEY_BUDGET = (int64_t)1 << 27;               // 128 Mi (stream, query) pairs = 1 GiB of keys per chunk

struct ScanSwitches {            // A/B switches of the fp16 search
    int scan = SCAN_FOLD;        // $VQ_AMD_SCAN: 1, 2, 4, 51, 52, 53; anything else is 5
    bool small_scan = true;      // $VQ_AMD_SCAN_SMALL=0: batches of <= SP_STREAM_MAX_Q queries also take the MFMA-tile scan
    int rb = 2;                  // $VQ_AMD_SCAN_RB, 0..5: see plan_scan
    bool rescore_qpw4 = false;   // $VQ_AMD_RESCORE_QPW4=1: the four-queries-per-workgroup kernels for small batches with k > 20 too
    bool rescore_small64 = true; // $VQ_AMD_RESCORE_SMALL64=0: no 64-candidate one-query kernel
};

static inline ScanSwitches scan_switches_from_env() {
    ScanSwitches s;
    if (const char* e = getenv("VQ_AMD_SCAN")) {
        const int v = atoi(e);
        s.scan = (v == 1 || v == 2 || v == 4 || v == 51 || v == 52 || v == 53) ? v : SCAN_FOLD;
    }
    if (const char* e = getenv("VQ_AMD_SCAN_SMALL")) s.small_scan = atoi(e) != 0;
    if (const char* e = getenv("VQ_AMD_SCAN_RB")) s.rb = std::min(5, std::max(0, atoi(e)));
    if (const char* e = getenv("VQ_AMD_RESCORE_QPW4")) s.rescore_qpw4 = atoi(e) == 1;
    if (const char* e = getenv("VQ_AMD_RESCORE_SMALL64")) s.rescore_small64 = atoi(e) != 0;
    return s;
}

struct ScanPlan {
    int err = 0;                 // VQ_ERR_INVALID with `msg` when this build does not carry the kind the switch names
    char msg[192];
    int scan = 0;                // ScanKind
    int QT = 0, RANGE = 0;       // queries / rows per scan workgroup (STREAM: per pass / per stream)
    int64_t n_pad = 0, streams = 0;      // rows padded to whole ranges; 128-row streams = keys per query
    int ranges = 0;
    int64_t q_chunk = 0;         // queries per chunk (the key budget), a multiple of QT
    int nqg = 1;                 // STREAM: groups of 16 queries the scan holds per pass
    bool fused_q = false;        // STREAM: the scan rounds the (one to four) queries itself, no conversion launch
    int rb = 2;                  // the 256 x 2048 scans: log2 of the row ranges per block of 32 workgroups
    int scan_lds = 0;            // dynamic LDS of the scan, bytes
    int rescore = 0;             // RescoreKind
    int rescore_qpw = 0;         // queries per re-score workgroup
    int rescore_lds = 0;         // dynamic LDS of the re-score, bytes
    int layout = 0;              // key layout the re-score is told: 1 TILE128, 2 the 256 x 2048 scans, 3 STREAM
    bool rescore_files_flags = false;    // the re-score workgroup writes the flagged list and the counters itself: no collect_flags_kernel
};

// the per-chunk values: `cur` queries of the chunk
static inline int64_t q_pad(const ScanPlan& p, int cur) { return ((int64_t)cur + p.QT - 1) / p.QT * p.QT; }
static inline int q_tiles(const ScanPlan& p, int cur) { return (int)(q_pad(p, cur) / p.QT); }
static inline int n_chunks(const ScanPlan& p, int nq) { return (int)((nq + p.q_chunk - 1) / p.q_chunk); }
// the 256 x 2048 scans: blocks of 32 workgroups along the ranges (a kernel argument)
static inline int range_groups(const ScanPlan& p) { return (p.ranges + (1 << p.rb) - 1) >> p.rb; }
struct ScanGrid { int x, y; };
static inline ScanGrid scan_grid(const ScanPlan& p, int cur) {
    const int qt = q_tiles(p, cur);
    if (p.scan == SCAN_STREAM) return ScanGrid{(int)((p.streams + 3) / 4), qt};         // four waves = four streams per workgroup
    if (p.scan == SCAN_TILE128) return ScanGrid{qt * p.ranges, 1};
    const int qb = 32 >> p.rb;                                                          // query tiles per block
    return ScanGrid{range_groups(p) * ((qt + qb - 1) / qb) * 32, 1};
}
static inline int rescore_grid(const ScanPlan& p, int cur) { return (cur + p.rescore_qpw - 1) / p.rescore_qpw; }

// diag_build / experiments_build: what `make DIAG=1` / `make EXPERIMENTS=1` add.
static inline ScanPlan plan_scan(int dim, int64_t n, int nq, int k, const ScanSwitches& sw, bool diag_build, bool experiments_build) {
    ScanPlan p;
    if ((sw.scan == SCAN_PHASE4 || sw.scan == SCAN_DEEP) && !experiments_build) {       // measured and superseded
        p.err = VQ_ERR_INVALID;
        snprintf(p.msg, sizeof(p.msg), "VQ_AMD_SCAN=%d is an experiment: rebuild with `make EXPERIMENTS=1`", sw.scan);
        return p;
    }
    if (sw.scan > SCAN_FOLD && !diag_build) {
        p.err = VQ_ERR_INVALID;
        snprintf(p.msg, sizeof(p.msg), "VQ_AMD_SCAN=%d is built into diagnostic libraries only: `make DIAG=1 OUT=... OBJDIR=...`", sw.scan);
        return p;
    }
    // small batches (the reference's one-query-at-a-time search, video_search_system.py:297) take the HBM-bound
    // streaming scan; the 256-query MFMA tile is for batches
    const bool small = nq <= SP_STREAM_MAX_Q && (dim == 512 || dim == 256 || dim == 768) && sw.small_scan;
    p.scan = small ? SCAN_STREAM : dim % 128 != 0 ? SCAN_TILE128 : sw.scan;             // the 256 x 2048 scans need dim % 128 == 0
    const bool stream = p.scan == SCAN_STREAM, tile128 = p.scan == SCAN_TILE128;
    p.nqg = stream && nq > SP_STREAM_QB && dim <= 512 ? 2 : 1;                          // 768-d: 96 + 96 VGPRs for one group
    p.fused_q = stream && nq <= SP_STREAM_FUSED_MAX_Q;
    p.QT = stream ? SP_STREAM_QB * p.nqg : tile128 ? SP_TILE128_QT : SP_BATCH_QT;
    p.RANGE = stream ? SP_STREAM_ROWS : tile128 ? SP_TILE128_RANGE : SP_BATCH_RANGE;
    p.n_pad = (n + p.RANGE - 1) / p.RANGE * p.RANGE;
    p.streams = p.n_pad / SP_STREAM_ROWS;
    p.ranges = (int)(p.n_pad / p.RANGE);
    const int64_t nq_pad = ((int64_t)nq + p.QT - 1) / p.QT * p.QT;
    p.q_chunk = std::min<int64_t>(std::max<int64_t>(p.QT, SP_KEY_BUDGET / p.streams / p.QT * p.QT), nq_pad);
    // workgroup -> (row range, query tile) blocking inside an XCD's 32 concurrent workgroups: $VQ_AMD_SCAN_RB = log2 of the
    // ranges per block (default 2: 4 ranges x 8 query tiles); the two experiments have 4 x 8 compiled in.  Measured with the
    // plain "query tile fastest" order: 55 % of the L2 requests missed (47 GB from beyond L2 for a 1 GB matrix: 32 distinct
    // 256 KB query tiles do not fit a 4 MiB L2).  A 4 x 8 block walks its ranges in step: the live set is 4 row tiles + 8 query
    // tiles = 3 MiB, every row tile is fetched once per 8 workgroups, and blocks advance range-group fastest so the next block
    // reuses the query tiles.
    p.rb = p.scan >= SCAN_FOLD ? sw.rb : 2;
    p.scan_lds = stream || tile128 ? 0 : p.scan == SCAN_PHASE4 ? SP_PHASE4_LDS : SP_FOLD_LDS;
    p.layout = stream ? 3 : tile128 ? 1 : 2;

    const bool large = k > SP_K_SMALL;                   // k in (20, 64]: the wide candidate pool, whatever scan produced the keys
    // k in (20, 40] from the streaming scan (the caller's k * 2 for a user k of 11 .. 20): the 64-candidate form of the single-query kernel
    const bool small64 = stream && large && k <= SP_K_SMALL64 && dim <= 512 && !sw.rescore_qpw4 && sw.rescore_small64;
    if (small64) p.rescore = RESCORE_SMALL64;
    else if (large && stream && !sw.rescore_qpw4) p.rescore = k > SP_K_MID ? RESCORE_XLARGE1 : RESCORE_LARGE1;
    else if (large) p.rescore = k > SP_K_MID ? RESCORE_XLARGE4 : RESCORE_LARGE4;
    else p.rescore = stream ? RESCORE_SMALL32 : RESCORE_BATCH8;
    const bool one_wg = p.rescore == RESCORE_SMALL32 || p.rescore == RESCORE_SMALL64;   // one workgroup per query, candidate rows + the query in LDS
    p.rescore_qpw = p.rescore == RESCORE_BATCH8 ? SP_BATCH8_QPW : p.rescore == RESCORE_LARGE4 || p.rescore == RESCORE_XLARGE4 ? SP_LARGE_QPW : 1;
    p.rescore_lds = one_wg ? ((p.rescore == RESCORE_SMALL64 ? SP_SMALL64_C : SP_SMALL32_C) * (dim + 4) + dim) * 4 : 0;
    p.rescore_files_flags = one_wg && nq == 1;           // a single query's workgroup has seen the only flag
    return p;
}

}  // namespace vq
