// Which GEMM kernel a shape gets: plan, then launch.
//
//   plan_gemm(...)      pure host arithmetic: (shape, leading dimensions, epilogue kind, forced kernel id, build kind,
//                       environment switches) -> at most two steps {kernel, rows, first row, tiles per workgroup} or an
//                       error.  No HIP call; vq_debug_gemm_plan returns it on a machine without a GPU.
//   launch_gemm_auto    the single entry of every tower GEMM and of vq_debug_gemm: plan_gemm, then one switch over the
//                       launchers of gemm_mfma*.h.
//
// Auto (id 0) picks the 256x256 deep-prefetch kernel when the problem tiles by it and yields at least 128 workgroups,
// else the 128x128 kernel; the 160-row ring tiles where they put one workgroup on more CUs than 256-row tiles would;
// and sends the rows of a thin last round of 256x256 tiles to the 128x128 kernel.  Concurrent handles (id 6) keep
// neither the 160-row tiles nor the tail split - other streams fill the idle CUs - and give the LayerNorm-consuming
// GEMMs three or four tiles per workgroup.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "gemm_mfma256.h"
#include "gemm_mfma160.h"
#include "gemm_mfma256d.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace vq {

// The values of $VQ_AMD_GEMM and of bits 1-5 of vq_debug_gemm's flags: they do not change.  A plan step names its
// launcher by the id that forces that launcher.
enum GemmKernel : int {
    GK_AUTO = 0,                 // the dispatch described above
    GK_TILE128 = 1,              // 128x128 (gemm_mfma.h) everywhere
    GK_PHASE4 = 2,               // 256x256 four-phase (gemm_mfma256.h)
    GK_EXP_RING256 = 3,          // experiment: 256x256 ring
    GK_EXP_PERSISTENT = 4,       // experiment: persistent 256x256
    GK_RING160 = 5,              // 160x256 ring (gemm_mfma160.h)
    GK_AUTO_NO160 = 6,           // auto without the 160-row tiles and the tail split: concurrent handles
    GK_EXP_WAVE4 = 7,            // experiment: four-wave 256x256
    GK_DEEP = 8,                 // 256x256 deep prefetch, buffer_load..lds staging (gemm_mfma256d.h): the default 256x256 mainloop
    GK_EXP_PHASE2 = 9,           // experiment: two-phase 256x256
    GK_EXP_FUSED = 10,           // experiment: gemm_mfma256f.h
    GK_DEEP_GLOBAL_LDS = 11,     // the deep prefetch with global_load_lds staging
    GK_EXP_128X256 = 12,         // experiment: 128x256 tiles, two workgroups per CU, wherever the 256x256 kernel would run
    GK_EXP_128X256_ANY = 13,     //             ... on every shape that tiles
    GK_AUTO_MULTI = 14,          // as 6
    GK_MULTI_WHERE_WORTH = 15,   // multi-tile workgroups of three wherever the shape allows
    GK_MULTI_ANY = 16,           // tests: the multi-tile kernel (gemm_tn256dm) on any shape that tiles; as a step: that kernel
    GK_EXP_128X256P_LAG = 20,    // experiment: persistent out-of-phase 128x256 tiles, second workgroup of a CU half a tile late
    GK_EXP_128X256P = 21,        //             ... no lag (the in-step control of the A/B)
    GK_ASM256 = 24,              // diagnostic builds: the hand-scheduled four-wave 256x256 loop (gemm_asm256.h) on every shape that tiles
};

// Tile of the two 128x256 experiments (their headers are not part of a product build; experiments/gemm_experiments.h
// asserts that they agree).
constexpr int GX_BM = 128, GX_BN = 256, GX_SUB_K = 32;

struct GemmOptions {             // the environment switches of the dispatch, read once per process
    bool deep = true;            // $VQ_AMD_GEMM256=4phase: auto picks the second-generation mainloop (A/B switch)
    bool multi = true;           // $VQ_AMD_GEMM_MULTI=0: one tile per workgroup everywhere
    int multi_min_wgs = 128;     // $VQ_AMD_GEMM_MULTI_MIN: fewest workgroups a multi-tile launch may leave.  Default 128 [r03]: with three batches
                                 // in flight qkv (450 tiles -> 150 workgroups) gains 0.6-0.9 % frames/s too (192 kept it on single tiles)
    bool tail_split = true;      // $VQ_AMD_GEMM_TAIL=0 keeps one launch per GEMM
    int tiles_per_wg = 0;        // $VQ_AMD_GEMM_TPW forces the tiles per multi-tile workgroup
    bool use160 = true;          // $VQ_AMD_GEMM160=0 keeps the 256x256 kernel for every shape
};

static inline const GemmOptions& gemm_options() {
    static const GemmOptions opt = [] {
        GemmOptions o;
        auto off = [](const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; };
        if (const char* e = getenv("VQ_AMD_GEMM256")) o.deep = strcmp(e, "4phase") != 0;
        o.multi = !off("VQ_AMD_GEMM_MULTI");
        if (const char* e = getenv("VQ_AMD_GEMM_MULTI_MIN")) o.multi_min_wgs = atoi(e);
        o.tail_split = !off("VQ_AMD_GEMM_TAIL");
        if (const char* e = getenv("VQ_AMD_GEMM_TPW")) o.tiles_per_wg = atoi(e);
        o.use160 = !off("VQ_AMD_GEMM160");
        return o;
    }();
    return opt;
}

static inline bool gemm_use160() { return gemm_options().use160; }

// True when 160-row tiles fill more CUs than 256-row tiles in a single wave of workgroups.
static inline bool prefer_tn160(int M, int N, int K) {
    if (M % G5_BM || N % G5_BN || K % G3_SUB_K || K < (G5_NSLOT - 1) * G3_SUB_K) return false;
    const int64_t t160 = (int64_t)(M / G5_BM) * (N / G5_BN);
    const int64_t t256 = (int64_t)((M + G2_BM - 1) / G2_BM) * (N / G2_BN);
    return t160 <= 256 && t256 < 200 && t160 > t256;
}

struct GemmStep { int kernel, rows, row0, tiles_per_wg; };      // kernel: a GemmKernel; tiles_per_wg: GK_MULTI_ANY steps only, else 1
struct GemmPlan {
    int n_steps = 0;
    GemmStep step[2];
    int err = 0;                 // VQ_ERR_* with `msg` when the id does not exist in this build
    char msg[192];
};

// Tile quantisation: T tiles of 256x256 over 256 CUs run ceil(T/256) rounds.  When the last round is less than half
// full, its tiles' rows go to the 128x128 kernel instead (4x the workgroups, two per CU: one short round) - same K
// order per output element, so the results are bit-identical.  Returns the rows that stay with the 256x256 kernel
// (whole tile rows inside the full rounds), 0 for no split.
static inline int gemm_tail_split_rows(int M, int N) {
    const int tiles_n = N / G2_BN;
    const int64_t tiles = (int64_t)(M / G2_BM) * tiles_n;
    const int rem = (int)(tiles % 256);
    if (tiles <= 256 || rem == 0 || rem >= 128) return 0;
    const int m_main = (int)((tiles - rem) / tiles_n) * G2_BM;
    return m_main > 0 && m_main < M ? m_main : 0;
}

// row_in: the epilogue consumes per-row LayerNorm statistics (epi_row_in), so only the kernels with the row-stat
// prologue apply (deep, multi-tile, 128x128).  diag_build / experiments_build: what `make DIAG=1` / `make EXPERIMENTS=1` add.
static inline GemmPlan plan_gemm(int M, int N, int K, int lda, int ldw, bool row_in, int force,
                                 bool diag_build, bool experiments_build, const GemmOptions& opt) {
    GemmPlan p;
    auto one = [&](int kernel, int tpw = 1) { p.n_steps = 1; p.step[0] = GemmStep{kernel, M, 0, tpw}; return p; };
    auto experiment = [&](int kernel) {           // measured and rejected mainloops are not part of the product library
        if (experiments_build) return one(kernel);
        p.err = VQ_ERR_INVALID;
        snprintf(p.msg, sizeof(p.msg), "gemm kernel %d is an experiment: rebuild with `make EXPERIMENTS=1`", kernel);
        return p;
    };
    const bool fits256 = M % G2_BM == 0 && N % G2_BN == 0 && K % (2 * G2_BK) == 0;
    const bool fits128x256 = M % GX_BM == 0 && N % GX_BN == 0 && K % (2 * GX_SUB_K) == 0 && K >= 4 * GX_SUB_K;
    const bool ld64 = lda % 64 == 0 && ldw % 64 == 0;         // the lane-offset staging of the multi-tile and two-phase kernels
    const int tiles_n = N / G2_BN;
    const int64_t tiles = (int64_t)(M / G2_BM) * tiles_n;

    // ids that name one kernel for every shape that tiles: a shape that does not is dispatched as for a concurrent handle
    int id = force;
    if (id == GK_ASM256) {
        if (!diag_build) {
            p.err = VQ_ERR_INVALID;
            snprintf(p.msg, sizeof(p.msg), "gemm kernel 24 (hand-scheduled four-wave loop) is built into diagnostic libraries only: `make DIAG=1 OUT=... OBJDIR=...`");
            return p;
        }
        if (fits256) return one(GK_ASM256);
        id = GK_AUTO_NO160;
    }
    if (id == GK_EXP_128X256P_LAG || id == GK_EXP_128X256P || id == GK_EXP_128X256 || id == GK_EXP_128X256_ANY) {
        const bool everywhere = id != GK_EXP_128X256;
        if (!experiments_build || (fits128x256 && (everywhere || (int64_t)(M / GX_BM) * (N / GX_BN) >= 256))) return experiment(id);
        id = GK_AUTO_NO160;
    }
    if (id == GK_EXP_PHASE2 && !experiments_build) return experiment(id);

    bool want256;                // the 256x256 kernel, if the shape tiles by it
    int best = GK_DEEP;          // which 256x256 kernel that is
    bool may_split;              // a lone batch: the thin last round goes to the 128x128 kernel
    if (row_in) {
        want256 = id != GK_TILE128 && (id == GK_DEEP || tiles >= 128);
        may_split = id == GK_AUTO;
        if (fits256 && want256) {
            if (id == GK_EXP_PHASE2 && ld64) return experiment(id);
            // Three tiles of a tile row per workgroup where that still leaves >= multi_min_wgs workgroups (fc1 and, since round 3, qkv at batch
            // 256): the second and third tile's first operands land under the previous epilogue (fc1 -3.5 % with one batch in flight,
            // +0.5 % frames/s with three; qkv drops to 150 workgroups: -29 % alone, +0.6-0.9 % frames/s with three batches in flight -
            // the idle CUs belong to the other batches then).  Concurrent handles only: a lone batch keeps the tail split.
            const bool worth = (id == GK_AUTO_NO160 || id == GK_AUTO_MULTI) && opt.multi && tiles / 3 >= opt.multi_min_wgs;
            if ((worth || id == GK_MULTI_WHERE_WORTH) && ld64 && tiles_n % 3 == 0) {
                // [r04] FOUR tiles per workgroup where that fills the chip's 256 CUs better than three: ViT-L/14@336's q|k|v GEMM is 73 x 12
                // tiles = 292 workgroups of three (two rounds, the second 14 % full) or 219 of four (one round, 86 % full).
                auto fill = [&](int t) { const int64_t w = tiles / t; return (double)w / (double)(((w + 255) / 256) * 256); };
                int tpw = 3;
                if (tiles_n % 4 == 0 && tiles / 4 >= opt.multi_min_wgs && fill(4) > fill(3) + 0.05) tpw = 4;
                if (opt.tiles_per_wg >= 1 && tiles_n % opt.tiles_per_wg == 0) tpw = opt.tiles_per_wg;
                return one(GK_MULTI_ANY, tpw);
            }
        }
    } else {
        if (id == GK_RING160 || (id == GK_AUTO && opt.use160 && prefer_tn160(M, N, K))) return one(GK_RING160);
        if (id == GK_DEEP || id == GK_DEEP_GLOBAL_LDS || id == GK_PHASE4) return one(id);
        if (id == GK_EXP_WAVE4 || id == GK_EXP_FUSED) return experiment(id);
        if ((id == GK_EXP_RING256 || id == GK_EXP_PERSISTENT) && (!experiments_build || fits256)) return experiment(id);
        if (id == GK_EXP_PHASE2 && fits256 && ld64) return experiment(id);
        if (id == GK_MULTI_WHERE_WORTH && fits256 && ld64 && tiles_n % 3 == 0 && tiles >= 128) return one(GK_MULTI_ANY, 3);
        if (id == GK_MULTI_ANY && fits256 && ld64)
            return one(GK_MULTI_ANY, tiles_n % 3 == 0 ? 3 : tiles_n % 4 == 0 ? 4 : tiles_n % 2 == 0 ? 2 : 1);
        // whatever is left is auto without the 160-row tiles, or (any other id from 2 up) the 256x256 kernel wherever it tiles
        const bool is_auto = id == GK_AUTO || id == GK_AUTO_NO160 || id == GK_AUTO_MULTI || id == GK_MULTI_WHERE_WORTH || id == GK_MULTI_ANY;
        want256 = is_auto ? tiles >= 128 : id >= 2;
        best = opt.deep ? GK_DEEP : GK_PHASE4;
        may_split = id == GK_AUTO || id == GK_MULTI_ANY;
    }
    if (!(fits256 && want256)) return one(GK_TILE128);
    // not for concurrent handles: other streams fill the idle CUs of a thin round
    const int m_main = may_split && opt.tail_split ? gemm_tail_split_rows(M, N) : 0;
    if (!m_main) return one(best);
    p.n_steps = 2;
    p.step[0] = GemmStep{best, m_main, 0, 1};
    p.step[1] = GemmStep{GK_TILE128, M - m_main, m_main, 1};
    return p;
}

}  // namespace vq

#ifdef VQ_DIAG       // the hand-scheduled four-wave kernel (id 24) changed nothing in frames/s (DESIGN.md section 4 "Round 3" (5)): diagnostic builds only
#include "gemm_asm256.h"
#endif
#ifdef VQ_GEMM_EXPERIMENTS      // `make EXPERIMENTS=1`: the measured-and-rejected mainloops and launch_gemm_experiment
#include "experiments/gemm_experiments.h"
namespace vq { constexpr bool GEMM_EXPERIMENTS_BUILD = true; }
#else
namespace vq { constexpr bool GEMM_EXPERIMENTS_BUILD = false; }
#endif

namespace vq {

#ifdef VQ_DIAG
constexpr bool GEMM_DIAG_BUILD = true;
#else
constexpr bool GEMM_DIAG_BUILD = false;
#endif

// defined by experiments/gemm_experiments.h; a product build never instantiates the call below
template <bool IS_F16, class Epi>
static int launch_gemm_experiment(hipStream_t st, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                                  int M, int N, int K, const Epi& epi, int kernel);

template <bool IS_F16, class Epi>
static int launch_gemm_auto(hipStream_t st, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                            int M, int N, int K, const Epi& epi, int force = 0) {
    constexpr bool row_in = epi_row_in<Epi>::value;
    const GemmPlan plan = plan_gemm(M, N, K, lda, ldw, row_in, force, GEMM_DIAG_BUILD, GEMM_EXPERIMENTS_BUILD, gemm_options());
    if (plan.err) return fail(plan.err, "%s", plan.msg);
    for (int i = 0; i < plan.n_steps; ++i) {
        const GemmStep& s = plan.step[i];
        int rc;
        // Row-stat epilogues instantiate tn256d, tn256dm and tn only (the kernels with the row-stat prologue); the plan gives them no other.
        switch (s.kernel) {
            case GK_TILE128: rc = launch_gemm_tn<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi, s.row0); break;
            case GK_DEEP: rc = launch_gemm_tn256d<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi); break;
            case GK_MULTI_ANY: rc = launch_gemm_tn256dm<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi, s.tiles_per_wg); break;
#ifdef VQ_DIAG
            case GK_ASM256: rc = launch_gemm_tn256a<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi); break;
#endif
            default:
                if constexpr (!row_in) {
                    if (s.kernel == GK_RING160) { rc = launch_gemm_tn160_ring<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi); break; }
                    if (s.kernel == GK_PHASE4) { rc = launch_gemm_tn256<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi); break; }
                    if (s.kernel == GK_DEEP_GLOBAL_LDS) { rc = launch_gemm_tn256d<IS_F16, Epi, false>(st, A, lda, W, ldw, s.rows, N, K, epi); break; }
                }
                if constexpr (GEMM_EXPERIMENTS_BUILD) rc = launch_gemm_experiment<IS_F16>(st, A, lda, W, ldw, s.rows, N, K, epi, s.kernel);
                else rc = fail(VQ_ERR_STATE, "gemm plan names kernel %d, which this build does not carry", s.kernel);
        }
        if (rc) return rc;
    }
    return 0;
}

}  // namespace vq
