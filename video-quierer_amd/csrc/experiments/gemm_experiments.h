// The measured-and-rejected GEMM mainloops: kept for A/B runs through vq_debug_gemm,
// vq_debug_gemm_ablate and $VQ_AMD_GEMM, compiled by `make EXPERIMENTS=1` only.  gemm_dispatch.h includes this file
// in such a build and nowhere else; a product build reads nothing under experiments/.
#pragma once
#include "gemm_mfma256_ring.h"
#include "gemm_mfma256p.h"
#include "gemm_mfma256w4.h"
#include "gemm_mfma256e.h"
#include "gemm_mfma256f.h"
#include "gemm_mfma128x256.h"
#include "gemm_mfma128x256p.h"

namespace vq {

static_assert(G12_BM == GX_BM && G12_BN == GX_BN && G12_SUB_K == GX_SUB_K && GP_BM == GX_BM && GP_BN == GX_BN && GP_SUB_K == GX_SUB_K,
              "plan_gemm tests the 128x256 experiments' shapes with GX_*");

// One step of a plan whose kernel is an experiment id.  plan_gemm has checked the shape where the id has a fallback;
// the others fail in their launcher's own checks.  Row-stat epilogues reach only the kernels with a row-stat prologue.
template <bool IS_F16, class Epi>
static int launch_gemm_experiment(hipStream_t st, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                                  int M, int N, int K, const Epi& epi, int kernel) {
    switch (kernel) {
        case GK_EXP_PHASE2: return launch_gemm_tn256e<IS_F16>(st, A, lda, W, ldw, M, N, K, epi);
        case GK_EXP_128X256: case GK_EXP_128X256_ANY: return launch_gemm_tn128x256<IS_F16>(st, A, lda, W, ldw, M, N, K, epi);
        case GK_EXP_128X256P_LAG: case GK_EXP_128X256P:
            return launch_gemm_tn128x256p<IS_F16>(st, A, lda, W, ldw, M, N, K, epi, kernel == GK_EXP_128X256P_LAG ? 1 : 0, gp_dephase_cycles(K));
    }
    if constexpr (!epi_row_in<Epi>::value) {
        switch (kernel) {
            case GK_EXP_RING256: return launch_gemm_tn256_ring<IS_F16>(st, A, lda, W, ldw, M, N, K, epi);
            case GK_EXP_PERSISTENT: return launch_gemm_tn256p<IS_F16>(st, A, lda, W, ldw, M, N, K, epi);
            case GK_EXP_WAVE4: return launch_gemm_tn256w4<IS_F16>(st, A, lda, W, ldw, M, N, K, epi);
            case GK_EXP_FUSED: return launch_gemm_tn256f<IS_F16>(st, A, lda, W, ldw, M, N, K, epi);
        }
    }
    return fail(VQ_ERR_STATE, "gemm plan names kernel %d, which is no experiment", kernel);
}

}  // namespace vq
