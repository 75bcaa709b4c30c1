// The measured-and-superseded batch scan mainloops: kept for A/B runs behind VQ_AMD_SCAN=2|4, compiled by
// `make EXPERIMENTS=1` only.  vq_index.hip includes this file in such a build and nowhere else; a product build reads nothing
// under experiments/ and its plan_scan (scan_plan.h) refuses both kinds.
#pragma once
#include "../scan_plan.h"
#include "knn_scan_phase4.h"
#include "knn_scan_deep.h"

namespace vq {

static_assert(SP_FOLD_LDS == SCAN4_LDS_BYTES, "plan_scan gives SCAN_DEEP the LDS bytes of SCAN_FOLD");

// the kernel of an experiment kind (its dynamic-LDS limit is the caller's to raise), null for any other kind
static inline const void* scan_experiment_kernel(int kind) {
    return kind == SCAN_PHASE4 ? (const void*)scan2_f16_top2_kernel : kind == SCAN_DEEP ? (const void*)scan4_f16_top2_kernel : nullptr;
}

// One chunk's scan with an experiment kind: both take 4 ranges x 8 query tiles per 32 workgroups (plan: rb = 2).
static inline void launch_scan_experiment(int kind, int grid, int lds, hipStream_t st, const uint16_t* q16, const uint16_t* x16, int dim, int64_t n,
                                          int q_tiles, int ranges, int range_groups, int64_t q_pad, uint32_t* keys) {
    hipLaunchKernelGGL(kind == SCAN_PHASE4 ? scan2_f16_top2_kernel : scan4_f16_top2_kernel, dim3(grid), dim3(G2_THREADS), (size_t)lds, st, q16, x16, dim,
                       n, q_tiles, ranges, range_groups, q_pad, keys);
}

}  // namespace vq
