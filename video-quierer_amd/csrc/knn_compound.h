// Compound search (vq_index_search_compound, include/vq_amd.h): the k best rows under  D(r) = max over clauses of (min over the
// clause's terms of d(j, r)),  rows struck where a veto term has  d(v, r) < fp32(D(r) + margin).  Up to 16 terms, one virtual query.
//
//   plan_compound (host only)        path, key streams, candidate pool, the clause structure in scan lane order
//   compound_dist_kernel             exact path: fp64-chain distances of all terms -> table [m][ld], combined row D [n] (+inf where struck)
//   compound_finish_kernel           exact path: term_dist of the k winners from the table; a +inf slot (a struck row the selection
//                                    listed because fewer than k rows survive) becomes -1 / +inf
//   compound_terms_to_f16_kernel     fp16 path: the terms in lane order, rounded as queries_to_f16_kernel rounds queries
//   compound_scan_kernel<NKS>        pass 1: scan3_f16_top2_kernel's stream (knn_scan_small.h) with the term axis reduced per row
//   compound_rescore_kernel          pass 2: candidates re-scored exactly, the veto decided exactly, the proof, the call's flag
// The selection between them is the plain search's (select_small_kernel / select_chunk_kernel + merge_topk_kernel).
//
// Exact path.  compound_dist_kernel is exact_dist_kernel's tile (64 rows, the same index-order fp64 chain, the same
// 1.0f - (float)acc) with 16 term columns instead of 32 query columns, the combine fused behind it (the tile's distances meet in
// LDS, one thread per row applies the definition) and a gate: as the redo of an fp16 call it leaves at once unless the call's flag
// is set, so the launches queued never depend on the outcome.  The table is kept: term_dist reads the winners' columns from it.
//
// Pass 1.  scan3's accumulator layout is kept: lane (j = l & 15, g = l >> 4) holds the scores of term j for rows 4g .. 4g + 3 of a
// block, so the 16 terms of a row sit in the 16 lanes of one DPP row.  plan_compound places the terms so that every clause is a run
// of adjacent lanes (clauses in order, then the veto terms as one more run, then unused lanes, each a run of its own).  Per row:
//   a segmented inclusive max-scan over the DPP row (row_shr 1, 2, 4, 8; a lane takes its left neighbour at distance o only when
//   that lane is in its run) leaves every run's maximum in the run's last lane;  S16 = min over the clauses' last lanes and
//   V16 = the veto run's maximum are spread to all 16 lanes by two 4-step DPP butterflies (skipped without veto terms).
// The transposed form (MFMA operands swapped: 4 terms per lane in registers, the others at l ^ 16, l ^ 32, l ^ 48) needs clauses
// aligned to groups of 4 lanes to reduce in registers; five clauses of three terms do not fit 16 lanes that way, and its two
// cross-row steps are ds_bpermute round trips where a DPP step is one VALU instruction.  The segmented scan takes any clause
// structure: 12 + 2 + 8 (+ 8 with veto terms) VALU instructions per row value, about 150 per 16-row block beside the 16 MFMAs and
// 16 KiB of loads of the block; the pass has about 7,000 issue cycles per block and SIMD at HBM speed.  Resources:
// profiles/compound_search/kernel_resource_usage.txt (no spills, 2 workgroups per CU as scan3).
//   A row is masked (scan3's MASKED sentinel: "no row") when  V16 - S16 > veto_thr,  veto_thr = 2 E2 + CP_SLACK + 2^-21 |margin| -
//   margin  evaluated on the host in fp64 and rounded up, E2 = scan_eps_unit(dim) x max|row| x 2 (a term with |q| > 2 leaves the
//   call unproven anyway).  Then s(v) - S > CP_SLACK + 2^-21 |margin| - margin for the exact scores, which implies the strike
//   (below), so no possible survivor is dropped; every other row is decided exactly in pass 2.  The combined score is packed with
//   the 7-bit local row index and folded into the stream's top-2; key layout 3 with one query: [streams][2].
//
// Pass 2 and the proof.  One workgroup.  The C best keys (C = 32 for k <= 20, 64 for k <= 40, 80 for k <= 64, 128 for k <= 100:
// plan_scan's pools for one query) become candidates: T = the (C + 1)-th largest of the 256 thread maxima, so at least C + 1 keys
// reach T; the keys >= T are collected (more than CP_LIST of them: not proven) and ranked; `rest` = the largest key that is no
// candidate.  Every candidate gets its m fp64-chain dots, d(j) = 1.0f - dot(j), D and the strike exactly as the definition says.
//   Notation: s(j, r) the exact dot, S(r) = min over clauses of max over the clause's terms of s(j, r), Sf(r) the same over the
//   fp32-rounded dots.  Rounding and x -> 1.0f - x are monotone, so D(r) = fp32(1 - Sf(r)) and Sf(r) = fp32(S(r)).
//   E = scan_eps_unit(dim) x max|row| x max_j |q_j| bounds |s16(j, r) - s(j, r)| for every term and row, the packed index bits
//   included (knn_scan_f16.h); min and max are 1-Lipschitz in every argument, so |S16(r) - S(r)| <= E as well.
//   s_k = Sf of the k-th surviving candidate in (D, tie) order.  A row r that was not re-scored and is not masked has
//   S16(r) <= B for B = its stream's second key (rows a stream did not emit) or B = rest (keys that are no candidates).  The call
//   is proven when  B + E + CP_SLACK < s_k  (fp32) for rest and for every candidate that is a stream's second key, |q_j|^2 lies in
//   [0.25, 4] for every term, the list did not overflow and k candidates survive (or fewer, which can never be proven here: a veto
//   that leaves the pool short sends the call to the exact path).  Then S(r) <= B + E < s_k - CP_SLACK, and D(r) > D_k strictly:
//     |S| < 4 (|row|^2 <= 2, |q|^2 <= 4), so fp32(S(r)) <= S(r) + 2^-23; the two fp32 additions of the test err by at most 2^-23
//     each; and 1 - x for x in (-4, 4) has spacing at most 2^-22, so  Sf(r) <= s_k - 2^-21  guarantees  fp32(1 - Sf(r)) > fp32(1 -
//     s_k) = D_k.  Needed: 2^-23 + 2 x 2^-23 + 2^-21 = 7 x 2^-23 < CP_SLACK = 2^-20.  (LABEL_SLACK and SET_SLACK are 2^-19: they
//     cover a difference of two bounded scores; here one side, s_k, is exact.)
//   The strike in scores: d(v) < fp32(D + margin) holds whenever  s(v) - S + margin > 2^-21 + 2^-22 + 2^-24 (4 + |margin|): the two
//   roundings of each distance (2^-23 each, |.| < 4), the rounding of D + margin (2^-24 relative, |D| < 4).  Pass 1 adds three
//   fp32 operations on magnitudes below 4 + |margin| (3 x 2^-24 (4 + |margin|)); in all 7 x 2^-22 + 2^-22 |margin|, which the
//   scan's 2 x CP_SLACK = 2^-19 and 2^-21 |margin| cover.  margin = -inf gives veto_thr = +inf (nothing masked), +inf gives -inf
//   (every row masked: V16 - S16 is finite), NaN is refused.
// Stream rescans are kept, in another order than the plain re-score's: while a second-key candidate's key could reach the k-th
// score SO FAR, the stream of the largest such key is scored in full (128 rows x m chains), its candidates leave the pool and the
// k-th score s_k is taken again over the larger pool; up to CP_RESCAN_MAX streams, then the bounds are tested against the last
// s_k.  s_k only rises when rows join the pool, so a candidate passed over because its key lay below an earlier s_k lies below
// the later one too.  Consecutive frames of a video share a stream, so the best k rows of a query aimed at one moment sit in one
// or two streams that emit two keys each: tested against the candidates' own k-th score (far down among unrelated rows) no such
// call was ever proven (the first probe run: 0 of 10 calls on 1M video-like rows); rescanning every stream open against that
// first score took four streams every time where one or two settle the call.  A second key outside the rescanned streams that
// could still matter leaves the call unproven.
// An unproven call is redone by the exact path on the device, gated by the flag the re-score wrote; nothing is read back.
#pragma once
#include "vq_common.h"
#include "gemm_mfma.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"

namespace vq {

constexpr int CP_MAX_M = 16;                        // terms per call: the B operand's 16 columns
constexpr int CP_MAX_C = 128;                       // largest candidate pool
constexpr int CP_LIST = 512;                        // collected keys the re-score ranks (4 x the largest pool, as the plain re-score)
constexpr int CP_RESCAN_MAX = 4;                    // streams re-scored in full per call (RV_RESCAN_MAX)
constexpr int CP_POOL = CP_MAX_C + CP_RESCAN_MAX * 128;      // rows scored exactly at the most
constexpr float CP_SLACK = 1.0f / 1048576;          // 2^-20 (derivation above)
constexpr int CP_K_MAX = 100;                       // fp16 path: the plain search's limit (RV_K_MAX)
// mode 0 takes the fp16 path from this many rows.  Not the plain search's 16,384: the one-workgroup re-score with its stream
// rescans costs 0.1 ms (one rescan) to 0.5 ms (four) where the exact path takes 0.09 ms at 16,384 rows and 0.43 ms at 262,144.
// Measured (scripts/compound_search_probe.py, m = 3, k = 20): a query aimed at one moment of a video crosses between 32,768 and
// 65,536 rows, one unrelated to the rows held between 262,144 and 524,288; at 262,144 rows the fp16 path is 2.7x ahead on the
// first and 0.09 ms behind on the second (profiles/compound_search/probe.txt).
constexpr int64_t CP_FP16_MIN_ROWS = 262144;
static_assert(CP_K_MAX == RV_K_MAX, "the compound fp16 path follows the plain search's k limit");

struct CompoundSpec {                               // the definition's clause structure, by term
    int8_t clause[CP_MAX_M];                        // clause number, -1: veto term
    int m, clauses;
};
struct CompoundLanes {                              // ... and by scan lane (bit j = lane j of a DPP row)
    uint32_t seg_start;                             // first lane of a run
    uint32_t clause_tail;                           // last lane of a clause
    uint32_t veto_tail;                             // last lane of the veto run (no bit: no veto terms)
    int8_t term[CP_MAX_M];                          // the term a lane holds, -1: none (zero column)
};

struct CompoundPlan {
    bool fp16 = false;
    int64_t streams = 0;                            // 128-row streams = key pairs of the one virtual query
    int pool = 0;                                   // candidates re-scored exactly (0 on the exact path)
    int64_t ld = 0, exact_bytes = 0;                // exact path / redo: the term table [m][ld] fp32
    float eps = 0.f;                                // unit rows and terms: a k-th and (k+1)-th exact D more than 4 eps apart are proven
    CompoundSpec spec;
    CompoundLanes lanes;
};

static inline int compound_pool(int k) { return k <= 20 ? 32 : k <= 40 ? 64 : k <= 64 ? 80 : CP_MAX_C; }

// clause_of is well-formed (check_compound_args) or null (vq_debug_compound_plan: m terms of one-term clauses)
static inline CompoundPlan plan_compound(int64_t n, int dim, int m, const int32_t* clause_of, int k, int mode, bool near_unit) {
    CompoundPlan p;
    const bool ok = scan_fp16_dim(dim) && near_unit && k <= CP_K_MAX && n >= 1;
    p.fp16 = mode == 2 ? ok : mode == 0 && ok && n >= CP_FP16_MIN_ROWS;
    p.streams = (n + 127) / 128;
    p.pool = p.fp16 ? compound_pool(k) : 0;
    p.ld = (n + 63) / 64 * 64;
    p.exact_bytes = (int64_t)m * p.ld * 4;
    p.eps = scan_fp16_dim(dim) ? scan_eps_unit(dim) * 1.0001f * 1.0001f + 0.5f * CP_SLACK : 0.f;
    p.spec.m = m; p.spec.clauses = 0;
    for (int j = 0; j < CP_MAX_M; ++j) {
        p.spec.clause[j] = j < m ? (int8_t)(clause_of ? clause_of[j] : j) : (int8_t)-1;
        if (j < m && p.spec.clause[j] >= p.spec.clauses) p.spec.clauses = p.spec.clause[j] + 1;
    }
    // lane order: the clauses' terms (their numbers do not decrease over the non-veto terms), then the veto terms, then nothing
    CompoundLanes& L = p.lanes;
    L.seg_start = L.clause_tail = L.veto_tail = 0;
    int lane = 0, prev = -2;
    for (int j = 0; j < m; ++j) {
        const int c = p.spec.clause[j];
        if (c < 0) continue;
        if (c != prev) { L.seg_start |= 1u << lane; if (lane > 0 && prev >= 0) L.clause_tail |= 1u << (lane - 1); }
        L.term[lane++] = (int8_t)j; prev = c;
    }
    if (lane > 0) L.clause_tail |= 1u << (lane - 1);
    const int first_veto = lane;
    for (int j = 0; j < m; ++j)
        if (p.spec.clause[j] < 0) L.term[lane++] = (int8_t)j;
    if (lane > first_veto) { L.seg_start |= 1u << first_veto; L.veto_tail = 1u << (lane - 1); }
    for (; lane < CP_MAX_M; ++lane) { L.seg_start |= 1u << lane; L.term[lane] = -1; }
    return p;
}

// the scan's veto threshold (header): fp64 on the host, rounded up to fp32
static inline float compound_veto_thr(float eps_rows, float margin) {
    if (margin == __builtin_inff()) return -__builtin_inff();
    if (margin == -__builtin_inff()) return __builtin_inff();
    const double t = 2.0 * (2.0 * (double)eps_rows) + 2.0 * (double)CP_SLACK + __builtin_fabs((double)margin) / 2097152.0 - (double)margin;
    float f = (float)t;
    if ((double)f < t) f = __builtin_nextafterf(f, __builtin_inff());
    return f;
}

// ---- the definition on one row's term distances (fp32 compares and one fp32 addition); dot: the fp32-rounded dots ----
// returns D; *struck: a veto term strikes the row; *sf: the combined fp32 score (D = 1.0f - sf)
__device__ __forceinline__ float compound_combine(const float* dot /*[m], stride `ds`*/, int ds, const CompoundSpec& sp, float margin,
                                                  bool* struck, float* sf) {
    const float INF = __builtin_inff();
    float D = -INF, S = INF, cur = INF, curs = -INF;
    int prev = -1;
    for (int j = 0; j < sp.m; ++j) {
        const int c = sp.clause[j];
        if (c < 0) continue;
        const float s = dot[j * ds], d = 1.0f - s;
        if (c != prev && prev >= 0) { D = fmaxf(D, cur); S = fminf(S, curs); cur = INF; curs = -INF; }
        cur = fminf(cur, d); curs = fmaxf(curs, s); prev = c;
    }
    D = fmaxf(D, cur); S = fminf(S, curs);
    const float lim = D + margin;
    bool st = false;
    for (int j = 0; j < sp.m; ++j)
        if (sp.clause[j] < 0 && 1.0f - dot[j * ds] < lim) st = true;
    *struck = st; *sf = S;
    return D;
}

// ---- exact path: term distances of a 64-row tile (exact_dist_kernel's chain), combined ----
// gate: null (the call's answer) or the call's flag (the redo runs only when it is set)
__global__ __launch_bounds__(256)
void compound_dist_kernel(const float* __restrict__ rows, int64_t n, int dim, const float* __restrict__ terms, const CompoundSpec sp,
                          float margin, float* __restrict__ table /*[m][ld]*/, int64_t ld, float* __restrict__ D_out /*[n]*/,
                          const unsigned long long* __restrict__ gate) {
    if (gate && *gate == 0) return;
    __shared__ float xs[64][65];
    __shared__ double qs[CP_MAX_M][64];
    __shared__ float dots[CP_MAX_M][64];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    const int m = sp.m;
    double acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 0.0;
    for (int d0 = 0; d0 < dim; d0 += 64) {
        for (int i = tid; i < 64 * 64; i += 256) {
            const int rr = i >> 6, cc = i & 63;
            const int64_t gr = row0 + rr;
            xs[rr][cc] = (gr < n && d0 + cc < dim) ? rows[gr * dim + d0 + cc] : 0.f;
        }
        for (int i = tid; i < CP_MAX_M * 64; i += 256) {
            const int qq = i >> 6, cc = i & 63;
            qs[qq][cc] = (qq < m && d0 + cc < dim) ? (double)terms[(int64_t)qq * dim + d0 + cc] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int c = 0; c < 64; ++c) {
            const double xv = (double)xs[r][c];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += xv * qs[g * 4 + j][c];   // product exact in fp64
        }
        __syncthreads();
    }
    const int64_t gr = row0 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = g * 4 + j;
        const float s = (float)acc[j];
        dots[q][r] = s;
        if (gr < n && q < m) table[(int64_t)q * ld + gr] = 1.0f - s;
    }
    __syncthreads();
    if (tid < 64 && gr < n) {
        bool struck; float sf;
        const float D = compound_combine(&dots[0][tid], 64, sp, margin, &struck, &sf);
        D_out[gr] = struck ? __builtin_inff() : D;
    }
}

// ---- exact path: the winners' term distances; struck rows the selection listed (D = +inf) leave ----
__global__ __launch_bounds__(256)
void compound_finish_kernel(int32_t* __restrict__ ids, float* __restrict__ dist, int k, const float* __restrict__ table, int64_t ld, int m,
                            float* __restrict__ term_dist /*[k][m] or null*/, const unsigned long long* __restrict__ gate) {
    if (gate && *gate == 0) return;
    for (int t = threadIdx.x; t < k; t += 256) {
        int id = ids[t];
        if (id >= 0 && !(dist[t] < __builtin_inff())) { id = -1; ids[t] = -1; }
        if (term_dist)
            for (int j = 0; j < m; ++j) term_dist[(size_t)t * m + j] = id >= 0 ? table[(int64_t)j * ld + id] : __builtin_inff();
    }
}

// ---- fp16 path: terms [m][dim] fp32 -> q16 [16][dim] in lane order (zero rows for lanes without a term) ----
__global__ __launch_bounds__(256)
void compound_terms_to_f16_kernel(const float* __restrict__ terms, const CompoundLanes lanes, int dim, uint16_t* __restrict__ q16) {
    const int lane = blockIdx.x, t = lanes.term[lane];
    for (int i = threadIdx.x * 4; i < dim; i += 1024) {
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0) v = *(const float4*)(terms + (size_t)t * dim + i);
        typedef __attribute__((ext_vector_type(4))) _Float16 h4;
        const h4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        *(uint2*)(q16 + (size_t)lane * dim + i) = __builtin_bit_cast(uint2, h);
    }
}

// DPP helpers over a row of 16 lanes.  shr: lane j reads lane j - O (lanes j < O keep their own value)
template <int O>
__device__ __forceinline__ float row_shr(float x) {
    const int xi = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, 0x110 + O, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_min(float x) {
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true)));
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true)));
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true)));
    x = fminf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true)));
    return x;
}
__device__ __forceinline__ float row16_max(float x) {
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true)));
    x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true)));
    return x;
}

// ---- pass 1: scan3_f16_top2_kernel<NKS, 1>'s stream with the term axis reduced per row (header) ----
template <int NKS>                                   // dim / 32
__global__ __launch_bounds__(256, 2)
void compound_scan_kernel(const uint16_t* __restrict__ Q16 /*[16][dim], lane order*/, const uint16_t* __restrict__ X16, int64_t n_valid,
                          int64_t streams, const CompoundLanes lanes, float veto_thr, uint32_t* __restrict__ keys /*[streams][2]*/) {
    typedef mfma_op<true> op;
    typedef op::frag frag;
    constexpr int DIM = NKS * 32;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stream = (int64_t)blockIdx.x * 4 + wave;
    if (stream >= streams) return;                         // wave-uniform; no barriers below
    const int r16 = lane & 15, g = lane >> 4;

    frag qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const frag*)(Q16 + (size_t)r16 * DIM + ks * 32 + g * 8);

    // this lane's run starts at the highest set bit of seg_start at or below it (bit 0 is always set)
    const int start = 31 - __builtin_clz(lanes.seg_start & ((2u << r16) - 1u));
    const bool take1 = r16 - 1 >= start, take2 = r16 - 2 >= start, take4 = r16 - 4 >= start, take8 = r16 - 8 >= start;
    const bool ctail = (lanes.clause_tail >> r16) & 1u, vtail = (lanes.veto_tail >> r16) & 1u;
    const bool has_veto = lanes.veto_tail != 0;            // uniform

    const float NEG = -__builtin_inff(), MASKED = -3.0e38f;   // finite sentinel: see scan_f16_top2_kernel
    const uint16_t* xrow = X16 + ((size_t)stream * 128 + r16) * DIM + g * 8;
    frag xf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) xf[ks] = *(const frag*)(xrow + ks * 32);

    float m1 = NEG, m2 = NEG;
    const bool ragged = (stream + 1) * 128 > n_valid;      // wave-uniform
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            acc = op::run(xf[ks], qf[ks], acc);
            if (rb + 1 < 8) {                                                                            // refill in rotation
                xf[ks] = *(const frag*)(xrow + (size_t)(rb + 1) * 16 * DIM + ks * 32);
                __builtin_amdgcn_sched_barrier(0);      // or the scheduler sinks the load to its use (one register, vmcnt(0) per MFMA)
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[r];
            float t;
            t = row_shr<1>(v); v = take1 ? fmaxf(v, t) : v;
            t = row_shr<2>(v); v = take2 ? fmaxf(v, t) : v;
            t = row_shr<4>(v); v = take4 ? fmaxf(v, t) : v;
            t = row_shr<8>(v); v = take8 ? fmaxf(v, t) : v;
            float s = row16_min(ctail ? v : __builtin_inff());
            if (has_veto) {
                const float vs = row16_max(vtail ? v : NEG);
                if (vs - s > veto_thr) s = MASKED;
            }
            const int local = rb * 16 + 4 * g + r;
            if (ragged && stream * 128 + local >= n_valid) s = MASKED;
            const float kf = __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, s) & ~127u) | (uint32_t)local);
            m2 = __builtin_amdgcn_fmed3f(m1, m2, kf);
            m1 = fmaxf(m1, kf);
        }
        __builtin_amdgcn_sched_barrier(0);      // the fold stays with its block
    }
    // merge the four row groups (lanes l, l^16, l^32, l^48): top-2 of two sorted pairs
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float b1 = __shfl_xor(m1, o), b2 = __shfl_xor(m2, o);
        const float lo = fminf(m1, b1);
        m1 = fmaxf(m1, b1);
        m2 = fmaxf(lo, fmaxf(m2, b2));
    }
    if (lane == 0) *(uint2*)(keys + (size_t)stream * 2) = uint2{__builtin_bit_cast(uint32_t, m1), __builtin_bit_cast(uint32_t, m2)};
}

// exact_dot_chain_pf's chain (knn_scan_f16.h: index order, fp64, one rounding at the end) with sixteen 16-byte loads of the row in
// flight instead of eight: the one workgroup of pass 2 waits a memory round trip per batch and has registers to spare.  dim % 64 == 0.
__device__ __forceinline__ float compound_dot_chain(const float* __restrict__ row, const float* __restrict__ q, int dim) {
    double acc = 0.0;
    for (int i = 0; i < dim; i += 64) {
        float4 a[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) a[u] = *(const float4*)(row + i + 4 * u);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float4 b = *(const float4*)(q + i + 4 * u);
            acc += (double)a[u].x * (double)b.x;
            acc += (double)a[u].y * (double)b.y;
            acc += (double)a[u].z * (double)b.z;
            acc += (double)a[u].w * (double)b.w;
        }
    }
    return (float)acc;
}

// ---- pass 2: candidates, exact compound scores, the veto, the proof (header).  One workgroup. ----
// gc: {proven, rows re-scored, redo}: gc[2] is the call's flag, the gate of the exact kernels behind this one
__global__ __launch_bounds__(256)
void compound_rescore_kernel(const uint32_t* __restrict__ keys, int64_t streams, const float* __restrict__ rows, int64_t n_valid, int dim,
                             const float* __restrict__ terms, const CompoundSpec sp, float margin, int k, int C, float eps_rows,
                             int32_t* __restrict__ out_ids, float* __restrict__ out_dist, float* __restrict__ term_dist /*[k][m] or null*/,
                             unsigned long long* __restrict__ gc, const TieOrder tie) {
    __shared__ float tmax[256];
    __shared__ __attribute__((aligned(8))) int2 sel[CP_LIST];          // {key bits, source = stream * 2 + which}
    __shared__ float cand_key[CP_MAX_C];
    __shared__ int cand_src[CP_MAX_C];
    __shared__ int pool_row[CP_POOL];                                  // slots [0, C): the candidates in key order; behind them the rescanned streams' rows
    __shared__ float pool_dot[CP_POOL][CP_MAX_M];
    __shared__ uint64_t pool_key[CP_POOL];                             // dist_key(D, tie) of a surviving row: unique, ranked by counting
    __shared__ float pool_S[CP_POOL];
    __shared__ float red[4], q2_s[CP_MAX_M];
    __shared__ float thr_s, rest_s, sk_s;
    __shared__ int sel_n, have_s, open_s, scored_s, resc_n;
    __shared__ int resc_stream[CP_RESCAN_MAX];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float NEG = -__builtin_inff(), REAL = -2.0e38f;              // keys at or below REAL say "no row" (MASKED, or a missing stream)
    const int m = sp.m;

    // 1. thread maxima; T = the (C + 1)-th largest of them
    float mx = NEG;
    for (int64_t s = tid; s < streams; s += 256) mx = fmaxf(mx, __builtin_bit_cast(float, keys[s * 2]));      // a stream's 2nd key is never above its 1st
    tmax[tid] = mx;
    if (tid < CP_MAX_C) { cand_key[tid] = NEG; cand_src[tid] = -1; pool_row[tid] = -1; }
    if (tid == 0) { sel_n = 0; thr_s = NEG; rest_s = NEG; open_s = 0; scored_s = 0; resc_n = 0; }
    __syncthreads();
    {
        int rank = 0;
        for (int j = 0; j < 256; ++j) { const float o = tmax[j]; rank += (o > mx) || (o == mx && j < tid); }
        if (rank == C) thr_s = mx;                                      // ranks are a permutation: one writer (C <= 128 < 256)
    }
    // |q_j|^2 of every term: one wave per term in turn
    for (int j = wave; j < m; j += 4) {
        float s2 = 0.f;
        for (int i = lane; i < dim; i += 64) { const float v = terms[(size_t)j * dim + i]; s2 += v * v; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
        if (lane == 0) q2_s[j] = s2;
    }
    __syncthreads();
    // 2. collect the keys >= T; the largest key left behind
    {
        const float thr = fmaxf(thr_s, REAL);
        float below = NEG;
        for (int64_t s = tid; s < streams; s += 256) {
            const uint2 two = *(const uint2*)(keys + s * 2);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const uint32_t kb = w ? two.y : two.x;
                const float v = __builtin_bit_cast(float, kb);
                if (v >= thr && v > REAL) {
                    const int pos = atomicAdd(&sel_n, 1);
                    if (pos < CP_LIST) sel[pos] = int2{(int)kb, (int)(s * 2) + w};
                } else {
                    below = fmaxf(below, v);
                }
            }
        }
        below = wave64_max(below);
        if (lane == 0) red[wave] = below;
    }
    __syncthreads();
    const int ns = min(sel_n, CP_LIST);
    for (int i = tid; i < ns; i += 256) {
        const float vi = __builtin_bit_cast(float, sel[i].x); const int si = sel[i].y;
        int rank = 0;
        for (int j = 0; j < ns; ++j) {
            const int2 e = sel[j];
            const float vj = __builtin_bit_cast(float, e.x);
            rank += (vj > vi) || (vj == vi && e.y < si);                // sources are distinct: ranks are a permutation
        }
        if (rank < C) {
            cand_key[rank] = vi; cand_src[rank] = si;
            const int64_t r = scan3_row_of(si >> 1, (int)(__builtin_bit_cast(uint32_t, vi) & 127u));
            pool_row[rank] = r < n_valid ? (int)r : -1;
        }
        if (rank == C) rest_s = vi;
    }
    __syncthreads();
    // 3. exact scoring of pool slots [lo, hi): the m fp64-chain dots, thread = (slot, term) pairs; then the definition per slot.
    //    pool_row: >= 0 a surviving row, -1 none, <= -2 a struck row
    auto score = [&](int lo, int hi) __attribute__((always_inline)) {
        for (int p = lo * m + tid; p < hi * m; p += 256) {
            const int c = p / m, j = p - c * m;
            const int r = pool_row[c];
            if (r >= 0) pool_dot[c][j] = compound_dot_chain(rows + (size_t)r * dim, terms + (size_t)j * dim, dim);
        }
        __syncthreads();
        for (int c = lo + tid; c < hi; c += 256) {
            const int r = pool_row[c];
            if (r < 0) continue;
            bool struck; float sf;
            const float D = compound_combine(&pool_dot[c][0], 1, sp, margin, &struck, &sf);
            pool_S[c] = sf;
            if (struck) pool_row[c] = -(r + 2); else pool_key[c] = dist_key(D, tie_of(tie, r));
            atomicAdd(&scored_s, 1);
        }
        __syncthreads();
    };
    // the survivors of slots [0, hi) ranked by (D, tie); sk_s = the combined score of the k-th, have_s = their number
    int my_rank[CP_POOL / 256 + 1];
    auto rank_pool = [&](int hi) __attribute__((always_inline)) {
        if (tid == 0) { sk_s = NEG; have_s = 0; }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < CP_POOL / 256 + 1; ++u) {
            const int c = tid + 256 * u;
            my_rank[u] = -1;
            if (c >= hi || pool_row[c] < 0) continue;
            const uint64_t mine = pool_key[c];
            int rank = 0;
            for (int j = 0; j < hi; ++j) rank += pool_row[j] >= 0 && pool_key[j] < mine;
            my_rank[u] = rank;
            if (rank == k - 1) sk_s = pool_S[c];                        // rows are distinct: one writer
            atomicAdd(&have_s, 1);
        }
        __syncthreads();
    };
    score(0, C);
    rank_pool(C);

    // 4. stream rescans.  A candidate that is its stream's SECOND key bounds the rows the stream did not emit; where that bound
    //    could still reach the k-th score so far, the stream's 128 rows are scored exactly instead (up to CP_RESCAN_MAX streams, by
    //    key), its candidates leave the pool, and the k-th score is taken again over the larger pool: it can only rise, so a
    //    bound that held before holds after.  Consecutive frames of a video share a stream: without this no query aimed at one
    //    moment of a video is ever proven (the best k rows sit in one or two streams, which emit two keys each).
    float q2max = 0.f; bool q_ok = true;
    for (int j = 0; j < m; ++j) { const float q2 = q2_s[j]; q2max = fmaxf(q2max, q2); q_ok = q_ok && q2 >= SCAN_Q2_MIN && q2 <= SCAN_Q2_MAX; }
    const float E = eps_rows * sqrtf(q2max) + CP_SLACK;                // NaN for a term that is not finite: every test fails
    const bool listed = sel_n <= CP_LIST;
    // one stream at a time, the open second key with the largest key first: after the stream that holds the best rows has joined
    // the pool the k-th score has usually risen past every other second key (the first form of this step rescanned every stream
    // open against the candidates' own k-th score: always four, 512 rows x m chains and a pool of 640 to rank)
    int pn = C;
    for (int it = 0; it < CP_RESCAN_MAX; ++it) {
        if (tid == 0) {
            int pick = -1;
            const float sk0 = sk_s;
            if (q_ok && listed)
                for (int c = 0; c < C && pick < 0; ++c) {                // candidates are in key order
                    if (cand_src[c] < 0 || !(cand_src[c] & 1) || cand_key[c] + E < sk0) continue;
                    bool done = false;
                    for (int w = 0; w < it; ++w) done = done || resc_stream[w] == (cand_src[c] >> 1);
                    if (!done) pick = cand_src[c] >> 1;                  // (a stream has one second key)
                }
            resc_stream[it] = pick;
            resc_n = pick >= 0 ? it + 1 : it;
        }
        __syncthreads();
        if (resc_n == it) break;                                         // block-uniform
        const int st = resc_stream[it];
        if (tid < C && cand_src[tid] >= 0 && (cand_src[tid] >> 1) == st) pool_row[tid] = -1;       // its stream's rows are all in the pool now
        if (tid < 128) {
            const int64_t r = scan3_row_of(st, tid);
            pool_row[pn + tid] = r < n_valid ? (int)r : -1;
        }
        __syncthreads();
        score(pn, pn + 128);
        pn += 128;
        rank_pool(pn);
    }
    const int nres = resc_n;

    // 5. the verdict: every key that stands for rows not scored exactly must lie below the k-th score
    const float sk = sk_s;
    const float rest = fmaxf(fmaxf(rest_s, fmaxf(red[0], red[1])), fmaxf(red[2], red[3]));
    if (tid < C && cand_src[tid] >= 0 && (cand_src[tid] & 1) && !(cand_key[tid] + E < sk)) {
        bool rescanned = false;
        for (int w = 0; w < nres; ++w) rescanned = rescanned || (cand_src[tid] >> 1) == resc_stream[w];
        if (!rescanned) atomicAdd(&open_s, 1);                          // a second key hides its stream's other rows
    }
    __syncthreads();
    const int have = have_s;
    const bool proven = q_ok && listed && have >= k && rest + E < sk && open_s == 0;
    for (int t = tid; t < k; t += 256)
        if (t >= have) {
            out_ids[t] = -1; out_dist[t] = __builtin_inff();
            if (term_dist) for (int j = 0; j < m; ++j) term_dist[(size_t)t * m + j] = __builtin_inff();
        }
#pragma unroll
    for (int u = 0; u < CP_POOL / 256 + 1; ++u) {
        const int c = tid + 256 * u, t = my_rank[u];
        if (t < 0 || t >= k) continue;
        out_ids[t] = pool_row[c]; out_dist[t] = key_dist(pool_key[c]);
        if (term_dist) for (int j = 0; j < m; ++j) term_dist[(size_t)t * m + j] = 1.0f - pool_dot[c][j];
    }
    if (tid == 0) { gc[0] = proven ? 1 : 0; gc[1] = (unsigned long long)scored_s; gc[2] = proven ? 0 : 1; }
}

}  // namespace vq
