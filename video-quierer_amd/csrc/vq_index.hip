// vq_index: exact cosine k-NN over a device-resident embedding matrix.
// Replaces HNSWIndex.add / add_batch / search / search_batch / size and backs
// save / load (reference src/indexes/hnsw.py:150-380, 488-528) — SURVEY.md §8a K-rows.
#include "../../include/vq_amd.h"
#include "vq_common.h"
#include "knn_kernels.h"
#include "knn_scan_f16.h"
#include "knn_fallback.h"
#include "knn_scan_fold.h"
#include "knn_grouped.h"
#include "knn_remove.h"
#include "knn_filter.h"
#include "knn_set.h"
#include "knn_distinct.h"
#include "knn_diverse.h"
#include "knn_sequence.h"
#include "knn_span.h"
#include "knn_align.h"
#include "knn_summary.h"
#include "knn_segment.h"
#include "knn_label.h"
#include "knn_compound.h"
#include "knn_cluster.h"
#include "knn_match.h"
#include "knn_neighbors.h"
#include "scan_plan.h"
#include "host_buffers.h"
#ifdef VQ_SCAN_EXPERIMENTS      // `make EXPERIMENTS=1`: the two superseded batch mainloops behind VQ_AMD_SCAN=2|4
#include "experiments/scan_experiments.h"
#endif

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>
#include <vector>

namespace vq {
int require_init();
enum IdxClass { I_NORMALIZE = 0, I_TO_F16, I_EXACT_DIST, I_SELECT, I_MFMA_SCAN, I_RESCORE, I_SEQ_DP };
static const char* kIdxClassNames[VQ_IDX_NCLASS] = {
    "normalize_rows", "rows_to_f16", "exact_dist_f64chain", "select_topk", "scan_f16_mfma_top2", "rescore_verify", "sequence_dp"};
#ifdef VQ_DIAG
constexpr bool SCAN_DIAG_BUILD = true;
#else
constexpr bool SCAN_DIAG_BUILD = false;
#endif
#ifdef VQ_SCAN_EXPERIMENTS
constexpr bool SCAN_EXPERIMENTS_BUILD = true;
#else
constexpr bool SCAN_EXPERIMENTS_BUILD = false;
#endif
// plan_scan (scan_plan.h, no HIP in it) computes with the kernels' geometry
static_assert(SP_STREAM_ROWS == SCAN_STREAM_ROWS && SP_TILE128_QT == SCAN_QT && SP_TILE128_RANGE == SCAN_RANGE && SP_BATCH_QT == SCAN2_QT &&
              SP_BATCH_RANGE == SCAN2_RANGE && SP_STREAM_QB == SCAN3_QB && SP_STREAM_FUSED_MAX_Q == SCAN3_FUSED_MAX_Q && SP_STREAM_MAX_Q == SCAN3_MAX_Q,
              "scan_plan.h: scan geometry");
static_assert(DST_FP16_MAX_K == RV_K_MAX && DST_MAX_DEPTH == 1024, "knn_distinct.h: the producers' k limits");
static_assert(SP_PHASE4_LDS == G2_LDS_BYTES && SP_FOLD_LDS == SCAN5_LDS_BYTES, "scan_plan.h: scan LDS bytes");
static_assert(SP_K_SMALL == RV_K_SMALL && SP_K_SMALL64 == RV_K_SMALL64 && SP_K_MID == RV_K_MID && SP_BATCH8_QPW == RV_QPW && SP_LARGE_QPW == RVL_QPW &&
              SP_LARGE_QPW == RVX_QPW && SP_SMALL32_C == RV_C && SP_SMALL64_C == 64, "scan_plan.h: re-score geometry");
}  // namespace vq

using namespace vq;

namespace {

// the index's device buffers: DevBuf under the index's out-of-memory message
template <class T> struct IdxBuf : DevBuf<T> { IdxBuf() : DevBuf<T>("index: scratch ") {} };

// One slot of the filtered search's staging ring: pinned memory and the event of the copy that last read it.
struct StageSlot {
    PinnedBuf<int32_t> h;
    hipEvent_t ev = nullptr;
    ~StageSlot() { if (ev) (void)hipEventDestroy(ev); }
};

// Where the last search's statistics are (vq_index_last_search_stats).
enum StatsAt {
    STATS_HOST,        // in vq_index::stats
    STATS_COUNTERS,    // on their way to h_counters behind the search
    STATS_GCOUNTERS,   // on their way to h_gcounters behind the search
    STATS_DEFERRED,    // a host-synchronous fp16 search: its kernels write h_counters; the caller (vq_index_search) reads them after its
                       // one wait and launches the fallback itself when a query was flagged
};

}  // namespace

struct vq_index {
    int dim = 0;
    int64_t size = 0, cap = 0;     // rows held / allocated
    IdxBuf<float> rows;            // fp32 master [cap][dim] (normalised rows, what the reference keeps in .data); `cap` above counts its rows
    IdxBuf<uint16_t> rows16;       // fp16 scan copy [cap][dim]
    hipStream_t stream = nullptr, own_stream = nullptr;
    std::mutex mu;
    std::vector<std::pair<const void*, size_t>> dyn_lds;    // kernels whose dynamic-LDS limit this handle has raised (set_dyn_lds)
    // scratch
    IdxBuf<float> d_q;             // queries [nq][dim]
    IdxBuf<float> d_dist;          // exact distances
    IdxBuf<uint64_t> d_partial;    // per-chunk top-k keys
    IdxBuf<char> d_res;            // a host form's results until they are copied back, laid out by outs_place: one call at a time
                                   // holds the lock and ends with a stream wait, so one block serves every family
    IdxBuf<float> d_upd;           // vq_index_update_rows: staged rows [n][dim] + their row numbers behind them;
                                   // vq_index_remove_rows: one chunk of moved rows
    IdxBuf<int32_t> d_rmw;         // vq_index_remove_rows: row maps, prefix sums, rebuilt ranks / labels (words)
    // (distance, id) tie order (vq_index_set_id_ranks): rank of each row's id in the caller's id order + the inverse behind it in one
    // allocation; rank_n = the number of rows they cover (0 = none set: ties come back in row order).  A search with
    // rank_n != size is refused.
    IdxBuf<int32_t> d_rank; int32_t* d_rank_inv = nullptr; int64_t rank_n = 0;      // d_rank.cap = 2 x the rows it holds (rank | inverse)
    TieOrder tie() const { return rank_n ? TieOrder{d_rank, d_rank_inv} : TieOrder{nullptr, nullptr}; }
    // group labels (vq_index_set_groups), one allocation: label per row, padded with -1 to whole 128-row streams; the by-group CSR
    // row list (goff [n_groups + 1], grows [n]); per stream the label its 128 rows share, or -1.  group_n = the rows they cover
    // (0 = none set); a grouped search with group_n != size is refused.
    IdxBuf<int32_t> d_group; int32_t* d_goff = nullptr; int32_t* d_grows = nullptr; int32_t* d_sgroup = nullptr;
    int64_t group_n = 0; int32_t n_groups = 0;
    std::vector<int32_t> h_goff;    // host mirror of goff (kept by set_groups / remove_rows): a filtered search sizes itself from it
    // filtered-search scratch (knn_filter.h): allowed groups, their row offsets, the row list and its tie words or the allowed
    // groups' bitmap; the filter list goes up from a ring of pinned staging slots, each reused once its event (the copy) is done
    IdxBuf<int32_t> d_flt;
    static constexpr int FLT_STAGE_SLOTS = 4;
    StageSlot flt_stage[FLT_STAGE_SLOTS]; int flt_slot = 0;
    IdxBuf<int32_t> d_fcand;       // masked fp16 path: candidate streams [nq][FLT_CAND] | n [nq] | listed [nq] | thr [nq]
    IdxBuf<uint64_t> d_flist;      // ... re-scored keys [nq][FLT_LIST]
    // grouped-search scratch (knn_grouped.h) and its outcome counters (pinned copy read by last_search_stats)
    IdxBuf<uint32_t> d_gbest;
    IdxBuf<int32_t> d_gcand;       // cand [qc][CAND] | pref [qc][CAND + 1] | n [qc] | flags [qc] | thr [qc]
    IdxBuf<uint64_t> d_gkeys;      // best [qc][CAND] (fp16 path), per-block lists (exact path / redo)
    IdxBuf<uint64_t> d_gpart;
    IdxBuf<unsigned long long> d_gcounters; PinnedBuf<unsigned long long> h_gcounters;
    // positions (vq_index_set_positions): one int32 per row; pos_n = the rows they cover (0 = none set).  A distinct search with
    // pos_n != size is refused.  Distinct-search scratch (knn_distinct.h): the plain search's answer at the plan's depth
    // (ids | distances), the filed queries' slot list, the redo's selection (ids | distances); its counters are d_gcounters
    IdxBuf<int32_t> d_pos; int64_t pos_n = 0;
    IdxBuf<int32_t> d_dpre;
    IdxBuf<int32_t> d_dslots;
    IdxBuf<int32_t> d_dsel;
    // diverse search (knn_diverse.h): the prefix's pair bit matrix [nq][D][ceil(D / 64)]; the redo's chunk minima [slots][chunks];
    // its picked rows [slots].  The prefix, the slot list and the counters are the distinct search's (d_dpre, d_dslots, d_gcounters)
    IdxBuf<uint64_t> d_vbits;
    IdxBuf<uint64_t> d_vpart;
    IdxBuf<int32_t> d_vpick;
    // sequence search (knn_sequence.h): every group's rows in (position, tie) order with their positions and ties beside them
    // (order | positions | ties, [3][seq_n]), built on the host by the first sequence search after the labels, the positions or
    // the id ranks changed (seq_n = the rows it covers, 0 = none; seq_largest = the longest group).  Scratch: cost keys (carry
    // [n] | two working arrays [2][n]), words (lo | hi | block minima [3][n] | end rows [G]), back-pointers
    IdxBuf<int32_t> d_seq; int64_t seq_n = 0; int64_t seq_largest = 0;
    IdxBuf<uint64_t> d_seqc;
    IdxBuf<int32_t> d_seqw;
    IdxBuf<int32_t> d_seqbp;
    // span search (knn_span.h): words (each chunk's spans (a, b) [chunk][G][2] | the global form's lo | pm | minima [3][n]), the
    // global form's prefix sums [n + G]
    IdxBuf<int32_t> d_spanw;
    IdxBuf<int64_t> d_spanp;
    // warped alignment (knn_align.h): the carried DP row's costs [n] | the groups' costs [G]; its starts [n] | the groups' (a, b)
    // [G][2] | the selection's groups [k]; a batch of winners' entry-column tables
    IdxBuf<int64_t> d_alignc;
    IdxBuf<int32_t> d_aligna;
    IdxBuf<int32_t> d_alignbp;
    // keyframe summary (knn_summary.h): the call's lists, keyframe counts and the wide form's per-row / per-block words; the
    // blocks' packed maxima; the mean's block sums and the widened mean directions
    IdxBuf<int32_t> d_sumw;
    IdxBuf<uint64_t> d_sumk;
    IdxBuf<double> d_sumd;
    // chapter segmentation (knn_segment.h): the call's entries, the chapters' cuts and a batch's back-pointers; a batch's prefix
    // rows and band tables; its global-form E keys
    IdxBuf<int32_t> d_segw;
    IdxBuf<double> d_segd;
    IdxBuf<uint64_t> d_sege;
    // zero-shot labelling (knn_label.h): control words {filed rows, flag, largest |p|^2} + the filed-row list + the rows' labels
    // and best distances (ctl [4] | filed [n_pad] | label [n_pad] | best [n_pad]); the exact path's running keys; the tile
    // path's parts
    IdxBuf<int32_t> d_lw;
    IdxBuf<uint64_t> d_lrun;
    IdxBuf<uint32_t> d_lparts;
    IdxBuf<int32_t> d_lgw;         // ... the split group form's lists, unlabelled counts and chosen labels; its pieces' histograms and show keys
    IdxBuf<uint32_t> d_lghist;
    IdxBuf<uint64_t> d_lgshow;
    // library clustering (knn_cluster.h): control words | previous labels | labels | distances | by-label row list [n each] |
    // counts | list offsets | piece offsets | counts and show rows of the host form [P + 1 each]; the blocks' label counts
    // [blocks][P]; the pieces' fp64 sums [pieces][dim]; the clusters' show keys [P]; the host form's changed counts (mapped:
    // cluster_scan_kernel writes one per iteration, the host reads it after its wait)
    IdxBuf<int32_t> d_clw;
    IdxBuf<uint32_t> d_cltab;
    IdxBuf<double> d_clsum;
    IdxBuf<uint64_t> d_clkey;
    PinnedBuf<int32_t> h_clchanged{true};
    // compound search (knn_compound.h): the exact path's term table [m][ld]
    IdxBuf<float> d_ctab;
    // shared-footage search (knn_match.h): the hit-bit table [m][ceil(n / 32)]; the filed (query, row) pairs; control words
    // (cursor, flag) + the groups' best-run keys [G]; the queries' threshold half-widths [m] + the selection's unused distances [k]
    IdxBuf<uint32_t> d_mbits;
    IdxBuf<uint64_t> d_mfiled;
    IdxBuf<uint64_t> d_mw;
    IdxBuf<float> d_mqe;
    // library neighbours (knn_neighbors.h): the call's row list; a chunk's tags; a chunk's gathered fp32 masters (row-list calls;
    // their fp16 copies go to d_q16).  Keys, flags, the redo's scratch and the counters are the fp16 search's and the grouped
    // search's (d_keys, d_flags, d_slots, d_counters, d_fb_partial; totals in d_gcounters)
    IdxBuf<int32_t> d_nbrows;
    IdxBuf<int32_t> d_nbtag;
    IdxBuf<float> d_nbq;
    // clip-search scratch (knn_set.h): per-group sums [2][G], candidate list / positions [2][G] + count + flag, |q_i| [m],
    // order keys [G] + the selection's block lists, candidate keys
    IdxBuf<double> d_ssum;
    IdxBuf<int32_t> d_scand;
    IdxBuf<float> d_sqn;
    IdxBuf<uint64_t> d_sekey;
    IdxBuf<uint64_t> d_sckeys;
    // fp16 scan scratch
    IdxBuf<uint16_t> d_q16;
    IdxBuf<uint32_t> d_keys;
    IdxBuf<int32_t> d_flags;
    // device-side fallback (knn_fallback.h): flagged query numbers, counters {flagged, proven, rescanned, fallback},
    // per-split top-k lists; the counters travel to pinned memory behind the search, read by last_search_stats.  h_counters is
    // mapped: a host-synchronous search lets its kernels write the counters there (h_counters.dev)
    IdxBuf<int32_t> d_slots;
    IdxBuf<int32_t> d_counters; PinnedBuf<int32_t> h_counters{true};
    IdxBuf<uint64_t> d_fb_partial;
    // host forms: pinned staging for the queries, and a pinned + MAPPED result buffer.  vq_index_search (host arrays in and out, the
    // reference caller's call) has its kernels write straight into it — no device-to-host copy command on the one-query path
    PinnedBuf<float> h_q;
    PinnedBuf<char> h_res{true};
    StatsAt stats_at = STATS_HOST;
    int64_t stats[3] = {0, 0, 0};
    // |row|^2 range of rows added without normalisation (device: min/max fp32 bits); read back lazily by the first
    // search after such an add.  near_unit = the fp16 scan's error bound applies (knn_scan_f16.h scan_eps_unit).
    IdxBuf<uint32_t> d_norm_range;
    bool norm_dirty = false, near_unit = true;
    float row_norm_max = 1.0f;
    ScanSwitches scan_switches;    // the fp16 search's A/B switches (scan_plan.h), read from the environment at create
    // What pass 1 of the last fp16 search left in d_keys / d_gbest (vq_index_debug_read_scan_keys / _group_best): host
    // bookkeeping only, no launch and no wait.  Forgotten when the rows change (rows_changed) or another search takes the buffer.
    // masked: 0 no filter, 1 a group filter's bitmap, 2 eligibility by tag (library neighbours).  kind: 1 the grouped search's
    // scan3_group_max, 2 the clip search's scan3_group_max, 3 set_group_max_kernel; chunks / tile_chunks: the query chunks of the
    // call that left the record, and how many of them ran set_group_max_kernel.
    struct LastScan { bool valid = false; int masked = 0; int layout = 0, cur = 0; int64_t streams = 0, q0 = 0; } last_scan;
    struct LastGroupScan { bool valid = false; int cur = 0; int32_t n_groups = 0; int64_t q0 = 0; int kind = 0, chunks = 0, tile_chunks = 0; } last_gscan;
    // What the tile paths of the last labelling and shared-footage calls left in d_lparts / d_mbits + d_mfiled
    // (vq_index_debug_read_label_parts / _match_bits), kept and forgotten like the two above.
    struct LastLabel { bool valid = false; int64_t n = 0, n_pad = 0; int ranges = 0, P = 0; } last_label;
    struct LastMatch { bool valid = false; int m = 0; int64_t W = 0, n = 0, cap = 0; } last_match;
    void rows_changed() { last_scan.valid = false; last_gscan.valid = false; last_label.valid = false; last_match.valid = false; }
    bool profiling = false;
    struct Ev { int cls; hipEvent_t a, b; };
    std::vector<Ev> events;
    std::vector<hipEvent_t> pool;
};

namespace {

struct Prof {
    vq_index* x; int cls; hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t get(vq_index* x) {
        if (!x->pool.empty()) { hipEvent_t ev = x->pool.back(); x->pool.pop_back(); return ev; }
        hipEvent_t ev; (void)hipEventCreate(&ev); return ev;
    }
    Prof(vq_index* i, int c) : x(i), cls(c) {
        if (x->profiling) { a = get(x); b = get(x); (void)hipEventRecord(a, x->stream); }
    }
    ~Prof() { if (x->profiling) { (void)hipEventRecord(b, x->stream); x->events.push_back({cls, a, b}); } }
};

int reserve_rows(vq_index* x, int64_t need) {
    if (need <= x->cap) return 0;
    int64_t ncap = std::max<int64_t>(need, std::max<int64_t>(1024, x->cap * 2));
    ncap = round_up(ncap, SCAN2_RANGE);       // the fp16 scans walk whole 1024/2048-row ranges
    IdxBuf<float> nr; IdxBuf<uint16_t> nh;                    // freed again if a step below fails
    hipError_t e = hipMalloc((void**)&nr.p, (size_t)ncap * x->dim * 4);
    if (e != hipSuccess) return fail(VQ_ERR_OOM, "index: hipMalloc of %lld rows failed: %s", (long long)ncap, hipGetErrorString(e));
    e = hipMalloc((void**)&nh.p, (size_t)ncap * x->dim * 2);
    if (e != hipSuccess) return fail(VQ_ERR_OOM, "index: hipMalloc (fp16 copy) failed: %s", hipGetErrorString(e));
    VQ_HIP(hipMemsetAsync(nh, 0, (size_t)ncap * x->dim * 2, x->stream));   // pad rows of the scan copy stay finite
    if (x->size > 0) {
        VQ_HIP(hipMemcpyAsync(nr, x->rows, (size_t)x->size * x->dim * 4, hipMemcpyDeviceToDevice, x->stream));
        VQ_HIP(hipMemcpyAsync(nh, x->rows16, (size_t)x->size * x->dim * 2, hipMemcpyDeviceToDevice, x->stream));
    }
    VQ_HIP(hipStreamSynchronize(x->stream));
    x->rows.swap(nr); x->rows16.swap(nh);                     // the old storage goes with nr / nh
    x->cap = ncap;
    return 0;
}

// at most 2048 workgroups of 256 threads for `count` items (grid-stride kernels)
int grid_for(int64_t count) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(count, 256), 2048)); }

// An asynchronous copy reads a buffer of the enclosing frame (or the caller's): whichever way that function is left (every VQ_HIP /
// VQ_TRY returns early on error), the stream is drained before the buffer dies (declare the guard after it: destroyed first).
struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } };

// The |row|^2 range starts at [1, 1].  Blocks on the stream (`init` is on this stack frame).
int init_norm_range(vq_index* x) {
    const uint32_t init[2] = {0x3f800000u, 0x3f800000u};            // 1.0f, 1.0f
    VQ_HIP(hipMemcpyAsync(x->d_norm_range, init, 8, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

// Rows the caller says are unit (HNSWIndex.load, SimpleVideoIndex) are measured instead of trusted.  The range only widens.
int measure_norm_range(vq_index* x, const float* d_rows, int64_t n) {
    if (!x->d_norm_range) {
        VQ_TRY(x->d_norm_range.reserve(2));
        VQ_TRY(init_norm_range(x));
    }
    hipLaunchKernelGGL(row_norm_range_kernel, dim3(cdiv(n, 4)), dim3(256), 0, x->stream, d_rows, n, x->dim, x->d_norm_range);
    x->norm_dirty = true;
    return 0;
}

// rows already on the device at x->rows + size*dim
int finish_add(vq_index* x, int64_t n, int normalize) {
    float* dst = x->rows + x->size * x->dim;
    {
        Prof p(x, I_NORMALIZE);
        if (normalize) hipLaunchKernelGGL(normalize_rows_kernel, dim3(cdiv(n, NORM_ROWS)), dim3(NORM_ROWS), 0, x->stream, dst, n, x->dim);
        else VQ_TRY(measure_norm_range(x, dst, n));
    }
    {
        Prof p(x, I_TO_F16);
        const int64_t count4 = n * x->dim / 4;
        hipLaunchKernelGGL(rows_to_f16_kernel, dim3(grid_for(count4)), dim3(256), 0, x->stream, dst, x->rows16 + x->size * x->dim, count4);
    }
    VQ_HIP(hipGetLastError());
    x->size += n;
    x->rows_changed();
    return 0;
}

// |row|^2 range -> near_unit / row_norm_max.  Blocks on the stream: called where the entry point blocks anyway (vq_index_add,
// vq_index_update_rows) so that searches after a host add stay asynchronous; the device-side add leaves it to the first search.
int refresh_norm_range(vq_index* x) {
    if (!x->norm_dirty) return 0;
    uint32_t range[2];
    VQ_HIP(hipMemcpyAsync(range, x->d_norm_range, 8, hipMemcpyDeviceToHost, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));
    const float lo = __builtin_bit_cast(float, range[0]), hi = __builtin_bit_cast(float, range[1]);
    x->near_unit = lo >= 0.5f && hi <= 2.0f;
    x->row_norm_max = hi > 1.0f ? sqrtf(hi) * 1.0001f : 1.0001f;
    x->norm_dirty = false;
    return 0;
}

// ---- what the search families share ----

// A kernel's dynamic-LDS limit (MaxDynamicSharedMemorySize) is set for the CURRENT device only.  A handle's memory and stream are one device's,
// so what has been set is remembered per handle (under its lock): a search pays a look at a short list, no lock and no call.
int set_dyn_lds(vq_index* x, const void* fn, size_t bytes) {
    for (const auto& d : x->dyn_lds)
        if (d.first == fn && d.second >= bytes) return 0;
    VQ_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    x->dyn_lds.emplace_back(fn, bytes);
    return 0;
}

// The one writer of where the last search's statistics are.  STATS_HOST carries the values {verified, rescanned, exact}: an exact
// path passes (0, 0, queries), a reader of arrived counters what it read.
void set_stats(vq_index* x, StatsAt at, int64_t verified = 0, int64_t rescanned = 0, int64_t exact = 0) {
    x->stats_at = at;
    if (at == STATS_HOST) { x->stats[0] = verified; x->stats[1] = rescanned; x->stats[2] = exact; }
}
void stats_from_counters(vq_index* x) {          // h_counters has arrived (the caller has waited for the stream)
    set_stats(x, STATS_HOST, x->h_counters[1], x->h_counters[2], x->h_counters[3]);
}

// Refusals.  fn: the entry point's name.
int check_mode(const char* fn, int mode) {
    VQ_CHECK(mode >= 0 && mode <= 2, "%s: mode %d unknown", fn, mode);
    return 0;
}
int check_ranks(const vq_index* x, const char* fn) {
    VQ_CHECK(x->rank_n == 0 || x->rank_n == x->size, "%s: the id ranks cover %lld rows, the index holds %lld "
             "(call vq_index_set_id_ranks again after adding rows, or clear them)", fn, (long long)x->rank_n, (long long)x->size);
    return 0;
}
// (labels that cover a non-empty index always have their host mirror: set_groups and remove_rows write both)
int check_labels(const vq_index* x, const char* fn) {
    VQ_CHECK(x->group_n == x->size && (int64_t)x->h_goff.size() == (int64_t)x->n_groups + 1, "%s: the group labels cover %lld rows, "
             "the index holds %lld (call vq_index_set_groups after adding rows)", fn, (long long)x->group_n, (long long)x->size);
    return 0;
}
int check_positions(const vq_index* x, const char* fn) {
    VQ_CHECK(x->pos_n == x->size, "%s: the positions cover %lld rows, the index holds %lld (call vq_index_set_positions after "
             "adding or removing rows)", fn, (long long)x->pos_n, (long long)x->size);
    return 0;
}
// mode 0 (auto): the fp16 scans pay once the matrix is large enough to amortise their fixed costs
constexpr int64_t FP16_AUTO_MIN_ROWS = 16384;
static_assert(DST_FP16_MIN_ROWS == FP16_AUTO_MIN_ROWS, "knn_distinct.h: the auto mode's threshold");
static_assert(NB_FP16_MIN_ROWS == FP16_AUTO_MIN_ROWS, "knn_neighbors.h: the auto mode's threshold");

// device memory with no result in any slot (b: the grouped forms' second id array, or null), where a search of a non-empty
// index finds nothing to look at (an empty filter; a peer's empty shard)
int fill_empty(vq_index* x, int64_t count, int32_t* a, int32_t* b, float* dist) {
    hipLaunchKernelGGL(fill_no_result_kernel, dim3(cdiv(count, 256)), dim3(256), 0, x->stream, a, dist, count);
    if (b) hipLaunchKernelGGL(fill_no_result_kernel, dim3(cdiv(count, 256)), dim3(256), 0, x->stream, b, dist, count);
    VQ_HIP(hipGetLastError());
    return 0;
}

// ---- a family's outputs (host_buffers.h: OutField, Outs) ----
// Both forms of a family run one call sequence; the form says where its arrays are and how the queries reach the device.
enum Form {
    ON_DEVICE,         // the _device form: queries and outputs are device memory, nothing is copied, nothing waits
    HOST_PINNED,       // a host form whose queries go up through the pinned staging buffer
    HOST_PAGEABLE,     // a host form whose queries go up straight from the caller's memory
};

// device memory <- the field's empty value, on the stream (a 64-bit empty value repeats its 32-bit half: only zero is in use)
int out_fill_stream(vq_index* x, void* p, const OutField& f) {
    if (p && f.count) VQ_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)(uint32_t)f.empty, f.bytes() / 4, x->stream));
    return 0;
}

// The answer of an empty index: every field that was asked for holds its empty value, written on the host (host forms) or on
// the stream (device forms).  The statistics read zero.
int outs_empty(vq_index* x, Form form, const Outs& o) {
    for (int i = 0; i < o.n; ++i) {
        if (!o.f[i].dst) continue;
        if (form == ON_DEVICE) VQ_TRY(out_fill_stream(x, o.f[i].dst, o.f[i]));
        else out_fill_host(o.f[i].dst, o.f[i]);
    }
    set_stats(x, STATS_HOST, 0, 0, 0);
    return 0;
}

// ... and of a run that finds nothing to look at (a filter that allows no row): the placed fields, on the stream
int outs_empty_placed(vq_index* x, const Outs& o) {
    for (int i = 0; i < o.n; ++i) VQ_TRY(out_fill_stream(x, o.f[i].dev, o.f[i]));
    return 0;
}

int host_results(vq_index* x, int64_t bytes) {          // h_res holds at least `bytes` (pinned + mapped; the stream is idle when it is replaced)
    if (bytes <= x->h_res.cap) return 0;
    VQ_HIP(hipStreamSynchronize(x->stream));
    return x->h_res.reserve(bytes, 64 << 10);
}

// Where the run writes each field.  Device forms: the caller's arrays.  Host forms: pieces of d_res (outs_layout), except for
// owned fields, whose `dev` the family sets itself; a field that was not asked for keeps dev = null.
int outs_place(vq_index* x, Form form, Outs* o) {
    if (form == ON_DEVICE) {
        for (int i = 0; i < o->n; ++i) o->f[i].dev = o->f[i].dst;
        return 0;
    }
    int64_t off[OUT_MAX_FIELDS];
    const int64_t bytes = outs_layout(*o, off);
    VQ_TRY(x->d_res.reserve(bytes));
    if (o->how != COPY_TO_CALLER) VQ_TRY(host_results(x, bytes));
    for (int i = 0; i < o->n; ++i)
        if (off[i] >= 0) o->f[i].dev = x->d_res.p + off[i];
    return 0;
}

// Host forms: every field that was asked for, from where the run wrote it to the caller's array, in list order; then the call's
// one wait.  Device forms: nothing.
int outs_return(vq_index* x, Form form, const Outs& o) {
    if (form == ON_DEVICE) return 0;
    auto pinned = [&](const OutField& f) { return x->h_res.p + ((char*)f.dev - x->d_res.p); };
    if (o.how == COPY_PINNED_BLOCK) {
        int64_t off[OUT_MAX_FIELDS];
        VQ_HIP(hipMemcpyAsync(x->h_res, x->d_res, (size_t)outs_layout(o, off), hipMemcpyDeviceToHost, x->stream));
    } else {
        for (int i = 0; i < o.n; ++i)
            if (o.f[i].dst)
                VQ_HIP(hipMemcpyAsync(o.how == COPY_TO_CALLER ? o.f[i].dst : pinned(o.f[i]), o.f[i].dev, o.f[i].bytes(), hipMemcpyDeviceToHost, x->stream));
    }
    VQ_HIP(hipStreamSynchronize(x->stream));
    if (o.how != COPY_TO_CALLER)
        for (int i = 0; i < o.n; ++i)
            if (o.f[i].dst) std::memcpy(o.f[i].dst, pinned(o.f[i]), o.f[i].bytes());
    return 0;
}

// A host form's queries [nq][dim] -> d_q, by the form's route: through the pinned staging buffer (vq_index_search's fast path,
// the filtered searches and every family from the clip search on, the two debug passes, the cluster update), or straight from
// the caller's pageable memory (the plain search's large batches, the grouped, distinct and diverse searches).  Each form keeps
// the route it was written with: on large batches the runtime stages a pageable copy itself, in pieces, and which route wins
// there has not been measured, so the two are not merged here.
int stage_queries(vq_index* x, const float* queries, int nq, Form route = HOST_PINNED) {
    const int64_t count = (int64_t)nq * x->dim;
    VQ_TRY(x->d_q.reserve(count));
    if (route == HOST_PINNED) {
        VQ_TRY(x->h_q.reserve(count, (64 << 10) / 4));
        std::memcpy(x->h_q, queries, (size_t)count * 4);
        queries = x->h_q;
    }
    VQ_HIP(hipMemcpyAsync(x->d_q, queries, (size_t)count * 4, hipMemcpyHostToDevice, x->stream));
    return 0;
}

// What the two forms of a family share behind their refusals: the queries get to the device (or are there), the outputs get
// their places, `run(d_queries)` queues the work, the host form's results come back.
template <class Run>
int run_form(vq_index* x, Form form, const float* queries, int nq, Outs* o, Run run) {
    if (form != ON_DEVICE && queries) VQ_TRY(stage_queries(x, queries, nq, form));       // (a family without queries passes null)
    VQ_TRY(outs_place(x, form, o));
    VQ_TRY(run(form == ON_DEVICE ? queries : x->d_q.p));
    return outs_return(x, form, *o);
}

// Host forms: is every |q|^2 of q [count][dim] inside what the fp16 bound covers?  what (a query's name in the message) set:
// a value that is not finite is refused.  what null: nothing is refused, and such a query simply reads as out of range.
int queries_in_range(const char* fn, const char* what, const float* q, int count, int dim, bool* in_range) {
    *in_range = true;
    for (int j = 0; j < count; ++j) {
        double s2 = 0.0;
        for (int i = 0; i < dim; ++i) {
            const float v = q[(size_t)j * dim + i];
            if (what) VQ_CHECK(v - v == 0.f, "%s: %s %d holds a value that is not finite", fn, what, j);
            s2 += (double)v * v;
        }
        if (!(s2 >= SCAN_Q2_MIN && s2 <= SCAN_Q2_MAX)) *in_range = false;
    }
    return 0;
}

// queries [cur][dim] -> d_q16 [q_pad][dim], zero rows behind cur
void queries_to_f16(vq_index* x, const float* d_queries, int cur, int64_t q_pad) {
    Prof p(x, I_TO_F16);
    hipLaunchKernelGGL(queries_to_f16_kernel, dim3(grid_for(q_pad * x->dim / 4)), dim3(256), 0, x->stream, d_queries, x->d_q16, cur, q_pad, x->dim);
}

// fp64-chain distances of `cur` queries to every row -> d_dist [cur][ld].  small: the one-launch kernel that keeps up to EDS_MAX_Q
// queries in LDS (knn_kernels.h); it exists when exact_small_fits(), and each caller has its own rule for taking it.
bool exact_small_fits(const vq_index* x) { return (size_t)EDS_MAX_Q * x->dim * 8 <= (size_t)96 << 10; }
int exact_dist(vq_index* x, bool small, const float* qp, int cur, int64_t ld) {
    const int64_t n = x->size;
    const size_t qbytes = (size_t)EDS_MAX_Q * x->dim * 8;
    if (small) VQ_TRY(set_dyn_lds(x, (const void*)exact_dist_small_kernel, qbytes));
    Prof p(x, I_EXACT_DIST);
    if (small)
        hipLaunchKernelGGL(exact_dist_small_kernel, dim3(cdiv(n, 64)), dim3(256), qbytes, x->stream, x->rows, n, x->dim, qp, cur, x->d_dist, ld);
    else
        hipLaunchKernelGGL(exact_dist_kernel, dim3(cdiv(n, 64), cdiv(cur, 32)), dim3(256), 0, x->stream, x->rows, n, x->dim, qp, cur, x->d_dist, ld);
    return 0;
}

// The exact paths' selection: per slice of queries, `dist(q0, cur, ld)` queues the distances to m columns into d_dist [cur][ld],
// then the k best columns of each query under `tie` -> ids / out.  one_wg: one workgroup per query (select_small_kernel, at most
// SEL_SMALL_MAX_N columns) instead of chunks + merge.
template <class Dist>
int exact_topk(vq_index* x, int64_t m, int nq, int k, bool one_wg, const TieOrder tie, int32_t* ids, float* out, Dist dist) {
    const int64_t ld = round_up(m, 64);
    const int64_t budget = (int64_t)128 << 20;                 // 512 MiB of fp32 distances per slice
    const int qslice = (int)std::max<int64_t>(32, std::min<int64_t>(nq, budget / ld) / 32 * 32);
    VQ_TRY(x->d_dist.reserve((int64_t)std::min(qslice, (int)round_up(nq, 32)) * ld));
    const int nchunks = cdiv(m, SEL_CHUNK);
    if (!one_wg) VQ_TRY(x->d_partial.reserve((int64_t)std::min(qslice, nq) * nchunks * k));
    for (int q0 = 0; q0 < nq; q0 += qslice) {
        const int cur = std::min(qslice, nq - q0);
        int32_t* ids0 = ids + (int64_t)q0 * k;
        float* out0 = out + (int64_t)q0 * k;
        VQ_TRY(dist(q0, cur, ld));
        Prof p(x, I_SELECT);
        if (one_wg) {
            hipLaunchKernelGGL(select_small_kernel, dim3(cur), dim3(256), 0, x->stream, x->d_dist, ld, m, k, ids0, out0, tie, nullptr, 0);
        } else {
            hipLaunchKernelGGL(select_chunk_kernel, dim3(cur, nchunks), dim3(256), 0, x->stream, x->d_dist, ld, m, k, nchunks, x->d_partial, tie, nullptr, 0);
            hipLaunchKernelGGL(merge_topk_kernel, dim3(cur), dim3(256), 0, x->stream, x->d_partial, nchunks, k, ids0, out0, tie, nullptr, 0);
        }
    }
    VQ_HIP(hipGetLastError());
    set_stats(x, STATS_HOST, 0, 0, nq);
    return 0;
}

// Exact scan: fp64-chain distances for a slice of queries into d_dist, then selection.
int search_exact(vq_index* x, const float* d_queries, int nq, int k, int32_t* d_ids, float* d_dist_out) {
    // a handful of queries over a small index — the reference caller's one search at a time over a few thousand frames:
    // two short launches (knn_kernels.h)
    const bool small = nq <= EDS_MAX_Q && x->size <= SEL_SMALL_MAX_N && x->dim % 4 == 0 && exact_small_fits(x);
    return exact_topk(x, x->size, nq, k, small, x->tie(), d_ids, d_dist_out, [&](int q0, int cur, int64_t ld) {
        return exact_dist(x, small, d_queries + (int64_t)q0 * x->dim, cur, ld);
    });
}

// Device-side fallback geometry (knn_fallback.h).  First round: the first FB_FAST_SLOTS flagged queries over fine row splits (many
// short workgroups: the usual handful of unproven queries is back in ~0.1 ms); bulk rounds: the rest over coarse splits, as many
// flagged queries per round as 64 MiB of per-split lists hold.  One scratch buffer (d_fb_partial) serves both.
struct FallbackPlan {
    int fast_splits, splits;       // row splits of the first round / of a bulk round
    int64_t fast_rows, rows;       // rows per split
    int64_t round_q;               // flagged queries per bulk round
    int64_t partial;               // elements of d_fb_partial
};
FallbackPlan fallback_plan(int64_t n, int nq, int k) {
    FallbackPlan f;
    f.fast_splits = (int)std::max<int64_t>(1, std::min<int64_t>(FB_MAX_SPLITS, cdiv(n, FB_FAST_ROWS)));
    f.fast_rows = round_up(cdiv(n, f.fast_splits), FB_TILE);
    f.fast_splits = std::max(1, cdiv(n, f.fast_rows));          // whole tiles per split can leave the last splits without a row: not launched
    f.splits = (int)std::max<int64_t>(1, std::min<int64_t>(FB_MAX_SPLITS, cdiv(n, FB_SPLIT_ROWS)));
    f.rows = round_up(cdiv(n, f.splits), FB_TILE);
    f.splits = std::max(1, cdiv(n, f.rows));
    f.round_q = std::max<int64_t>(FB_QG, std::min<int64_t>(round_up(nq, FB_QG), ((int64_t)64 << 20) / ((int64_t)f.splits * k * 8) / FB_QG * FB_QG));
    f.partial = std::max<int64_t>(f.round_q * f.splits, (int64_t)FB_FAST_SLOTS * f.fast_splits) * k;
    return f;
}

// the fp16 paths' outcome counters {flagged, proven, rescanned, fallback} and their pinned, mapped copy
int ensure_counters(vq_index* x) {
    VQ_TRY(x->d_counters.reserve(FB_NCOUNTERS));
    return x->h_counters.reserve(FB_NCOUNTERS);
}
// the grouped and clip fp16 paths' counters and their pinned copy
int ensure_gcounters(vq_index* x) {
    VQ_TRY(x->d_gcounters.reserve(3));
    return x->h_gcounters.reserve(3);
}

// what launch_fallback needs for nq queries: the flagged-query list, the counters, the per-split lists
int reserve_fallback(vq_index* x, int nq, int k) {
    VQ_TRY(x->d_slots.reserve(round_up(nq, 1024)));
    VQ_TRY(ensure_counters(x));
    return x->d_fb_partial.reserve(fallback_plan(x->size, nq, k).partial);
}

// The exact redo of the queries whose proof did not close (knn_fallback.h), sized from the device-side flagged count.
// mask (filtered search): the masked kernel, which lists allowed rows only
// elig (library neighbours): the per-query eligibility of knn_fallback.h's second template parameter
template <class Elig = EligAll>
void launch_fallback(vq_index* x, const float* d_queries, int nq, int k, int32_t* d_ids, float* d_dist_out, const int32_t* counters,
                     const GroupMask* mask = nullptr, const Elig elig = Elig{}) {
    auto fb = mask ? exact_fallback_kernel<true, Elig> : exact_fallback_kernel<false, Elig>;
    const GroupMask gm = mask ? *mask : GroupMask{};
    const int64_t n = x->size;
    const FallbackPlan f = fallback_plan(n, nq, k);
    Prof p(x, I_EXACT_DIST);
    hipLaunchKernelGGL(fb, dim3(f.fast_splits, 1), dim3(FB_TILE), 0, x->stream, x->rows, n, x->dim,
                       d_queries, x->d_slots, counters, 0, FB_FAST_SLOTS, k, f.fast_rows, x->d_fb_partial, x->tie(), gm, elig);
    hipLaunchKernelGGL(fallback_merge_kernel, dim3(FB_FAST_SLOTS), dim3(256), 0, x->stream, x->d_fb_partial, f.fast_splits, k, x->d_slots,
                       counters, 0, FB_FAST_SLOTS, d_ids, d_dist_out, x->tie());
    for (int64_t base = FB_FAST_SLOTS; base < nq; base += f.round_q) {
        hipLaunchKernelGGL(fb, dim3(f.splits, FB_SLOT_LANES), dim3(FB_TILE), 0, x->stream, x->rows, n, x->dim,
                           d_queries, x->d_slots, counters, (int)base, (int)f.round_q, k, f.rows, x->d_fb_partial, x->tie(), gm, elig);
        hipLaunchKernelGGL(fallback_merge_kernel, dim3(64), dim3(256), 0, x->stream, x->d_fb_partial, f.splits, k, x->d_slots,
                           counters, (int)base, (int)f.round_q, d_ids, d_dist_out, x->tie());
    }
}

// ---- fp16 MFMA scan + exact re-score with proof (scan_plan.h decides, these launch); unproven queries go through the fallback ----
// the streaming scan's instance for the handle's dim (256, 512 or 768) and the groups of 16 queries it holds per pass (two: the
// plain form at dim <= 512).  FUSED: fp32 queries, rounded by the scan; MASK: the filtered search's
template <bool FUSED, bool MASK>
auto scan3_instance(int dim, int nqg) -> decltype(&scan3_f16_top2_kernel<8, 1, FUSED, MASK>) {
    if constexpr (!FUSED && !MASK)
        if (nqg == 2 && dim != 768) return dim == 512 ? scan3_f16_top2_kernel<16, 2> : scan3_f16_top2_kernel<8, 2>;
    return dim == 768 ? scan3_f16_top2_kernel<24, 1, FUSED, MASK> : dim == 512 ? scan3_f16_top2_kernel<16, 1, FUSED, MASK>
                                                                              : scan3_f16_top2_kernel<8, 1, FUSED, MASK>;
}
// streaming group-max scan (grouped and clip search): the instance for the handle's dim, masked by the allowed groups' bitmap or not
template <bool MASK>
auto scan3_group_max_instance(int dim) -> decltype(&scan3_group_max_kernel<8, MASK>) {
    return dim == 768 ? scan3_group_max_kernel<24, MASK> : dim == 512 ? scan3_group_max_kernel<16, MASK> : scan3_group_max_kernel<8, MASK>;
}
auto scan3_group_max(int dim, bool masked) -> decltype(&scan3_group_max_kernel<8>) {
    return masked ? scan3_group_max_instance<true>(dim) : scan3_group_max_instance<false>(dim);
}

// One chunk's scan: `cur` queries -> d_keys.  qp: the chunk's fp32 queries, which only the fused streaming scan reads; every other
// scan reads d_q16 (queries_to_f16).
int launch_scan(vq_index* x, const ScanPlan& p, const float* qp, int cur) {
    const int64_t n = x->size, qpad = q_pad(p, cur);
    const int qt = q_tiles(p, cur);
    const ScanGrid g = scan_grid(p, cur);
    auto fold = scan5_f16_top2_kernel<0>;
    switch (p.scan) {
        case SCAN_STREAM: {
            Prof pr(x, I_MFMA_SCAN);
            if (p.fused_q)
                hipLaunchKernelGGL((scan3_instance<true, false>(x->dim, 1)), dim3(g.x, g.y), dim3(256), 0, x->stream, (const uint16_t*)qp, x->rows16, n,
                                   p.streams, qpad, x->d_keys, cur, GroupMask{});
            else
                hipLaunchKernelGGL((scan3_instance<false, false>(x->dim, p.nqg)), dim3(g.x, g.y), dim3(256), 0, x->stream, x->d_q16, x->rows16, n,
                                   p.streams, qpad, x->d_keys, 0, GroupMask{});
            return 0;
        }
        case SCAN_TILE128: {
            Prof pr(x, I_MFMA_SCAN);
            hipLaunchKernelGGL(scan_f16_top2_kernel, dim3(g.x), dim3(GEMM_THREADS), 0, x->stream, x->d_q16, x->rows16, x->dim, n, qt, qpad, x->d_keys);
            return 0;
        }
        case SCAN_FOLD: break;
#ifdef VQ_DIAG
        case SCAN_FOLD_NONE: fold = scan5_f16_top2_kernel<1>; break;
        case SCAN_FOLD_AFTER: fold = scan5_f16_top2_kernel<2>; break;
        case SCAN_FOLD_CLEAR: fold = scan5_f16_top2_kernel<0, false>; break;
#endif
        default:
#ifdef VQ_SCAN_EXPERIMENTS
            if (const void* fn = scan_experiment_kernel(p.scan)) {
                VQ_TRY(set_dyn_lds(x, fn, p.scan_lds));
                Prof pr(x, I_MFMA_SCAN);
                launch_scan_experiment(p.scan, g.x, p.scan_lds, x->stream, x->d_q16, x->rows16, x->dim, n, qt, p.ranges, range_groups(p), qpad, x->d_keys);
                return 0;
            }
#endif
            return fail(VQ_ERR_STATE, "scan plan names kind %d, which this build does not carry", p.scan);
    }
    VQ_TRY(set_dyn_lds(x, (const void*)fold, p.scan_lds));
    Prof pr(x, I_MFMA_SCAN);
    hipLaunchKernelGGL(fold, dim3(g.x), dim3(G2_THREADS), p.scan_lds, x->stream, x->d_q16, x->rows16, x->dim, n, qt, p.ranges, range_groups(p), qpad,
                       x->d_keys, x->dim, p.rb);
    return 0;
}

// One chunk's re-score: d_keys -> the exact top-k of `cur` queries (ids, dist) and their outcome (flags).  counters: where a
// re-score workgroup that files its own flag writes the outcome counters (plan.rescore_files_flags).
int launch_rescore(vq_index* x, const ScanPlan& p, const float* qp, int cur, int k, int32_t* ids, float* dist, int32_t* flags, int32_t* counters) {
    const int64_t n = x->size, qpad = q_pad(p, cur);
    const float eps_rows = scan_eps_unit(x->dim) * x->row_norm_max;
    const dim3 grid(rescore_grid(p, cur));
    auto batch = rescore_verify_kernel;                 // several queries per workgroup, or one: told the key layout
    auto one = rescore_verify_small_kernel;             // one query per workgroup, its candidate rows in LDS: the streaming scan's keys only
    size_t one_lds_max = 0;                             // ... the limit is raised to what the largest dim takes: it is the kernel's, not this handle's
    switch (p.rescore) {
        case RESCORE_BATCH8: break;
        case RESCORE_LARGE4: batch = rescore_verify_large_kernel; break;
        case RESCORE_XLARGE4: batch = rescore_verify_xlarge_kernel; break;
        case RESCORE_LARGE1: batch = rescore_verify_large1_kernel; break;
        case RESCORE_XLARGE1: batch = rescore_verify_xlarge1_kernel; break;
        case RESCORE_SMALL32: one_lds_max = (RV_C * (768 + 4) + 768) * 4; break;
        case RESCORE_SMALL64: one = rescore_verify_small64_kernel; one_lds_max = (64 * (512 + 4) + 512) * 4; break;
        default: return fail(VQ_ERR_STATE, "scan plan names re-score kind %d", p.rescore);
    }
    if (one_lds_max) VQ_TRY(set_dyn_lds(x, (const void*)one, one_lds_max));
    Prof pr(x, I_RESCORE);
    if (one_lds_max)
        hipLaunchKernelGGL(one, grid, dim3(256), (size_t)p.rescore_lds, x->stream, x->d_keys, p.streams, qpad, x->rows, n, x->dim, qp, cur, k, ids, dist, flags,
                           eps_rows, p.rescore_files_flags ? x->d_slots.p : nullptr, p.rescore_files_flags ? counters : nullptr, x->tie());
    else
        hipLaunchKernelGGL(batch, grid, dim3(256), 0, x->stream, x->d_keys, p.streams, qpad, x->rows, n, x->dim, qp, cur, k, ids, dist, flags, p.layout,
                           eps_rows, x->tie(), EligAll{});
    return 0;
}

// host_sync: the caller (vq_index_search) waits for the stream anyway, so the outcome counters are written by the kernels into
// host-visible memory and the fallback launches are left to it — it reads the flagged count after its one wait and launches
// them only when there is something to redo (normally nothing: two launches and a copy command fewer per search).
int search_fp16(vq_index* x, const float* d_queries, int nq, int k, int32_t* d_ids, float* d_dist_out, bool host_sync = false) {
    const ScanPlan p = plan_scan(x->dim, x->size, nq, k, x->scan_switches, SCAN_DIAG_BUILD, SCAN_EXPERIMENTS_BUILD);
    if (p.err) return fail(p.err, "%s", p.msg);
    VQ_TRY(x->d_q16.reserve(p.q_chunk * x->dim));
    VQ_TRY(x->d_keys.reserve(p.streams * p.q_chunk * 2));
    VQ_TRY(x->d_flags.reserve(q_pad(p, nq)));
    VQ_TRY(reserve_fallback(x, nq, k));
    int32_t* const counters = host_sync ? x->h_counters.dev : x->d_counters.p;
    x->last_scan.valid = false;
    for (int64_t q0 = 0; q0 < nq; q0 += p.q_chunk) {
        const int cur = (int)std::min<int64_t>(p.q_chunk, nq - q0);
        const float* qp = d_queries + q0 * x->dim;
        if (!p.fused_q) queries_to_f16(x, qp, cur, q_pad(p, cur));
        VQ_TRY(launch_scan(x, p, qp, cur));
        x->last_scan = {true, false, p.layout, cur, p.streams, q0};
        VQ_TRY(launch_rescore(x, p, qp, cur, k, d_ids + q0 * k, d_dist_out + q0 * k, x->d_flags + q0, counters));
    }
    VQ_HIP(hipGetLastError());
    // Queries the proof could not close are redone by the exact scan, on the device: the flags are compacted into a
    // list and the fallback kernels size themselves from its length (all of them leave at once when it is empty), so
    // nothing here waits for the stream.  Rounds beyond the first exist only when more queries could be flagged than
    // one round's scratch holds.
    if (!p.rescore_files_flags)
        hipLaunchKernelGGL(collect_flags_kernel, dim3(1), dim3(1024), 0, x->stream, x->d_flags, nq, x->d_slots, counters);
    VQ_HIP(hipGetLastError());
    if (host_sync) { set_stats(x, STATS_DEFERRED); return 0; }
    launch_fallback(x, d_queries, nq, k, d_ids, d_dist_out, counters);
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_counters, x->d_counters, FB_NCOUNTERS * 4, hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_COUNTERS);
    return 0;
}

int search_dispatch(vq_index* x, const float* d_queries, int nq, int k, int mode, int32_t* d_ids, float* d_dist, bool host_sync = false) {
    static const char* fn = "vq_index_search";
    VQ_TRY(check_mode(fn, mode));
    VQ_TRY(check_ranks(x, fn));
    // rows were added un-normalised ON THE DEVICE since the last look (vq_index_add_device: the one add that does not block):
    // is the matrix still near-unit?  This is the only place a search waits for its stream.
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    const bool fp16_ok = x->dim % GEMM_BK == 0 && k <= RV_K_MAX && x->size >= 1 && x->near_unit;
    if (mode == 2) VQ_CHECK(fp16_ok, "vq_index_search: fp16 scan needs dim %% 64 == 0, k <= %d and near-unit rows "
                                     "(0.5 <= |row|^2 <= 2; rows added with normalize=0 are measured)", RV_K_MAX);
    const bool use_fp16 = mode == 2 || (mode == 0 && fp16_ok && x->size >= FP16_AUTO_MIN_ROWS);
    return use_fp16 ? search_fp16(x, d_queries, nq, k, d_ids, d_dist, host_sync) : search_exact(x, d_queries, nq, k, d_ids, d_dist);
}

// ---- grouped search (knn_grouped.h) ----
// lanes per group in group_block_topk_kernel / set_group_min_kernel, from the mean group size
int lanes_per_group(int64_t rows, int32_t groups) {
    const int64_t mean = rows / std::max<int32_t>(1, groups);
    return mean >= 256 ? 64 : mean >= 64 ? 16 : mean >= 8 ? 4 : 1;
}

// The grouped exact paths' selection: per slice of queries, `dist(q0, cur, ld)` queues the distances to m columns into d_dist
// [cur][ld]; block_topk takes the minimum of each of G groups (columns goff / grows) and each block's k best; then the merge.
template <class Dist>
int grouped_exact_topk(vq_index* x, decltype(&group_block_topk_kernel<true>) block_topk, int64_t m, int G, const int32_t* goff,
                       const int32_t* grows, const TieOrder tie, int nq, int k, int32_t* groups, int32_t* rows_out, float* dist_out, Dist dist) {
    const int64_t ld = round_up(m, 64);
    const int nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK), lpg = lanes_per_group(m, G);
    int64_t qslice = std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)128 << 20) / ld));          // 512 MiB of distances per slice
    qslice = std::max<int64_t>(1, std::min<int64_t>(qslice, ((int64_t)32 << 20) / ((int64_t)nblocks * kl)));   // 256 MiB of block lists
    VQ_TRY(x->d_dist.reserve(qslice * ld));
    VQ_TRY(x->d_gpart.reserve(qslice * nblocks * kl));
    for (int64_t q0 = 0; q0 < nq; q0 += qslice) {
        const int cur = (int)std::min<int64_t>(qslice, nq - q0);
        VQ_TRY(dist(q0, cur, ld));
        Prof p(x, I_SELECT);
        hipLaunchKernelGGL(block_topk, dim3(nblocks, cur), dim3(256), 0, x->stream, x->d_dist, ld, nullptr, x->dim, nullptr, goff, grows, G, lpg, kl,
                           nblocks, x->d_gpart, nullptr, tie, nullptr);
        hipLaunchKernelGGL(group_merge_kernel, dim3(cur), dim3(256), 0, x->stream, x->d_gpart, nblocks * kl, k, x->d_group,
                           groups + q0 * k, rows_out + q0 * k, dist_out + q0 * k, nullptr, tie);
    }
    VQ_HIP(hipGetLastError());
    set_stats(x, STATS_HOST, 0, 0, nq);
    return 0;
}

// Exact path: the plain path's fp64-chain distances for a slice of queries -> group minima and each block's k best -> merge.
int search_grouped_exact(vq_index* x, const float* d_queries, int nq, int k, int32_t* groups, int32_t* rows_out, float* dist) {
    const bool small = exact_small_fits(x) && nq <= EDS_MAX_Q;
    return grouped_exact_topk(x, group_block_topk_kernel<true>, x->size, x->n_groups, x->d_goff, x->d_grows, x->tie(), nq, k, groups, rows_out, dist,
                              [&](int64_t q0, int cur, int64_t ld) { return exact_dist(x, small, d_queries + q0 * x->dim, cur, ld); });
}

// fp16 path: group-max scan -> threshold + candidates -> exact re-score of the candidates' rows; flagged queries are redone
// exactly on the device (group_block_topk_kernel<false> computes their distances itself), so nothing here waits.
// allow (filtered search): the allowed groups' bitmap, n_allowed of them.  Pass 1 skips the rest, pass 2 selects among the
// allowed groups only (their gbest stays 0, below every row), the redo walks only allowed groups.
int search_grouped_fp16(vq_index* x, const float* d_queries, int nq, int k, int32_t* groups, int32_t* rows_out, float* dist,
                        const uint32_t* allow = nullptr, int32_t n_allowed = 0) {
    const int64_t n = x->size, streams = cdiv(n, SCAN_STREAM_ROWS), CA = GRP_CAND_MAX;
    const int G = x->n_groups, nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK);
    int64_t qc = std::max<int64_t>(16, ((int64_t)64 << 20) / G / 16 * 16);          // gbest [qc][G]: <= 256 MiB
    qc = std::min<int64_t>(std::min<int64_t>(qc, round_up(nq, 16)), 1024);
    while (qc > 16 && qc * nblocks * kl > ((int64_t)32 << 20)) qc -= 16;               // the redo's block lists: <= 256 MiB
    VQ_TRY(x->d_q16.reserve(qc * x->dim));
    VQ_TRY(x->d_gbest.reserve(qc * G));
    VQ_TRY(x->d_gcand.reserve(qc * CA + qc * (CA + 1) + 3 * qc));
    VQ_TRY(x->d_gkeys.reserve(qc * CA));
    VQ_TRY(x->d_gpart.reserve(qc * nblocks * kl));
    VQ_TRY(ensure_gcounters(x));
    int32_t* cand = x->d_gcand;
    int32_t* pref = cand + qc * CA;
    int32_t* cn = pref + qc * (CA + 1);
    int32_t* flags = cn + qc;
    float* thr = (float*)(flags + qc);
    VQ_HIP(hipMemsetAsync(x->d_gcounters, 0, 3 * sizeof(unsigned long long), x->stream));
    const float eps_rows = scan_eps_unit(x->dim) * x->row_norm_max;
    auto scan = scan3_group_max(x->dim, allow != nullptr);
    auto redo = allow ? group_block_topk_kernel<false, true> : group_block_topk_kernel<false>;
    // k among the allowed groups: the threshold is the k'-th largest gbest with k' = min(k, allowed) (a disallowed group's 0 is
    // below it), the finalize test asks for min(k, allowed) re-scored groups
    const int k_sel = allow ? std::min(k, (int)n_allowed) : k, g_fin = allow ? n_allowed : G;
    x->last_gscan.valid = false;
    for (int64_t q0 = 0; q0 < nq; q0 += qc) {
        const int cur = (int)std::min<int64_t>(qc, nq - q0);
        const int64_t q_pad = round_up(cur, 16);
        const float* qp = d_queries + q0 * x->dim;
        queries_to_f16(x, qp, cur, q_pad);
        VQ_HIP(hipMemsetAsync(x->d_gbest, 0, (size_t)cur * G * 4, x->stream));
        {
            Prof p(x, I_MFMA_SCAN);
            hipLaunchKernelGGL(scan, dim3(cdiv(streams, 4), (int)(q_pad / 16)), dim3(256), 0, x->stream, x->d_q16, x->rows16, streams,
                               x->d_group, x->d_sgroup, cur, G, x->d_gbest, allow);
        }
        x->last_gscan = {true, cur, (int32_t)G, q0, 1, 1, 0};
        {
            Prof p(x, I_RESCORE);
            hipLaunchKernelGGL(group_threshold_kernel, dim3(cur), dim3(256), 0, x->stream, x->d_gbest, G, k_sel, qp, x->dim, eps_rows, x->d_goff,
                               cand, pref, cn, thr, x->d_gkeys, flags);
            hipLaunchKernelGGL(group_rescore_kernel, dim3(GRP_RESCORE_SPLITS, cur), dim3(256), 0, x->stream, x->d_q16, qp, x->rows, x->rows16,
                               x->dim, x->d_goff, x->d_grows, cand, pref, cn, thr, flags, x->d_gkeys, x->d_gcounters, x->tie());
            hipLaunchKernelGGL(group_finalize_kernel, dim3(cur), dim3(256), 0, x->stream, cn, x->d_gkeys, k, g_fin, x->d_group, flags,
                               groups + q0 * k, rows_out + q0 * k, dist + q0 * k, x->d_gcounters, x->tie());
        }
        {
            Prof p(x, I_EXACT_DIST);                 // the exact redo of flagged queries (every workgroup of an unflagged query leaves at once)
            hipLaunchKernelGGL(redo, dim3(nblocks, cur), dim3(256), 0, x->stream, nullptr, 0, x->rows, x->dim, qp,
                               x->d_goff, x->d_grows, G, lanes_per_group(n, G), kl, nblocks, x->d_gpart, flags, x->tie(), allow);
            hipLaunchKernelGGL(group_merge_kernel, dim3(cur), dim3(256), 0, x->stream, x->d_gpart, nblocks * kl, k, x->d_group,
                               groups + q0 * k, rows_out + q0 * k, dist + q0 * k, flags, x->tie());
        }
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

int search_grouped_dispatch(vq_index* x, const float* d_queries, int nq, int k, int mode, int32_t* groups, int32_t* rows_out, float* dist) {
    static const char* fn = "vq_index_search_grouped";
    VQ_TRY(check_mode(fn, mode));
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    const bool fp16_ok = (x->dim == 256 || x->dim == 512 || x->dim == 768) && k <= RV_K_MAX && x->size >= 1 && x->near_unit;
    if (mode == 2) VQ_CHECK(fp16_ok, "vq_index_search_grouped: the fp16 scan needs dim 256, 512 or 768, k <= %d and near-unit rows "
                                     "(0.5 <= |row|^2 <= 2; rows added with normalize=0 are measured)", RV_K_MAX);
    const bool use_fp16 = mode == 2 || (mode == 0 && fp16_ok && x->size >= FP16_AUTO_MIN_ROWS);       // the plain search's rule
    return use_fp16 ? search_grouped_fp16(x, d_queries, nq, k, groups, rows_out, dist)
                    : search_grouped_exact(x, d_queries, nq, k, groups, rows_out, dist);
}

// ---- distinct-moment search (knn_distinct.h) ----
// tests only, read per call: a prefix depth that replaces the plan's rule
int64_t distinct_depth_override() {
    const char* e = getenv("VQ_AMD_DISTINCT_DEPTH");
    return e ? std::max<long long>(0, atoll(e)) : 0;
}

// The plain search at the plan's depth -> the prefix walk; the queries it files are redone exactly, slice by slice: distances,
// the per-group walk, the plain selection, the scatter.  Nothing here waits for the stream.
int search_distinct_dispatch(vq_index* x, const float* d_queries, int nq, int k, int mode, int64_t min_gap, int32_t* d_ids, float* d_dist_out) {
    static const char* fn = "vq_index_search_distinct";
    VQ_TRY(check_mode(fn, mode));
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    VQ_TRY(check_positions(x, fn));
    const int64_t n = x->size, ld = round_up(n, 64);
    const DistinctPlan p = plan_distinct(n, nq, k, min_gap, mode, distinct_depth_override());
    const int D = (int)p.depth;
    const bool one_wg = n <= SEL_SMALL_MAX_N;
    const int nchunks = cdiv(n, SEL_CHUNK);
    VQ_TRY(x->d_dpre.reserve(2 * (int64_t)nq * D));
    VQ_TRY(x->d_dslots.reserve(nq));
    VQ_TRY(ensure_gcounters(x));
    if (p.slices) {
        VQ_TRY(x->d_dist.reserve(p.slice_q * ld));
        VQ_TRY(x->d_dsel.reserve(2 * p.slice_q * k));
        if (!one_wg) VQ_TRY(x->d_partial.reserve(p.slice_q * nchunks * k));
    }
    int32_t* pre_ids = x->d_dpre;
    float* pre_dist = (float*)(pre_ids + (int64_t)nq * D);
    VQ_HIP(hipMemsetAsync(x->d_gcounters, 0, 3 * sizeof(unsigned long long), x->stream));
    VQ_TRY(search_dispatch(x, d_queries, nq, D, mode, pre_ids, pre_dist));
    {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(distinct_prefix_kernel, dim3(nq), dim3(64), 0, x->stream, pre_ids, pre_dist, D, n, k, min_gap, x->d_group, x->d_pos,
                           d_ids, d_dist_out, x->d_dslots, x->d_gcounters);
    }
    const unsigned long long* cnt = x->d_gcounters;
    const unsigned long long* filed = cnt + DST_FILED;
    const int G = x->n_groups;
    for (int sl = 0; sl < p.slices; ++sl) {
        const int base = (int)(sl * p.slice_q), cap = (int)std::min<int64_t>(p.slice_q, nq - base);
        int32_t* sel_ids = x->d_dsel;
        float* sel_dist = (float*)(sel_ids + (int64_t)cap * k);
        {
            Prof pr(x, I_EXACT_DIST);
            hipLaunchKernelGGL(distinct_dist_kernel, dim3(std::min(cdiv(n, 64), DST_DIST_GRID), cdiv(cap, 32)), dim3(256), 0, x->stream, x->rows, n, x->dim, d_queries,
                               x->d_dslots, cnt, base, cap, x->d_dist, ld);
        }
        Prof pr(x, I_SELECT);
        if (min_gap > 0)
            hipLaunchKernelGGL(distinct_group_walk_kernel, dim3(std::max(1, std::min(cdiv(G, 4), 4096)), cap), dim3(256), 0, x->stream, x->d_dist, ld,
                               x->d_goff, x->d_grows, G, x->d_pos, x->tie(), k, min_gap, cnt, base, cap);
        if (one_wg) {
            hipLaunchKernelGGL(select_small_kernel, dim3(cap), dim3(256), 0, x->stream, x->d_dist, ld, n, k, sel_ids, sel_dist, x->tie(), filed, base);
        } else {
            hipLaunchKernelGGL(select_chunk_kernel, dim3(cap, nchunks), dim3(256), 0, x->stream, x->d_dist, ld, n, k, nchunks, x->d_partial, x->tie(),
                               filed, base);
            hipLaunchKernelGGL(merge_topk_kernel, dim3(cap), dim3(256), 0, x->stream, x->d_partial, nchunks, k, sel_ids, sel_dist, x->tie(), filed, base);
        }
        hipLaunchKernelGGL(distinct_scatter_kernel, dim3(cap), dim3(256), 0, x->stream, sel_ids, sel_dist, k, x->d_dslots, cnt, base, cap, d_ids,
                           d_dist_out);
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- diverse search (knn_diverse.h) ----
// tests only, read per call: a prefix depth that replaces the plan's rule
int64_t diverse_depth_override() {
    const char* e = getenv("VQ_AMD_DIVERSE_DEPTH");
    return e ? std::max<long long>(0, atoll(e)) : 0;
}

// The plain search at the plan's depth -> the pair pass -> the walk; the queries it files are redone exactly, slice by slice:
// distances once, then k rounds of pick (two levels) and suppress (the tile form and the row form are both queued; the filed
// count decides on the device which one works).  Nothing here waits for the stream.
int search_diverse_dispatch(vq_index* x, const float* d_queries, int nq, int k, int mode, float min_dist, int32_t* d_ids, float* d_dist_out) {
    static const char* fn = "vq_index_search_diverse";
    VQ_TRY(check_mode(fn, mode));
    VQ_TRY(check_ranks(x, fn));
    const int64_t n = x->size, ld = round_up(n, 64);
    const DiversePlan p = plan_diverse(n, nq, k, min_dist, mode, diverse_depth_override());
    const int D = (int)p.depth, W = cdiv(D, 64);
    const int nchunks = cdiv(n, DIV_PICK_CHUNK);
    VQ_TRY(x->d_dpre.reserve(2 * (int64_t)nq * D));
    VQ_TRY(x->d_dslots.reserve(nq));
    VQ_TRY(ensure_gcounters(x));
    if (p.pair_bytes) VQ_TRY(x->d_vbits.reserve(p.pair_bytes / 8));
    if (p.slices) {
        VQ_TRY(x->d_dist.reserve(p.slice_q * ld));
        VQ_TRY(x->d_vpart.reserve(p.slice_q * nchunks));
        VQ_TRY(x->d_vpick.reserve(p.slice_q));
    }
    int32_t* pre_ids = x->d_dpre;
    float* pre_dist = (float*)(pre_ids + (int64_t)nq * D);
    VQ_HIP(hipMemsetAsync(x->d_gcounters, 0, 3 * sizeof(unsigned long long), x->stream));
    VQ_TRY(search_dispatch(x, d_queries, nq, D, mode, pre_ids, pre_dist));
    if (p.pair_bytes) {
        Prof pr(x, I_EXACT_DIST);
        const int qmax = 32768;                                   // queries per launch (the grid's y extent)
        for (int q0 = 0; q0 < nq; q0 += qmax)
            hipLaunchKernelGGL(diverse_pair_kernel, dim3(W * cdiv(D, 32), std::min(qmax, nq - q0)), dim3(256), 0, x->stream, x->rows, n, x->dim,
                               pre_ids + (int64_t)q0 * D, D, W, min_dist, x->d_vbits + (int64_t)q0 * D * W);
    }
    {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(diverse_walk_kernel, dim3(nq), dim3(64), 0, x->stream, pre_ids, pre_dist, D, W, n, k,
                           p.pair_bytes ? x->d_vbits.p : nullptr, d_ids, d_dist_out, x->d_dslots, x->d_gcounters);
    }
    const unsigned long long* cnt = x->d_gcounters;
    for (int sl = 0; sl < p.slices; ++sl) {
        const int base = (int)(sl * p.slice_q), cap = (int)std::min<int64_t>(p.slice_q, nq - base);
        {
            Prof pr(x, I_EXACT_DIST);
            hipLaunchKernelGGL(distinct_dist_kernel, dim3(std::min(cdiv(n, 64), DST_DIST_GRID), cdiv(cap, 32)), dim3(256), 0, x->stream, x->rows, n, x->dim, d_queries,
                               x->d_dslots, cnt, base, cap, x->d_dist, ld);
        }
        for (int t = 0; t < k; ++t) {
            {
                Prof pr(x, I_SELECT);
                hipLaunchKernelGGL(diverse_pick_chunk_kernel, dim3(nchunks, cap), dim3(256), 0, x->stream, x->d_dist, ld, n, x->tie(), nchunks, x->d_vpart,
                                   cnt, base, cap);
                hipLaunchKernelGGL(diverse_pick_kernel, dim3(cap), dim3(256), 0, x->stream, x->d_vpart, nchunks, x->tie(), t, k, x->d_dslots, cnt, base, cap,
                                   x->d_vpick, d_ids, d_dist_out);
            }
            if (t + 1 == k) break;
            Prof pr(x, I_EXACT_DIST);
            hipLaunchKernelGGL(diverse_suppress_kernel, dim3(std::min(cdiv(n, 64), DST_DIST_GRID), cdiv(cap, 32)), dim3(256), 0, x->stream, x->rows, n, x->dim,
                               x->d_vpick, min_dist, cnt, base, cap, x->d_dist, ld);
            hipLaunchKernelGGL(diverse_suppress_rows_kernel, dim3(std::min(cdiv(n, SUM_THREADS), DST_DIST_GRID), std::min(cap, DIV_ROW_SLOTS)), dim3(SUM_THREADS),
                               (size_t)x->dim * 8, x->stream, x->rows, n, x->dim, x->d_vpick, min_dist, cnt, base, cap, x->d_dist, ld);
        }
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- vq_index_remove_rows (knn_remove.h) ----
// exclusive prefix sum of v[0..n) in place, v[n] = total; tiles holds cdiv(n, RM_SCAN_TILE) + 1 words
int rm_exclusive_scan(vq_index* x, int32_t* v, int64_t n, int32_t* tiles) {
    const int64_t ntiles = std::max<int64_t>(1, cdiv(n, RM_SCAN_TILE));
    hipLaunchKernelGGL(rm_scan_tile_sum_kernel, dim3((unsigned)ntiles), dim3(256), 0, x->stream, v, n, tiles);
    hipLaunchKernelGGL(rm_scan_carry_kernel, dim3(1), dim3(256), 0, x->stream, tiles, ntiles);
    hipLaunchKernelGGL(rm_scan_apply_kernel, dim3((unsigned)ntiles), dim3(256), 0, x->stream, v, n, tiles, ntiles);
    VQ_HIP(hipGetLastError());
    return 0;
}

// ---- filtered search (knn_filter.h) ----
struct FilterPlan {
    int64_t m = 0;                 // |S|: the allowed rows
    int32_t nA = 0;                // allowed groups
    bool all = false;              // an empty exclude list: S is the whole index
    int32_t* soff = nullptr;       // gather path: [nA + 1] list offsets of the allowed groups
    int32_t* list = nullptr;       // gather path: [m] the rows of S, group after group
    int32_t* tie_w = nullptr;      // gather path: [m] their tie words
    uint32_t* bits = nullptr;      // fp16 path: [cdiv(n_groups, 32)] the allowed groups' bitmap
};

// mode 0 takes the masked fp16 scan once S holds at least this share of the rows (measured, DESIGN.md "Filtered search"): the
// gather path reads 4 B x dim per allowed row, the masked scan 2 B x dim per row of every stream it does not skip plus its re-score
// (1M x 512: one query breaks even between 25 % and 60 % of the rows, 32 queries between 10 % and 25 %)
constexpr int FLT_CROSS_Q1_DEN = 2;       // batches of up to FLT_CROSS_FEW_Q queries: |S| >= n / 2
constexpr int FLT_CROSS_FEW_Q = 4;
constexpr int FLT_CROSS_QN_DEN = 5;       // larger batches: |S| >= n / 5

// the masked fp16 path exists for this call
bool filter_fp16_ok(const vq_index* x, int nq, int k) {
    return (x->dim == 256 || x->dim == 512 || x->dim == 768) && nq <= SCAN3_MAX_Q && k <= RV_K_MAX && x->size >= 1 && x->near_unit;
}

// Everything that can refuse a filtered call before any work is queued: the mode, and mode 2 where the masked path does not exist.
int filter_precheck(vq_index* x, const char* fn, int nq, int k, int mode, int32_t n_sel, int exclude) {
    VQ_TRY(check_mode(fn, mode));
    if (n_sel == 0 && exclude) return 0;                    // nothing excluded: the unfiltered search, under its own rules
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    if (mode == 2)
        VQ_CHECK(filter_fp16_ok(x, nq, k), "%s: the masked fp16 scan needs dim 256, 512 or 768, nq <= %d, k <= %d and near-unit rows "
                 "(0.5 <= |row|^2 <= 2); mode 1 takes any call", fn, SCAN3_MAX_Q, RV_K_MAX);
    return 0;
}

// A filter's labels, normalised once per call: sorted, a group named twice counted once; the rows they hold by the host mirror
// of goff (before any device work: the mode-0 choice needs |S| to pick what filter_prepare builds); and the first label, in the
// caller's order, that names no group.  Nothing is refused here: filter_prepare does that, behind the coverage checks.
struct FilterLabels {
    std::vector<int32_t> sel;
    int64_t in_rows = 0;
    bool bad = false; int32_t first_bad = 0;
    int64_t allowed_rows(const vq_index* x, int exclude) const { return exclude ? x->size - in_rows : in_rows; }
};
FilterLabels filter_labels(const vq_index* x, const int32_t* groups, int32_t n_sel) {
    FilterLabels f;
    for (int32_t i = 0; i < n_sel && !f.bad; ++i)
        if (groups[i] < 0 || groups[i] >= x->n_groups) { f.bad = true; f.first_bad = groups[i]; }
    f.sel.assign(groups, groups + n_sel);
    std::sort(f.sel.begin(), f.sel.end());
    f.sel.erase(std::unique(f.sel.begin(), f.sel.end()), f.sel.end());           // a group named twice counts once
    if (!f.bad && (int64_t)x->h_goff.size() == (int64_t)x->n_groups + 1)
        for (int32_t g : f.sel) f.in_rows += x->h_goff[(size_t)g + 1] - x->h_goff[(size_t)g];
    return f;
}
int check_label_range(const vq_index* x, const char* fn, const FilterLabels& f) {
    VQ_CHECK(!f.bad, "%s: group %d outside [0, %d)", fn, (int)f.first_bad, (int)x->n_groups);
    return 0;
}

// The next slot of the staging ring, holding at least `words`, free to be written: the copy that last read it has completed.
// The caller fills it, queues its copy and records the slot's event behind it.
int stage_slot(vq_index* x, int64_t words, StageSlot** out) {
    StageSlot& st = x->flt_stage[x->flt_slot];
    x->flt_slot = (x->flt_slot + 1) % vq_index::FLT_STAGE_SLOTS;
    if (st.ev) VQ_HIP(hipEventSynchronize(st.ev));
    else VQ_HIP(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    VQ_TRY(st.h.reserve(words, 16 << 10));
    *out = &st;
    return 0;
}

// Checks the labels and the filter.  Then, on the device, S's row list (gather path) or the allowed groups' bitmap (fp16 path).
// The list goes up from a ring of pinned staging slots: a slot is reused only after the copy vq_index::FLT_STAGE_SLOTS calls
// back has completed, so back-to-back asynchronous calls do not wait for each other.
int filter_prepare(vq_index* x, const char* fn, const FilterLabels& f, int exclude, bool fp16, FilterPlan* p) {
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    VQ_TRY(check_label_range(x, fn, f));
    const int32_t G = x->n_groups;
    const std::vector<int32_t>& sel = f.sel;
    const int32_t ns = (int32_t)sel.size();
    const int32_t* hg = x->h_goff.data();
    p->m = f.allowed_rows(x, exclude);
    p->nA = exclude ? G - ns : ns;
    p->all = exclude && ns == 0;
    if (p->all || p->m == 0) return 0;
    const int32_t nA = p->nA;
    const bool list = !fp16;
    auto words = [](int64_t c) { return round_up(std::max<int64_t>(c, 1), 4); };        // 16-byte aligned regions
    const int64_t w_A = words(nA), w_soff = words((int64_t)nA + 1), w_K = exclude && list ? words((int64_t)G + 1) : 0,
                  w_tiles = exclude && list ? words(cdiv(G, RM_SCAN_TILE) + 2) : 0, w_E = exclude ? words(ns) : 0,
                  w_list = list ? words(p->m) : 0, w_bits = fp16 ? words(cdiv(G, 32)) : 0;
    VQ_TRY(x->d_flt.reserve(w_A + w_soff + w_K + w_tiles + w_E + 2 * w_list + w_bits));
    int32_t* A = x->d_flt;
    p->soff = A + w_A;
    int32_t* K = p->soff + w_soff;
    int32_t* tiles = K + w_K;
    int32_t* E = tiles + w_tiles;
    p->list = list ? E + w_E : nullptr;
    p->tie_w = list ? E + w_E + w_list : nullptr;
    p->bits = fp16 ? (uint32_t*)(E + w_E + 2 * w_list) : nullptr;
    StageSlot* slot;
    VQ_TRY(stage_slot(x, exclude ? ns : w_A + nA + 1, &slot));
    StageSlot& st = *slot;
    int32_t* h = st.h;
    if (!exclude) {
        // the include list is the allowed groups: A and their offsets go up in one copy
        std::memcpy(h, sel.data(), (size_t)nA * 4);
        int32_t* so = h + w_A;
        int32_t run = 0;
        for (int32_t j = 0; j < nA; ++j) { so[j] = run; run += hg[sel[(size_t)j] + 1] - hg[sel[(size_t)j]]; }
        so[nA] = run;
        VQ_HIP(hipMemcpyAsync(A, h, (size_t)(w_A + nA + 1) * 4, hipMemcpyHostToDevice, x->stream));
    } else {
        std::memcpy(h, sel.data(), (size_t)ns * 4);        // ns > 0: an empty exclude list is the unfiltered search
        VQ_HIP(hipMemcpyAsync(E, h, (size_t)ns * 4, hipMemcpyHostToDevice, x->stream));
    }
    VQ_HIP(hipEventRecord(st.ev, x->stream));
    if (fp16) {
        VQ_HIP(hipMemsetAsync(p->bits, exclude ? 0xff : 0, (size_t)w_bits * 4, x->stream));
        hipLaunchKernelGGL(filter_bitmap_kernel, dim3(grid_for(ns)), dim3(256), 0, x->stream, exclude ? E : A, ns, p->bits);
    } else {
        if (exclude) {
            hipLaunchKernelGGL(filter_allowed_kernel, dim3(grid_for(G)), dim3(256), 0, x->stream, E, ns, G, K);
            VQ_TRY(rm_exclusive_scan(x, K, G, tiles));
            hipLaunchKernelGGL(filter_compact_groups_kernel, dim3(grid_for(G)), dim3(256), 0, x->stream, K, G, x->d_goff, A, p->soff);
            VQ_TRY(rm_exclusive_scan(x, p->soff, nA, tiles));
        }
        hipLaunchKernelGGL(filter_expand_kernel, dim3((unsigned)std::min<int64_t>(cdiv(nA, 4), 4096)), dim3(256), 0, x->stream, A, p->soff, nA,
                           x->d_goff, x->d_grows, x->tie(), p->list, p->tie_w);
    }
    VQ_HIP(hipGetLastError());
    return 0;
}

// distances of the listed rows for queries [0, cur) of a slice
void filter_dist(vq_index* x, const FilterPlan& p, const float* qp, int cur, int64_t ld) {
    Prof pr(x, I_EXACT_DIST);
    if (cur <= 8)
        hipLaunchKernelGGL(filter_dist_kernel<8>, dim3(cdiv(p.m, 64), 1), dim3(256), 0, x->stream, x->rows, p.list, p.m, x->dim, qp, cur, x->d_dist, ld);
    else
        hipLaunchKernelGGL(filter_dist_kernel<32>, dim3(cdiv(p.m, 64), cdiv(cur, 32)), dim3(256), 0, x->stream, x->rows, p.list, p.m, x->dim,
                           qp, cur, x->d_dist, ld);
}

// the gather paths' tie order: the list positions' tie words
TieOrder list_tie(const vq_index* x, const FilterPlan& p) { return TieOrder{p.tie_w, x->rank_n ? x->d_rank_inv : nullptr}; }

// Gather path, plain form: the plain exact path's selection over the list positions (knn_filter.h 4.)
int search_filtered_gather(vq_index* x, const float* d_queries, int nq, int k, const FilterPlan& p, int32_t* d_ids, float* d_dist_out) {
    return exact_topk(x, p.m, nq, k, p.m <= SEL_SMALL_MAX_N, list_tie(x, p), d_ids, d_dist_out, [&](int q0, int cur, int64_t ld) {
        filter_dist(x, p, d_queries + (int64_t)q0 * x->dim, cur, ld);
        return 0;
    });
}

// Gather path, grouped form: group minima over the allowed groups' list ranges -> block top-k -> group_merge_kernel
int search_grouped_filtered_gather(vq_index* x, const float* d_queries, int nq, int k, const FilterPlan& p, int32_t* groups,
                                   int32_t* rows_out, float* dist) {
    return grouped_exact_topk(x, group_block_topk_kernel<true, false, true>, p.m, p.nA, p.soff, nullptr, list_tie(x, p), nq, k, groups, rows_out, dist,
                              [&](int64_t q0, int cur, int64_t ld) { filter_dist(x, p, d_queries + q0 * x->dim, cur, ld); return 0; });
}

// Masked fp16 path, plain form (knn_filter.h): masked stream scan -> stream threshold -> re-score of the candidate streams'
// allowed rows -> top-k; flagged queries are redone by the masked exact fallback on the device, so nothing here waits.
int search_filtered_fp16(vq_index* x, const float* d_queries, int nq, int k, const FilterPlan& p, int32_t* d_ids, float* d_dist_out) {
    const int64_t n = x->size, streams = round_up(n, SCAN_STREAM_ROWS) / SCAN_STREAM_ROWS, q_pad = round_up(nq, SCAN3_QB);
    VQ_TRY(x->d_q16.reserve(q_pad * x->dim));
    VQ_TRY(x->d_keys.reserve(streams * q_pad * 2));
    VQ_TRY(x->d_flags.reserve(q_pad));
    VQ_TRY(x->d_fcand.reserve((int64_t)nq * FLT_CAND + 3 * (int64_t)nq));
    VQ_TRY(x->d_flist.reserve((int64_t)nq * FLT_LIST));
    VQ_TRY(reserve_fallback(x, nq, k));
    int32_t* cand = x->d_fcand;
    int32_t* cn = cand + (int64_t)nq * FLT_CAND;
    int32_t* ln = cn + nq;
    float* thr = (float*)(ln + nq);
    const GroupMask gm{x->d_group, x->d_sgroup, p.bits};
    x->last_scan.valid = false;
    queries_to_f16(x, d_queries, nq, q_pad);
    {
        Prof pr(x, I_MFMA_SCAN);
        hipLaunchKernelGGL((scan3_instance<false, true>(x->dim, 1)), dim3(cdiv(streams, 4), (int)(q_pad / SCAN3_QB)), dim3(256), 0, x->stream, x->d_q16, x->rows16, n, streams, q_pad,
                           x->d_keys, 0, gm);
    }
    x->last_scan = {true, true, 3, nq, streams, 0};
    {
        Prof pr(x, I_RESCORE);
        const TieOrder tie = x->tie();
        hipLaunchKernelGGL(filter_stream_threshold_kernel, dim3(nq), dim3(256), 0, x->stream, x->d_keys, streams, k, d_queries, x->dim,
                           scan_eps_unit(x->dim) * x->row_norm_max, cand, cn, thr, ln, x->d_flags);
        hipLaunchKernelGGL(filter_stream_rescore_kernel, dim3(FLT_RESCORE_SPLITS, nq), dim3(256), 0, x->stream, x->d_q16, d_queries, x->rows,
                           x->rows16, n, x->dim, gm, cand, cn, thr, x->d_flags, x->d_flist, ln, tie);
        hipLaunchKernelGGL(filter_stream_finalize_kernel, dim3(nq), dim3(256), 0, x->stream, x->d_flist, ln, k, p.m, x->d_flags, d_ids,
                           d_dist_out, tie);
    }
    hipLaunchKernelGGL(collect_flags_kernel, dim3(1), dim3(1024), 0, x->stream, x->d_flags, nq, x->d_slots, x->d_counters);
    launch_fallback(x, d_queries, nq, k, d_ids, d_dist_out, x->d_counters, &gm);
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_counters, x->d_counters, FB_NCOUNTERS * 4, hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_COUNTERS);
    return 0;
}

// mode 0: the masked fp16 scan where it exists, the index is large enough for the plain rule (FP16_AUTO_MIN_ROWS) and S is broad
bool filter_use_fp16(const vq_index* x, int nq, int k, int mode, int64_t m) {
    if (mode != 0) return mode == 2;
    const int den = nq <= FLT_CROSS_FEW_Q ? FLT_CROSS_Q1_DEN : FLT_CROSS_QN_DEN;
    return filter_fp16_ok(x, nq, k) && x->size >= FP16_AUTO_MIN_ROWS && m * den >= x->size;
}

int search_filtered_dispatch(vq_index* x, const float* d_queries, int nq, int k, int mode, const int32_t* sel, int32_t n_sel, int exclude,
                             int32_t* d_ids, float* d_dist) {
    static const char* fn = "vq_index_search_filtered";
    VQ_TRY(filter_precheck(x, fn, nq, k, mode, n_sel, exclude));
    if (n_sel == 0 && exclude) return search_dispatch(x, d_queries, nq, k, mode, d_ids, d_dist);       // nothing excluded: the plain search
    const FilterLabels f = filter_labels(x, sel, n_sel);
    const bool fp16 = filter_use_fp16(x, nq, k, mode, f.allowed_rows(x, exclude));
    FilterPlan p;
    VQ_TRY(filter_prepare(x, fn, f, exclude, fp16, &p));
    if (p.m == 0) {                                         // S is empty: no result for any query
        set_stats(x, STATS_HOST, 0, 0, nq);
        return fill_empty(x, (int64_t)nq * k, d_ids, nullptr, d_dist);
    }
    return fp16 ? search_filtered_fp16(x, d_queries, nq, k, p, d_ids, d_dist) : search_filtered_gather(x, d_queries, nq, k, p, d_ids, d_dist);
}

int search_grouped_filtered_dispatch(vq_index* x, const float* d_queries, int nq, int k, int mode, const int32_t* sel, int32_t n_sel,
                                     int exclude, int32_t* groups, int32_t* rows_out, float* dist) {
    static const char* fn = "vq_index_search_grouped_filtered";
    VQ_TRY(filter_precheck(x, fn, nq, k, mode, n_sel, exclude));
    if (n_sel == 0 && exclude) return search_grouped_dispatch(x, d_queries, nq, k, mode, groups, rows_out, dist);
    const FilterLabels f = filter_labels(x, sel, n_sel);
    const bool fp16 = filter_use_fp16(x, nq, k, mode, f.allowed_rows(x, exclude));
    FilterPlan p;
    VQ_TRY(filter_prepare(x, fn, f, exclude, fp16, &p));
    if (p.m == 0) {
        set_stats(x, STATS_HOST, 0, 0, nq);
        return fill_empty(x, (int64_t)nq * k, groups, rows_out, dist);
    }
    return fp16 ? search_grouped_fp16(x, d_queries, nq, k, groups, rows_out, dist, p.bits, p.nA)
                : search_grouped_filtered_gather(x, d_queries, nq, k, p, groups, rows_out, dist);
}

// ---- clip search (knn_set.h) ----
bool set_fp16_ok(const vq_index* x) { return scan_fp16_dim(x->dim) && x->size >= 1 && x->near_unit; }

// Everything that can refuse a clip search before any work is queued: the mode, stale ranks or labels, the filter's labels, and
// mode 2 where the fp16 path does not exist.
int set_precheck(vq_index* x, const char* fn, int mode, const FilterLabels& f) {
    VQ_TRY(check_mode(fn, mode));
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    VQ_TRY(check_label_range(x, fn, f));
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    if (mode == 2) VQ_CHECK(set_fp16_ok(x), "%s: the fp16 path needs dim 256, 512 or 768 and near-unit rows (0.5 <= |row|^2 <= 2; rows "
                                            "added with normalize=0 are measured); mode 1 takes any call", fn);
    return 0;
}

// d_queries [m][dim]; o: groups / distances [k], match rows [k][m] or not asked for, placed in device memory.  Asynchronous on
// the index's stream.
int search_set_run(vq_index* x, const char* fn, const float* d_queries, int m, int k, int mode, const FilterLabels& f, int exclude,
                   const Outs& o) {
    int32_t* const g_out = o.dev<int32_t>(0); float* const d_out = o.dev<float>(1); int32_t* const match = o.dev<int32_t>(2);
    FilterPlan p;
    VQ_TRY(filter_prepare(x, fn, f, exclude, true, &p));
    if (!p.all && p.m == 0) {                               // nothing allowed: every slot empty
        set_stats(x, STATS_HOST, 0, 0, 1);
        return outs_empty_placed(x, o);
    }
    const uint32_t* allow = p.all ? nullptr : p.bits;
    const int64_t n = x->size, ld = round_up(n, 64);
    const int G = x->n_groups, nA = p.all ? G : p.nA;
    const int nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK), lpg = lanes_per_group(n, G);
    const bool use_fp16 = mode == 2 || (mode == 0 && set_fp16_ok(x) && x->size >= FP16_AUTO_MIN_ROWS);     // the plain search's rule
    VQ_TRY(x->d_ssum.reserve(2 * (int64_t)G));
    VQ_TRY(x->d_scand.reserve(3 * (int64_t)G + 2));
    VQ_TRY(x->d_sekey.reserve((int64_t)G + (int64_t)nblocks * kl));
    double* sum16 = x->d_ssum; double* acc = sum16 + G;
    int32_t* cand = x->d_scand; int32_t* candpos = cand + G; int32_t* cand_n = candpos + G; int32_t* flag = cand_n + 1;
    uint32_t* skey = (uint32_t*)(flag + 1);                 // set_threshold_kernel's [G] scratch: d_gbest keeps the last chunk's maxima
    uint64_t* ekey = x->d_sekey; uint64_t* partial = ekey + G;
    const TieOrder tie = x->tie();

    // the exact path; fl = null: the call's answer (distances from the tiled kernel), else the redo gated by the flag
    auto run_exact = [&](const int32_t* fl) -> int {
        const bool from_dist = fl == nullptr;
        int64_t qs = std::max<int64_t>(1, std::min<int64_t>(m, ((int64_t)32 << 20) / G));                 // group minima: <= 256 MiB
        if (from_dist) qs = std::max<int64_t>(1, std::min<int64_t>(qs, ((int64_t)128 << 20) / ld));         // distances: <= 512 MiB
        VQ_TRY(x->d_gkeys.reserve(qs * G));
        if (from_dist) VQ_TRY(x->d_dist.reserve(qs * ld));
        auto gmin = from_dist ? (allow ? set_group_min_kernel<true, true> : set_group_min_kernel<true, false>)
                              : (allow ? set_group_min_kernel<false, true> : set_group_min_kernel<false, false>);
        for (int64_t q0 = 0; q0 < m; q0 += qs) {
            const int cur = (int)std::min<int64_t>(qs, m - q0);
            const float* qp = d_queries + q0 * x->dim;
            if (from_dist) VQ_TRY(exact_dist(x, false, qp, cur, ld));      // always the tiled kernel
            Prof pr(x, from_dist ? I_SELECT : I_EXACT_DIST);
            hipLaunchKernelGGL(gmin, dim3(nblocks, cur), dim3(256), 0, x->stream, x->d_dist, ld, x->rows, x->dim, qp, x->d_goff, x->d_grows, G, lpg,
                               x->d_gkeys, fl, tie, allow);
            hipLaunchKernelGGL(set_accum_dist_kernel, dim3(nblocks), dim3(256), 0, x->stream, x->d_gkeys, cur, G, q0 == 0 ? 1 : 0, acc, fl);
        }
        hipLaunchKernelGGL(set_final_exact_kernel, dim3(nblocks), dim3(256), 0, x->stream, acc, G, m, allow, ekey, fl);
        VQ_HIP(hipGetLastError());
        return 0;
    };

    if (!use_fp16) {
        VQ_TRY(run_exact(nullptr));
    } else {
        const int64_t streams = cdiv(n, SCAN_STREAM_ROWS);
        int64_t qc = std::max<int64_t>(16, ((int64_t)64 << 20) / G / 16 * 16);          // gbest [qc][G]: <= 256 MiB
        qc = std::min<int64_t>(qc, round_up(m, 16));
        if (qc >= SCAN2_QT) qc = qc / SCAN2_QT * SCAN2_QT;                              // whole query tiles of the batch mainloop
        VQ_TRY(x->d_q16.reserve(round_up(qc, SCAN2_QT) * x->dim));
        VQ_TRY(x->d_gbest.reserve(qc * G));
        x->last_gscan.valid = false;                        // the clip search's maxima take the grouped search's buffer
        VQ_TRY(x->d_sqn.reserve(m));
        VQ_TRY(x->d_sckeys.reserve(std::min<int64_t>(SET_KEY_BUDGET, (int64_t)G * m)));
        VQ_TRY(ensure_gcounters(x));
        VQ_TRY(set_dyn_lds(x, (const void*)set_group_max_kernel<false>, G2_LDS_BYTES));
        VQ_TRY(set_dyn_lds(x, (const void*)set_group_max_kernel<true>, G2_LDS_BYTES));
        VQ_HIP(hipMemsetAsync(x->d_gcounters, 0, 3 * sizeof(unsigned long long), x->stream));
        VQ_HIP(hipMemsetAsync(cand_n, 0, 8, x->stream));                                 // candidate count and the call's flag
        hipLaunchKernelGGL(set_query_norm_kernel, dim3(m), dim3(64), 0, x->stream, d_queries, x->dim, x->d_sqn, flag);
        const int ranges = cdiv(n, SCAN2_RANGE), range_groups = cdiv(ranges, 4);
        int chunks = 0, tile_chunks = 0;
        for (int64_t q0 = 0; q0 < m; q0 += qc) {
            const int cur = (int)std::min<int64_t>(qc, m - q0);
            const bool small = cur <= 16;                   // the streaming group-max scan of the grouped search
            ++chunks; tile_chunks += small ? 0 : 1;
            x->last_gscan = {true, cur, (int32_t)G, q0, small ? 2 : 3, chunks, tile_chunks};     // nothing behind the scan writes d_gbest
            const int64_t q_pad = round_up(cur, small ? 16 : SCAN2_QT);
            queries_to_f16(x, d_queries + q0 * x->dim, cur, q_pad);
            VQ_HIP(hipMemsetAsync(x->d_gbest, 0, (size_t)cur * G * 4, x->stream));
            {
                Prof pr(x, I_MFMA_SCAN);
                if (small) {
                    auto scan = scan3_group_max(x->dim, allow != nullptr);
                    hipLaunchKernelGGL(scan, dim3(cdiv(streams, 4), 1), dim3(256), 0, x->stream, x->d_q16, x->rows16, streams, x->d_group, x->d_sgroup,
                                       cur, G, x->d_gbest, allow);
                } else {
                    const int q_tiles = (int)(q_pad / SCAN2_QT), q_groups = cdiv(q_tiles, 8);
                    hipLaunchKernelGGL(allow ? set_group_max_kernel<true> : set_group_max_kernel<false>, dim3(range_groups * q_groups * 32), dim3(G2_THREADS),
                                       G2_LDS_BYTES, x->stream, x->d_q16, x->rows16, x->dim, streams, q_tiles, ranges, range_groups, x->d_group, x->d_sgroup,
                                       cur, G, x->d_gbest, allow);
                }
            }
            Prof pr(x, I_RESCORE);
            hipLaunchKernelGGL(set_accum_score_kernel, dim3(nblocks), dim3(256), 0, x->stream, x->d_gbest, cur, G, q0 == 0 ? 1 : 0, sum16);
        }
        {
            Prof pr(x, I_RESCORE);
            const int nsub = 256 / lpg;
            hipLaunchKernelGGL(set_threshold_kernel, dim3(1), dim3(256), 0, x->stream, sum16, G, m, std::min(k, nA), nA, allow, x->d_sqn,
                               scan_eps_unit(x->dim) * x->row_norm_max, x->d_goff, skey, cand, candpos, cand_n, ekey, flag, x->d_gcounters);
            hipLaunchKernelGGL(set_cand_keys_kernel, dim3(std::min(cdiv(G, nsub), 64), m), dim3(256), 0, x->stream, x->rows, x->dim, d_queries, m,
                               x->d_goff, x->d_grows, cand, cand_n, lpg, x->d_sckeys, flag, tie);
            hipLaunchKernelGGL(set_cand_sum_kernel, dim3(std::min(nblocks, 256)), dim3(256), 0, x->stream, x->d_sckeys, m, cand, cand_n, ekey, flag);
        }
        VQ_HIP(hipGetLastError());
        VQ_TRY(run_exact(flag));                            // every kernel of it leaves at once unless the flag is 2
    }
    {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(set_select_block_kernel, dim3(nblocks), dim3(256), 0, x->stream, ekey, G, kl, partial);
        hipLaunchKernelGGL(set_select_merge_kernel, dim3(1), dim3(256), 0, x->stream, partial, (int64_t)nblocks * kl, k, g_out, d_out,
                           use_fp16 ? flag : nullptr, use_fp16 ? x->d_gcounters.p : nullptr);
        if (match)
            hipLaunchKernelGGL(set_match_rows_kernel, dim3(k, std::min(cdiv(m, 4), 64)), dim3(256), 0, x->stream, g_out, m, x->rows, x->dim, d_queries,
                               x->d_goff, x->d_grows, candpos, x->d_sckeys, use_fp16 ? flag : nullptr, match, tie);
    }
    VQ_HIP(hipGetLastError());
    if (use_fp16) {
        VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
        set_stats(x, STATS_GCOUNTERS);
    } else {
        set_stats(x, STATS_HOST, 0, 0, 1);
    }
    return 0;
}

// ---- sequence search (knn_sequence.h) ----
// tests only, read per call: the LDS form's row limit, the distance budget and the back-pointer budget in bytes
int64_t seq_env(const char* name) {
    const char* e = getenv(name);
    return e ? std::max<long long>(0, atoll(e)) : 0;
}
SequencePlan seq_plan_env(int64_t n, int64_t largest_group, int m) {
    return plan_sequence(n, largest_group, m, seq_env("VQ_AMD_SEQ_LDS_ROWS"), seq_env("VQ_AMD_SEQ_DIST_BYTES"), seq_env("VQ_AMD_SEQ_BP_BYTES"));
}

// Every group's rows in (position, tie) order, with the positions and ties in that order: sorted on the host from the by-group
// row list, the positions and the id ranks as the device holds them, and uploaded.  Blocks on the stream; runs once after the
// labels, the positions or the ranks changed.
int seq_order_prepare(vq_index* x) {
    if (x->seq_n == x->size) return 0;
    const int64_t n = x->size;
    const int32_t G = x->n_groups;
    std::vector<int32_t> grows((size_t)n), pos((size_t)n), rank;
    std::vector<int32_t> h((size_t)(3 * n));
    StreamDrain drain{x->stream};
    VQ_HIP(hipMemcpyAsync(grows.data(), x->d_grows, (size_t)n * 4, hipMemcpyDeviceToHost, x->stream));
    VQ_HIP(hipMemcpyAsync(pos.data(), x->d_pos, (size_t)n * 4, hipMemcpyDeviceToHost, x->stream));
    if (x->rank_n) {
        rank.resize((size_t)n);
        VQ_HIP(hipMemcpyAsync(rank.data(), x->d_rank, (size_t)n * 4, hipMemcpyDeviceToHost, x->stream));
    }
    VQ_HIP(hipStreamSynchronize(x->stream));
    const int32_t* rk = x->rank_n ? rank.data() : nullptr;
    int64_t largest = 0;
    for (int32_t g = 0; g < G; ++g) {
        int32_t* b = grows.data() + x->h_goff[(size_t)g], *e = grows.data() + x->h_goff[(size_t)g + 1];
        largest = std::max<int64_t>(largest, e - b);
        std::sort(b, e, [&](int32_t a, int32_t c) {
            if (pos[(size_t)a] != pos[(size_t)c]) return pos[(size_t)a] < pos[(size_t)c];
            return rk ? rk[a] < rk[c] : a < c;
        });
    }
    int32_t* so = h.data(); int32_t* sp = so + n; int32_t* st = sp + n;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = grows[(size_t)i];
        so[i] = r; sp[i] = pos[(size_t)r]; st[i] = rk ? rk[r] : r;
    }
    VQ_TRY(x->d_seq.reserve(3 * std::max<int64_t>(n, x->cap)));
    VQ_HIP(hipMemcpyAsync(x->d_seq, h.data(), (size_t)n * 12, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));
    x->seq_n = n; x->seq_largest = largest;
    return 0;
}

// Everything that can refuse a sequence search before any work is queued.
int seq_precheck(vq_index* x, const char* fn, const FilterLabels& f) {
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    VQ_TRY(check_positions(x, fn));
    return check_label_range(x, fn, f);
}

// d_steps [m][dim]; o: groups / distances [k], chain rows [k][m] or not asked for, placed in device memory.  Asynchronous on
// the index's stream once the (position, tie) order is on the device.
int search_sequence_run(vq_index* x, const char* fn, const float* d_steps, int m, int k, int64_t min_gap, int64_t max_gap,
                        const FilterLabels& f, int exclude, const Outs& o) {
    int32_t* const g_out = o.dev<int32_t>(0); float* const d_out = o.dev<float>(1); int32_t* const chain = o.dev<int32_t>(2);
    FilterPlan fp;
    VQ_TRY(filter_prepare(x, fn, f, exclude, true, &fp));
    if (!fp.all && fp.m == 0) {                             // nothing allowed: every slot empty
        set_stats(x, STATS_HOST, 0, 0, 0);
        return outs_empty_placed(x, o);
    }
    VQ_TRY(seq_order_prepare(x));
    const uint32_t* allow = fp.all ? nullptr : fp.bits;
    const int64_t n = x->size, ld = round_up(n, 64);
    const int G = x->n_groups;
    const int nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK);
    const SequencePlan p = seq_plan_env(n, x->seq_largest, m);
    // positions are 32-bit: a gap of 2^32 or more behaves as 2^32, and the differences below stay far inside 64 bits
    const int64_t gap_cap = (int64_t)1 << 32;
    min_gap = std::min(min_gap, gap_cap); max_gap = std::min(max_gap, gap_cap);
    // the allowed groups the global form runs (the host mirror of goff and the sorted filter list)
    int64_t global_groups = 0;
    if (p.global_form) {
        size_t si = 0;
        for (int32_t g = 0; g < G; ++g) {
            while (si < f.sel.size() && f.sel[si] < g) ++si;
            const bool listed = si < f.sel.size() && f.sel[si] == g;
            if ((exclude ? !listed : listed) && x->h_goff[(size_t)g + 1] - x->h_goff[(size_t)g] > p.lds_rows) ++global_groups;
        }
    }
    const bool table = chain && p.bp_table && m > 1, redo = chain && !p.bp_table && m > 1;
    VQ_TRY(x->d_dist.reserve((int64_t)p.chunk_steps * ld));
    VQ_TRY(x->d_seqc.reserve(3 * n));
    VQ_TRY(x->d_seqw.reserve(3 * n + G));
    VQ_TRY(x->d_sekey.reserve((int64_t)G + (int64_t)nblocks * kl));
    VQ_TRY(ensure_gcounters(x));
    if (table) VQ_TRY(x->d_seqbp.reserve((int64_t)(m - 1) * n));
    if (redo) VQ_TRY(x->d_seqbp.reserve((int64_t)p.bp_slice_steps * n));
    VQ_TRY(set_dyn_lds(x, (const void*)seq_dp_lds_kernel, (size_t)p.lds_bytes));
    const int32_t* sorder = x->d_seq; const int32_t* spos = sorder + n; const int32_t* stie = spos + n;
    uint64_t* carry = x->d_seqc; uint64_t* cost = carry + n;
    int32_t* work = x->d_seqw; int32_t* end_idx = work + 3 * n;
    uint64_t* ekey = x->d_sekey; uint64_t* partial = ekey + G;
    int32_t* bp = table ? x->d_seqbp.p : nullptr;
    for (int j0 = 0; j0 < m; j0 += p.chunk_steps) {
        const int cur = std::min(p.chunk_steps, m - j0);
        VQ_TRY(exact_dist(x, false, d_steps + (int64_t)j0 * x->dim, cur, ld));         // always the tiled kernel
        Prof pr(x, I_SEQ_DP);
        hipLaunchKernelGGL(seq_dp_lds_kernel, dim3(G), dim3(SEQ_THREADS), (size_t)p.lds_bytes, x->stream, x->d_dist, ld, j0, cur, x->d_goff, sorder,
                           spos, stie, p.lds_rows, p.lds_alloc_rows, min_gap, max_gap, carry, bp, n, m, allow);
        if (p.global_form)
            hipLaunchKernelGGL(seq_dp_global_kernel, dim3(G), dim3(SEQ_THREADS), 0, x->stream, x->d_dist, ld, j0, cur, x->d_goff, sorder, spos, stie,
                               p.lds_rows, min_gap, max_gap, carry, work, cost, bp, n, m, allow);
    }
    {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(seq_final_kernel, dim3(G), dim3(SEQ_THREADS), 0, x->stream, carry, x->d_goff, stie, m, allow, ekey, end_idx);
        hipLaunchKernelGGL(set_select_block_kernel, dim3(nblocks), dim3(256), 0, x->stream, ekey, G, kl, partial);
        hipLaunchKernelGGL(set_select_merge_kernel, dim3(1), dim3(256), 0, x->stream, partial, (int64_t)nblocks * kl, k, g_out, d_out, nullptr,
                           nullptr);
        hipLaunchKernelGGL(seq_stats_kernel, dim3(1), dim3(256), 0, x->stream, ekey, G, (unsigned long long)global_groups,
                           (unsigned long long)p.step_chunks, x->d_gcounters);
    }
    if (chain) {
        Prof pr(x, I_SEQ_DP);
        if (m == 1 || table)
            hipLaunchKernelGGL(seq_trace_kernel, dim3(cdiv(k, 64)), dim3(64), 0, x->stream, g_out, k, m, x->d_goff, sorder, end_idx, bp, n, chain);
        else
            hipLaunchKernelGGL(seq_chain_redo_kernel, dim3(k), dim3(SEQ_THREADS), 0, x->stream, g_out, m, p.bp_slice_steps, x->rows, x->dim, d_steps,
                               x->d_goff, sorder, spos, stie, min_gap, max_gap, end_idx, work, cost, x->d_seqbp, n, chain);
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- span search (knn_span.h) ----
// tests only, read per call: the LDS form's row limit and the distance budget in bytes
SpanPlan span_plan_env(int64_t n, int64_t n_groups, int64_t largest_group, int nq) {
    return plan_spans(n, n_groups, largest_group, nq, seq_env("VQ_AMD_SPAN_LDS_ROWS"), seq_env("VQ_AMD_SPAN_DIST_BYTES"));
}

// d_queries [nq][dim]; o: groups / distances [nq][k], then masses, lengths [nq][k] and rows [nq][k][3], each or not asked for,
// placed in device memory.  Asynchronous on the index's stream once the (position, tie) order is on the device.
int search_spans_run(vq_index* x, const char* fn, const float* d_queries, int nq, int k, float tau, int64_t max_gap, int64_t max_span,
                     const FilterLabels& f, int exclude, const Outs& o) {
    int32_t* const g_out = o.dev<int32_t>(0); float* const d_out = o.dev<float>(1);
    int64_t* const mass = o.dev<int64_t>(2); int32_t* const len = o.dev<int32_t>(3); int32_t* const rows = o.dev<int32_t>(4);
    FilterPlan fp;
    VQ_TRY(filter_prepare(x, fn, f, exclude, true, &fp));
    if (!fp.all && fp.m == 0) {                             // nothing allowed: every slot empty
        set_stats(x, STATS_HOST, 0, 0, 0);
        return outs_empty_placed(x, o);
    }
    VQ_TRY(seq_order_prepare(x));
    const uint32_t* allow = fp.all ? nullptr : fp.bits;
    const int64_t n = x->size, ld = round_up(n, 64);
    const int G = x->n_groups;
    const int nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK);
    const SpanPlan p = span_plan_env(n, G, x->seq_largest, nq);
    // positions are 32-bit: a limit of 2^32 or more behaves as 2^32 ("none"), and the differences stay far inside 64 bits
    const int64_t cap = (int64_t)1 << 32;
    max_gap = std::min(max_gap, cap); max_span = std::min(max_span, cap);
    // the allowed groups the global form runs (the host mirror of goff and the sorted filter list)
    int64_t global_groups = 0;
    if (p.global_form) {
        size_t si = 0;
        for (int32_t g = 0; g < G; ++g) {
            while (si < f.sel.size() && f.sel[si] < g) ++si;
            const bool listed = si < f.sel.size() && f.sel[si] == g;
            if ((exclude ? !listed : listed) && x->h_goff[(size_t)g + 1] - x->h_goff[(size_t)g] > p.lds_rows) ++global_groups;
        }
    }
    const int64_t pairs = (int64_t)p.chunk_queries * G;
    VQ_TRY(x->d_dist.reserve((int64_t)p.chunk_queries * ld));
    VQ_TRY(x->d_sekey.reserve(pairs + (int64_t)nblocks * kl));
    VQ_TRY(x->d_spanw.reserve(2 * pairs + (p.global_form ? 3 * n : 0)));
    if (p.global_form) VQ_TRY(x->d_spanp.reserve(n + G));
    VQ_TRY(ensure_gcounters(x));
    VQ_TRY(set_dyn_lds(x, (const void*)span_lds_kernel, (size_t)p.lds_bytes));
    const int32_t* sorder = x->d_seq; const int32_t* spos = sorder + n; const int32_t* stie = spos + n;
    uint64_t* ekey = x->d_sekey; uint64_t* partial = ekey + pairs;
    int32_t* ab = x->d_spanw; int32_t* work = ab + 2 * pairs;
    const bool finish = mass || len || rows;
    for (int q0 = 0; q0 < nq; q0 += p.chunk_queries) {
        const int cur = std::min(p.chunk_queries, nq - q0);
        const int64_t at = (int64_t)q0 * k;
        VQ_TRY(exact_dist(x, false, d_queries + (int64_t)q0 * x->dim, cur, ld));       // always the tiled kernel
        {
            Prof pr(x, I_SEQ_DP);
            hipLaunchKernelGGL(span_lds_kernel, dim3(G, cur), dim3(SPAN_THREADS), (size_t)p.lds_bytes, x->stream, x->d_dist, ld, x->d_goff, sorder,
                               spos, p.lds_rows, p.lds_alloc_rows, tau, max_gap, max_span, G, allow, ekey, ab);
            if (p.global_form)
                hipLaunchKernelGGL(span_global_kernel, dim3(G), dim3(SPAN_THREADS), 0, x->stream, x->d_dist, ld, cur, x->d_goff, sorder, spos,
                                   p.lds_rows, tau, max_gap, max_span, G, allow, x->d_spanp.p, work, n, ekey, ab);
        }
        {
            Prof pr(x, I_SELECT);
            for (int q = 0; q < cur; ++q) {
                hipLaunchKernelGGL(set_select_block_kernel, dim3(nblocks), dim3(256), 0, x->stream, ekey + (int64_t)q * G, G, kl, partial);
                hipLaunchKernelGGL(set_select_merge_kernel, dim3(1), dim3(256), 0, x->stream, partial, (int64_t)nblocks * kl, k,
                                   g_out + at + (int64_t)q * k, d_out + at + (int64_t)q * k, nullptr, nullptr);
            }
            hipLaunchKernelGGL(span_stats_kernel, dim3(1), dim3(256), 0, x->stream, ekey, (int64_t)cur * G, q0 == 0 ? 1 : 0,
                               (unsigned long long)global_groups, (unsigned long long)p.query_chunks, x->d_gcounters);
        }
        if (finish) {
            Prof pr(x, I_SEQ_DP);
            hipLaunchKernelGGL(span_finish_kernel, dim3(k, cur), dim3(SPAN_THREADS), 0, x->stream, x->d_dist, ld, g_out + at, k, x->d_goff, sorder,
                               stie, tau, G, ab, mass ? mass + at : nullptr, len ? len + at : nullptr, rows ? rows + 3 * at : nullptr);
        }
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- warped alignment (knn_align.h) ----
// tests only, read per call: the LDS form's row limit, the distance budget and the winner tables' batch budget in bytes
AlignPlan align_plan_env(int64_t n, int64_t largest_group, int m, int winners, bool with_align) {
    return plan_align(n, largest_group, m, winners, with_align, seq_env("VQ_AMD_ALIGN_LDS_ROWS"), seq_env("VQ_AMD_ALIGN_DIST_BYTES"),
                      seq_env("VQ_AMD_ALIGN_BP_BYTES"));
}

// What the filter allows, by the host mirror of goff and the sorted filter list: the groups and the longest of them.
struct AlignShape { int64_t allowed = 0; int64_t largest = 0; };
template <class Visit>
void allowed_groups(const vq_index* x, const FilterLabels& f, int exclude, Visit visit) {
    size_t si = 0;
    for (int32_t g = 0; g < x->n_groups; ++g) {
        while (si < f.sel.size() && f.sel[si] < g) ++si;
        const bool listed = si < f.sel.size() && f.sel[si] == g;
        if (exclude ? !listed : listed) visit((int64_t)x->h_goff[(size_t)g + 1] - x->h_goff[(size_t)g]);
    }
}
AlignShape align_shape(const vq_index* x, const FilterLabels& f, int exclude) {
    AlignShape s;
    allowed_groups(x, f, exclude, [&](int64_t rows) { ++s.allowed; s.largest = std::max(s.largest, rows); });
    return s;
}

// d_clip [m][dim]; o: groups / distances [k], then costs [k], rows [k][2] and alignments [k][m][2], each or not asked for, placed
// in device memory.  Asynchronous on the index's stream once the (position, tie) order is on the device.
int align_clip_run(vq_index* x, const char* fn, const float* d_clip, int m, int k, float max_dist, const FilterLabels& f, int exclude,
                   const AlignShape& shape, const Outs& o) {
    int32_t* const g_out = o.dev<int32_t>(0); float* const d_out = o.dev<float>(1);
    int64_t* const cost = o.dev<int64_t>(2); int32_t* const rows = o.dev<int32_t>(3); int32_t* const align = o.dev<int32_t>(4);
    FilterPlan fp;
    VQ_TRY(filter_prepare(x, fn, f, exclude, true, &fp));
    if (!fp.all && fp.m == 0) {                             // nothing allowed: every slot empty
        set_stats(x, STATS_HOST, 0, 0, 0);
        return outs_empty_placed(x, o);
    }
    VQ_TRY(seq_order_prepare(x));
    const uint32_t* allow = fp.all ? nullptr : fp.bits;
    const int64_t n = x->size, ld = round_up(n, 64);
    const int G = x->n_groups;
    const int nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK);
    const int winners = (int)std::min<int64_t>(k, shape.allowed);
    const AlignPlan p = align_plan_env(n, shape.largest, m, winners, align != nullptr);
    int64_t global_groups = 0;
    if (p.global_form) allowed_groups(x, f, exclude, [&](int64_t rows_of) { global_groups += rows_of > p.lds_rows; });
    VQ_TRY(x->d_dist.reserve((int64_t)p.chunk_frames * ld));
    VQ_TRY(x->d_alignc.reserve(n + G));
    VQ_TRY(x->d_aligna.reserve(n + 2 * (int64_t)G + k));
    VQ_TRY(x->d_sekey.reserve((int64_t)G + (int64_t)nblocks * kl));
    if (align) VQ_TRY(x->d_alignbp.reserve(p.table_bytes / 4));
    VQ_TRY(ensure_gcounters(x));
    VQ_TRY(set_dyn_lds(x, (const void*)align_dp_lds_kernel, (size_t)p.lds_bytes));
    const int32_t* sorder = x->d_seq;
    int64_t* state_c = x->d_alignc; int64_t* gcost = state_c + n;
    int32_t* state_a = x->d_aligna; int32_t* gab = state_a + n; int32_t* sel = gab + 2 * (int64_t)G;
    uint64_t* ekey = x->d_sekey; uint64_t* partial = ekey + G;
    for (int i0 = 0; i0 < m; i0 += p.chunk_frames) {
        const int cur = std::min(p.chunk_frames, m - i0);
        VQ_TRY(exact_dist(x, false, d_clip + (int64_t)i0 * x->dim, cur, ld));          // always the tiled kernel
        Prof pr(x, I_SEQ_DP);
        hipLaunchKernelGGL(align_dp_lds_kernel, dim3(G), dim3(ALIGN_THREADS), (size_t)p.lds_bytes, x->stream, x->d_dist, ld, i0, cur, x->d_goff,
                           sorder, p.lds_rows, p.lds_alloc_rows, state_c, state_a, allow);
        if (p.global_form)
            hipLaunchKernelGGL(align_dp_global_kernel, dim3(G), dim3(ALIGN_THREADS), 0, x->stream, x->d_dist, ld, i0, cur, x->d_goff, sorder,
                               p.lds_rows, state_c, state_a, allow);
    }
    {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(align_final_kernel, dim3(G), dim3(ALIGN_THREADS), 0, x->stream, state_c, state_a, x->d_goff, m, max_dist, allow, ekey,
                           gcost, gab);
        hipLaunchKernelGGL(set_select_block_kernel, dim3(nblocks), dim3(256), 0, x->stream, ekey, G, kl, partial);
        hipLaunchKernelGGL(set_select_merge_kernel, dim3(1), dim3(256), 0, x->stream, partial, (int64_t)nblocks * kl, k, sel, d_out, nullptr,
                           nullptr);
        hipLaunchKernelGGL(align_order_kernel, dim3(k), dim3(256), 0, x->stream, ekey, G, gcost, sel, g_out);
        hipLaunchKernelGGL(seq_stats_kernel, dim3(1), dim3(256), 0, x->stream, ekey, G, (unsigned long long)global_groups,
                           (unsigned long long)p.frame_chunks, x->d_gcounters);
        if (cost || rows)
            hipLaunchKernelGGL(align_finish_kernel, dim3(cdiv(k, 64)), dim3(64), 0, x->stream, g_out, k, x->d_goff, sorder, gcost, gab, cost, rows);
    }
    if (align) {
        const int64_t stride = (int64_t)m * shape.largest;
        int32_t* table = x->d_alignbp;
        for (int b = 0; b < p.winner_batches; ++b) {
            const int w0 = b * p.winners_per_batch, nb = std::min(p.winners_per_batch, winners - w0);
            for (int i0 = 0; i0 < m; i0 += p.chunk_frames) {
                const int cur = std::min(p.chunk_frames, m - i0);
                if (p.frame_chunks > 1) VQ_TRY(exact_dist(x, false, d_clip + (int64_t)i0 * x->dim, cur, ld));   // (one chunk: still there)
                Prof pr(x, I_SEQ_DP);
                hipLaunchKernelGGL(align_trace_dp_kernel, dim3(nb), dim3(ALIGN_THREADS), 0, x->stream, x->d_dist, ld, i0, cur, g_out, w0, x->d_goff,
                                   sorder, state_c, state_a, table, stride);
            }
            Prof pr(x, I_SEQ_DP);
            const int count = b == p.winner_batches - 1 ? k - w0 : nb;        // the last batch also files the slots no group can fill
            hipLaunchKernelGGL(align_walk_kernel, dim3(cdiv(count, 64)), dim3(64), 0, x->stream, g_out, w0, count, m, x->d_goff, sorder, gab, table,
                               stride, align);
        }
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- keyframe summary (knn_summary.h) ----
SummaryPlan sum_plan_env(int64_t largest_group, int dim, int k) {
    return plan_summary(largest_group, dim, k, seq_env("VQ_AMD_SUM_LDS_ROWS"));      // tests only, read per call
}

// Everything that can refuse a summary before any work is queued.
int sum_precheck(vq_index* x, const char* fn, const int32_t* groups, int32_t n_sel) {
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    for (int32_t i = 0; i < n_sel; ++i)
        VQ_CHECK(groups[i] >= 0 && groups[i] < x->n_groups, "%s: group %d outside [0, %d)", fn, (int)groups[i], (int)x->n_groups);
    return 0;
}

// groups [n_sel]: host, checked.  rows_out / radius_out / members_out (or null) [n_sel][k]: device.  Asynchronous on the index's
// stream.  Entries of more than the plan's lds_rows rows (a group named twice: twice) go to the wide form through host-built lists.
int summarize_run(vq_index* x, const char* fn, const int32_t* groups, int32_t n_sel, int k, float max_radius, int32_t* rows_out,
                  float* radius_out, int32_t* members_out) {
    const int dim = x->dim;
    const int32_t* hg = x->h_goff.data();
    auto len_of = [&](int32_t g) { return (int64_t)hg[g + 1] - hg[g]; };
    int64_t largest = 0;
    for (int32_t i = 0; i < n_sel; ++i) largest = std::max(largest, len_of(groups[i]));
    const SummaryPlan p = sum_plan_env(largest, dim, k);
    int64_t lds_longest = 0, nw = 0, nb = 0, W = 0;
    for (int32_t i = 0; i < n_sel; ++i) {
        const int64_t L = len_of(groups[i]);
        if (L <= p.lds_rows) lds_longest = std::max(lds_longest, L);
        else { ++nw; nb += cdiv(L, SUM_BLOCK); W += L; }
    }
    VQ_CHECK(W < ((int64_t)1 << 31), "%s: the listed groups above %d rows hold %lld rows together, 2^31 or more", fn, p.lds_rows, (long long)W);
    auto words = [](int64_t c) { return round_up(std::max<int64_t>(c, 1), 4); };        // 16-byte aligned regions
    // host-built lists, one copy: sel [n_sel] | slot [nw] | group [nw] | boff [nw + 1] | soff [nw + 1] | blk_entry [nb]
    const int64_t w_sel = words(n_sel), w_nw = words(nw), w_nw1 = words(nw + 1), w_nb = words(nb);
    const int64_t w_lists = w_sel + 2 * w_nw + 2 * w_nw1 + w_nb;
    // behind them: kap [n_sel] | near [W] | owner [W] | bidx [nb] | cur [nw] | done [nw] | kappa [nw]
    VQ_TRY(x->d_sumw.reserve(w_lists + w_sel + 2 * words(W) + w_nb + 3 * w_nw));
    if (nw) {
        VQ_TRY(x->d_sumk.reserve(nb));
        VQ_TRY(x->d_sumd.reserve((nb + nw) * dim));
    }
    VQ_TRY(ensure_gcounters(x));
    const int alloc_rows = (int)round_up(std::max<int64_t>(lds_longest, 1), 64);
    const size_t lds_bytes = (size_t)summary_lds_bytes(lds_longest, dim), wide_lds = (size_t)dim * 8 + 64;
    VQ_TRY(set_dyn_lds(x, (const void*)sum_lds_kernel, lds_bytes));
    if (nw) {
        VQ_TRY(set_dyn_lds(x, (const void*)sum_wide_update_kernel<true>, wide_lds));
        VQ_TRY(set_dyn_lds(x, (const void*)sum_wide_update_kernel<false>, wide_lds));
    }
    StageSlot* slot;
    VQ_TRY(stage_slot(x, w_lists, &slot));
    int32_t* h = slot->h;
    int32_t* h_slot = h + w_sel; int32_t* h_group = h_slot + w_nw; int32_t* h_boff = h_group + w_nw; int32_t* h_soff = h_boff + w_nw1;
    int32_t* h_blk = h_soff + w_nw1;
    std::memcpy(h, groups, (size_t)n_sel * 4);
    int64_t e = 0, blk = 0, st = 0;
    for (int32_t i = 0; i < n_sel; ++i) {
        const int64_t L = len_of(groups[i]);
        if (L <= p.lds_rows) continue;
        h_slot[e] = i; h_group[e] = groups[i]; h_boff[e] = (int32_t)blk; h_soff[e] = (int32_t)st;
        for (int j = 0; j < cdiv(L, SUM_BLOCK); ++j) h_blk[blk++] = (int32_t)e;
        st += L; ++e;
    }
    h_boff[nw] = (int32_t)blk; h_soff[nw] = (int32_t)st;
    int32_t* d = x->d_sumw;
    VQ_HIP(hipMemcpyAsync(d, h, (size_t)w_lists * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipEventRecord(slot->ev, x->stream));
    const int32_t* sel = d;
    SumWide w;
    w.slot = d + w_sel; w.group = w.slot + w_nw; w.boff = w.group + w_nw; w.soff = w.boff + w_nw1; w.blk_entry = w.soff + w_nw1;
    int32_t* kap = d + w_lists;
    w.near = (uint32_t*)(kap + w_sel); w.owner = (int32_t*)w.near + words(W); w.bidx = w.owner + words(W);
    w.cur = w.bidx + w_nb; w.done = w.cur + w_nw; w.kappa = w.done + w_nw;
    w.bmax = x->d_sumk; w.bsum = x->d_sumd; w.cvec = nw ? x->d_sumd + nb * dim : nullptr;
    const TieOrder tie = x->tie();
    {
        Prof pr(x, I_EXACT_DIST);
        hipLaunchKernelGGL(sum_lds_kernel, dim3(n_sel), dim3(SUM_THREADS), lds_bytes, x->stream, x->rows, dim, x->d_goff, x->d_grows, tie, sel, k,
                           max_radius, p.lds_rows, alloc_rows, rows_out, radius_out, members_out, kap);
        if (nw) {
            const dim3 gb((unsigned)nb), ge((unsigned)nw), th(SUM_THREADS);
            hipLaunchKernelGGL(sum_wide_blocksum_kernel, gb, th, 0, x->stream, x->rows, dim, x->d_goff, x->d_grows, w);
            hipLaunchKernelGGL(sum_wide_mean_kernel, ge, th, 0, x->stream, dim, w);
            hipLaunchKernelGGL(sum_wide_update_kernel<true>, gb, th, wide_lds, x->stream, x->rows, dim, x->d_goff, x->d_grows, tie, w, 0);
            hipLaunchKernelGGL(sum_wide_pick_kernel, ge, th, 0, x->stream, x->d_goff, x->d_grows, w, 1, 0, k, max_radius, rows_out, radius_out);
            for (int t = 0; t < k; ++t) {
                hipLaunchKernelGGL(sum_wide_update_kernel<false>, gb, th, wide_lds, x->stream, x->rows, dim, x->d_goff, x->d_grows, tie, w, t);
                hipLaunchKernelGGL(sum_wide_pick_kernel, ge, th, 0, x->stream, x->d_goff, x->d_grows, w, 0, t, k, max_radius, rows_out, radius_out);
            }
            hipLaunchKernelGGL(sum_wide_members_kernel, ge, th, 0, x->stream, w, k, rows_out, radius_out, members_out, kap);
        }
        hipLaunchKernelGGL(sum_stats_kernel, dim3(1), dim3(256), 0, x->stream, kap, n_sel, (unsigned long long)(n_sel - nw), (unsigned long long)nw,
                           x->d_gcounters);
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- chapter segmentation (knn_segment.h) ----
SegmentPlan seg_plan_env(const int64_t* lengths, int32_t n_sel, int dim, int k, int64_t max_len, bool show) {
    return plan_segment(lengths, n_sel, dim, k, max_len, show, seq_env("VQ_AMD_SEG_COST_BYTES"), seq_env("VQ_AMD_SEG_LDS_ROWS"));   // tests only, read per call
}

// a group whose band table alone would pass the stated bound is refused: the work is quadratic
int seg_check_pairs(const char* fn, int32_t label, int64_t L, int64_t max_len) {
    const int64_t W = seg_run_limit(L, max_len);
    VQ_CHECK(L * W <= SEG_MAX_PAIRS, "%s: group %d holds %lld rows: %lld x %lld (rows x longest run) is more than 2^26 pairs; pass a smaller max_len",
             fn, (int)label, (long long)L, (long long)L, (long long)W);
    return 0;
}

// Everything that can refuse a segmentation before any work is queued.  len [n_sel]: the listed groups' rows.
int seg_precheck(vq_index* x, const char* fn, const int32_t* groups, int32_t n_sel, int k, int64_t max_len, std::vector<int64_t>* len) {
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(check_labels(x, fn));
    VQ_TRY(check_positions(x, fn));
    VQ_CHECK((int64_t)n_sel * k < ((int64_t)1 << 31), "%s: n_sel x k = %lld slots, 2^31 or more", fn, (long long)n_sel * k);
    len->resize((size_t)n_sel);
    for (int32_t i = 0; i < n_sel; ++i) {
        VQ_CHECK(groups[i] >= 0 && groups[i] < x->n_groups, "%s: group %d outside [0, %d)", fn, (int)groups[i], (int)x->n_groups);
        (*len)[(size_t)i] = (int64_t)x->h_goff[(size_t)groups[i] + 1] - x->h_goff[(size_t)groups[i]];
        VQ_TRY(seg_check_pairs(fn, groups[i], (*len)[(size_t)i], max_len));
    }
    return 0;
}

// groups [n_sel]: host, checked, with their lengths.  Outputs: device; show / mean may be null.  Asynchronous on the index's stream
// once the (position, tie) order is on the device.  Per batch of listed groups: prefix rows, band table, DP, show rows.
int segment_run(vq_index* x, const char* fn, const int32_t* groups, int32_t n_sel, const std::vector<int64_t>& len, int k, float penalty,
                int64_t max_len, int32_t* count, int32_t* first, int32_t* last, int32_t* lens, float* spread, int32_t* show, float* mean) {
    const int dim = x->dim;
    const SegmentPlan p = seg_plan_env(len.data(), n_sel, dim, k, max_len, show != nullptr);
    VQ_CHECK(p.tiles < ((int64_t)1 << 31) && p.prefix_rows < ((int64_t)1 << 31), "%s: a batch of %lld tiles and %lld prefix rows is too large",
             fn, (long long)p.tiles, (long long)p.prefix_rows);
    VQ_TRY(seq_order_prepare(x));
    // words: the entries of every batch, each batch closed by one more | cuts [n_sel][k][2] | a batch's back-pointers
    const int64_t n_ent = (int64_t)n_sel + p.batches;
    const int64_t w_ent = round_up(n_ent * SEG_ENTRY_WORDS, 4), w_cuts = round_up((int64_t)2 * n_sel * k, 4);
    VQ_TRY(x->d_segw.reserve(w_ent + w_cuts + p.bp_words));
    VQ_TRY(x->d_segd.reserve(p.prefix_rows * dim + p.table_bytes / 8));
    if (p.e_words) VQ_TRY(x->d_sege.reserve(p.e_words));
    VQ_TRY(ensure_gcounters(x));
    VQ_TRY(set_dyn_lds(x, (const void*)seg_dp_kernel, (size_t)p.lds_bytes));
    StageSlot* slot;
    VQ_TRY(stage_slot(x, w_ent, &slot));
    SegEntry* he = (SegEntry*)(int32_t*)slot->h;
    int64_t e = 0;
    int32_t b0 = 0;
    for (int bi = 0; bi < p.batches; ++bi) {
        const int32_t end = p.batch_end[(size_t)bi];
        SegEntry run{};                                                 // the running offsets; closes the batch
        for (int32_t i = b0; i < end; ++i, ++e) {
            const int64_t L = len[(size_t)i], W = seg_run_limit(L, max_len);
            he[e] = run;
            he[e].group = groups[i]; he[e].L = (int32_t)L; he[e].W = (int32_t)W; he[e].slot = i;
            he[e].band = L ? seg_band(L, W) : 1;
            run.toff += L * W; run.bpoff += std::min<int64_t>(k, L) * (L + 1); run.prow += (int32_t)(L + 1);
            if (L > p.lds_rows) run.eoff += 2 * (L + 1);
            if (L) run.tile0 += seg_tiles_b(L) * seg_band(L, W);
        }
        he[e++] = run;
        b0 = end;
    }
    int32_t* d = x->d_segw;
    VQ_HIP(hipMemcpyAsync(d, he, (size_t)n_ent * sizeof(SegEntry), hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipEventRecord(slot->ev, x->stream));
    const SegEntry* ent = (const SegEntry*)d;
    int32_t* cuts = d + w_ent;
    int32_t* bp = cuts + w_cuts;
    double* P = x->d_segd;
    double* tab = P + p.prefix_rows * dim;
    const int32_t* sorder = x->d_seq;
    const TieOrder tie = x->tie();
    {
        Prof pr(x, I_EXACT_DIST);
        e = 0; b0 = 0;
        for (int bi = 0; bi < p.batches; ++bi) {
            const int32_t end = p.batch_end[(size_t)bi], nb = end - b0;
            const int32_t tiles = he[e + nb].tile0;
            const SegEntry* be = ent + e;
            hipLaunchKernelGGL(seg_prefix_kernel, dim3(nb), dim3((unsigned)round_up(dim / 4, 64)), 0, x->stream, x->rows, dim, x->d_goff, sorder, be, P);
            if (tiles)
                hipLaunchKernelGGL(seg_pair_kernel, dim3((unsigned)tiles), dim3(SEG_PAIR_THREADS), 0, x->stream, be, nb, P, dim, tab);
            hipLaunchKernelGGL(seg_dp_kernel, dim3(nb), dim3(SEG_DP_THREADS), (size_t)p.lds_bytes, x->stream, be, tab, bp, x->d_sege.p, x->d_goff, sorder,
                               k, penalty, p.lds_rows, (int)(p.lds_bytes / 16), count, first, last, lens, spread, mean, cuts);
            if (show)
                hipLaunchKernelGGL(seg_show_kernel, dim3((unsigned)((int64_t)nb * k)), dim3(SEG_SHOW_THREADS), 0, x->stream, x->rows, dim, x->d_goff, sorder,
                                   be, P, cuts, k, tie, show);
            e += nb + 1; b0 = end;
        }
        hipLaunchKernelGGL(seg_stats_kernel, dim3(1), dim3(256), 0, x->stream, count, n_sel, (unsigned long long)p.pairs, (unsigned long long)p.batches,
                           x->d_gcounters);
    }
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- zero-shot labelling (knn_label.h) ----
bool label_fp16_ok(const vq_index* x) { return scan_fp16_dim(x->dim) && x->size >= 1 && x->near_unit; }

// Everything that can refuse a labelling call before any work is queued: the mode, for group outputs stale ranks or labels,
// and mode 2 where the tile path does not exist.
int label_precheck(vq_index* x, const char* fn, int mode, bool groups) {
    VQ_TRY(check_mode(fn, mode));
    if (groups) {
        VQ_TRY(check_ranks(x, fn));
        VQ_TRY(check_labels(x, fn));
    }
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    if (mode == 2) VQ_CHECK(label_fp16_ok(x), "%s: the fp16 path needs dim 256, 512 or 768 and near-unit rows (0.5 <= |row|^2 <= 2; rows "
                                              "added with normalize=0 are measured); mode 1 takes any call", fn);
    return 0;
}

int check_label_args(const char* fn, const vq_index* x, const void* prompts, int P, float max_dist, int m, bool groups, bool group_arrays) {
    VQ_CHECK(P >= 1 && P <= LABEL_MAX_P, "%s: P %d outside [1, %d]", fn, P, LABEL_MAX_P);
    VQ_CHECK(max_dist == max_dist, "%s: max_dist is NaN (+inf: every row is labelled)", fn);
    if (groups) VQ_CHECK(m >= 1 && m <= LABEL_MAX_M && group_arrays, "%s: group outputs take 1 <= m <= %d and all four arrays", fn, LABEL_MAX_M);
    VQ_TRY(require_init());
    VQ_CHECK(x && prompts, "%s: bad argument", fn);
    return 0;
}

// The group outputs from the rows' labels (device memory throughout).  Groups above LABEL_GROUP_SPLIT_ROWS rows take the split
// form: their pieces are listed on the host from the labels' mirror and go up in one copy from the staging ring.
int label_groups_run(vq_index* x, const int32_t* lab, const float* best, int P, int m, int32_t* tags, int32_t* votes, int32_t* show,
                     int32_t* unl) {
    const int32_t* hg = x->h_goff.data();
    const int G = x->n_groups;
    int64_t nl = 0, np = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t L = (int64_t)hg[g + 1] - hg[g];
        if (L > LABEL_GROUP_SPLIT_ROWS) { ++nl; np += cdiv(L, LABEL_GROUP_PIECE_ROWS); }
    }
    const TieOrder tie = x->tie();
    Prof pr(x, I_SELECT);
    hipLaunchKernelGGL(label_group_kernel, dim3(G), dim3(256), 0, x->stream, x->d_goff, x->d_grows, lab, best, P, m, LABEL_GROUP_SPLIT_ROWS, tie,
                       tags, votes, show, unl);
    if (nl) {
        auto words = [](int64_t c) { return round_up(std::max<int64_t>(c, 1), 4); };        // 16-byte aligned regions
        // host-built lists, one copy: piece_long [np] | piece_b [np] | piece_e [np] | long_group [nl] | long_poff [nl + 1]
        const int64_t w_np = words(np), w_nl = words(nl), w_nl1 = words(nl + 1), w_lists = 3 * w_np + w_nl + w_nl1;
        // behind them: punl [np] | lsel [nl][16]
        VQ_TRY(x->d_lgw.reserve(w_lists + w_np + words(nl * LABEL_MAX_M)));
        VQ_TRY(x->d_lghist.reserve(np * P));
        VQ_TRY(x->d_lgshow.reserve(np * LABEL_MAX_M));
        StageSlot* slot;
        VQ_TRY(stage_slot(x, w_lists, &slot));
        int32_t* h = slot->h;
        int32_t* h_pl = h; int32_t* h_pb = h + w_np; int32_t* h_pe = h_pb + w_np; int32_t* h_lg = h_pe + w_np; int32_t* h_lp = h_lg + w_nl;
        int64_t l = 0, q = 0;
        for (int g = 0; g < G; ++g) {
            const int64_t L = (int64_t)hg[g + 1] - hg[g];
            if (L <= LABEL_GROUP_SPLIT_ROWS) continue;
            h_lg[l] = g; h_lp[l] = (int32_t)q;
            for (int64_t b = hg[g]; b < hg[g + 1]; b += LABEL_GROUP_PIECE_ROWS) {
                h_pl[q] = (int32_t)l; h_pb[q] = (int32_t)b; h_pe[q] = (int32_t)std::min<int64_t>(b + LABEL_GROUP_PIECE_ROWS, hg[g + 1]);
                ++q;
            }
            ++l;
        }
        h_lp[nl] = (int32_t)q;
        int32_t* d = x->d_lgw;
        VQ_HIP(hipMemcpyAsync(d, h, (size_t)w_lists * 4, hipMemcpyHostToDevice, x->stream));
        VQ_HIP(hipEventRecord(slot->ev, x->stream));
        LabelPieces w;
        w.piece_long = d; w.piece_b = d + w_np; w.piece_e = d + 2 * w_np; w.long_group = d + 3 * w_np; w.long_poff = d + 3 * w_np + w_nl;
        w.punl = d + w_lists; w.lsel = w.punl + w_np;
        w.phist = x->d_lghist; w.pshow = (unsigned long long*)x->d_lgshow.p;
        hipLaunchKernelGGL(label_piece_hist_kernel, dim3((unsigned)np), dim3(256), 0, x->stream, x->d_grows, lab, P, w);
        hipLaunchKernelGGL(label_long_select_kernel, dim3((unsigned)nl), dim3(256), 0, x->stream, P, m, w, tags, votes, show, unl);
        hipLaunchKernelGGL(label_piece_show_kernel, dim3((unsigned)np), dim3(256), 0, x->stream, x->d_grows, lab, best, tie, w);
        hipLaunchKernelGGL(label_long_show_kernel, dim3(cdiv(nl * LABEL_MAX_M, 256)), dim3(256), 0, x->stream, (int)nl, m, tie, w, show);
    }
    VQ_HIP(hipGetLastError());
    return 0;
}

// d_prompts [P][dim]; lab_out / best_out [n] or null (the call's own scratch then); tags / votes / show [G][m] and unl [G] or
// tags null: all device memory.  force_exact: the host form found a prompt outside the fp16 bound's range.  Asynchronous on
// the index's stream; *lab / *best: where the rows' answers are.
int label_run(vq_index* x, const float* d_prompts, int P, int mode, bool force_exact, float max_dist, int32_t* lab_out, float* best_out,
              int m, int32_t* tags, int32_t* votes, int32_t* show, int32_t* unl, int32_t** lab_at, float** best_at) {
    const int64_t n = x->size;
    const LabelPlan p = plan_label(n, x->dim, P, mode, x->near_unit, 0);
    const int64_t n_pad = p.row_tiles * LABEL_ROW_TILE;
    VQ_TRY(x->d_lw.reserve(4 + 3 * n_pad));
    int32_t* ctl = x->d_lw; int32_t* filed = ctl + 4;
    int32_t* lab = lab_out ? lab_out : filed + n_pad;
    float* best = best_out ? best_out : (float*)(filed + 2 * n_pad);
    if (lab_at) *lab_at = lab;
    if (best_at) *best_at = best;
    x->last_label.valid = false;
    if (!p.fp16 || force_exact) {
        const int64_t ld = round_up(n, 64);
        VQ_TRY(x->d_lrun.reserve(n));
        VQ_TRY(x->d_dist.reserve((int64_t)p.exact_chunk * ld));
        for (int j0 = 0; j0 < P; j0 += p.exact_chunk) {
            const int cur = std::min(p.exact_chunk, P - j0);
            VQ_TRY(exact_dist(x, false, d_prompts + (int64_t)j0 * x->dim, cur, ld));       // always the tiled kernel
            Prof pr(x, I_SELECT);
            hipLaunchKernelGGL(label_colmin_kernel, dim3(grid_for(n)), dim3(256), 0, x->stream, x->d_dist, ld, n, cur, j0, j0 == 0 ? 1 : 0,
                               j0 + cur == P ? 1 : 0, max_dist, x->d_lrun, lab, best);
        }
        VQ_HIP(hipGetLastError());
        set_stats(x, STATS_HOST, 0, 0, n);
    } else {
        const int64_t p_pad = (int64_t)p.prompt_tiles * LABEL_PT;
        VQ_TRY(x->d_q16.reserve(p_pad * x->dim));
        VQ_TRY(x->d_lparts.reserve(p.part_bytes / 4));
        VQ_TRY(ensure_gcounters(x));
        VQ_TRY(set_dyn_lds(x, (const void*)label_tile_kernel, LABEL_LDS_BYTES));
        VQ_HIP(hipMemsetAsync(ctl, 0, 16, x->stream));
        VQ_HIP(hipMemsetAsync(x->d_gcounters, 0, 3 * sizeof(unsigned long long), x->stream));
        hipLaunchKernelGGL(label_prompt_norm_kernel, dim3(P), dim3(64), 0, x->stream, d_prompts, x->dim, ctl);
        queries_to_f16(x, d_prompts, P, p_pad);
        {
            Prof pr(x, I_MFMA_SCAN);
            hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)(p.row_tiles * p.prompt_ranges)), dim3(G2_THREADS), LABEL_LDS_BYTES, x->stream,
                               x->rows16, x->d_q16, x->dim, P, p.prompt_tiles, p.prompt_ranges, n_pad, x->d_lparts);
        }
        x->last_label = {true, n, n_pad, p.prompt_ranges, P};
        {
            Prof pr(x, I_RESCORE);
            hipLaunchKernelGGL(label_finalize_kernel, dim3(grid_for(n)), dim3(256), 0, x->stream, x->d_lparts, p.prompt_ranges, n_pad, n, x->rows,
                               x->dim, d_prompts, scan_eps_unit(x->dim) * x->row_norm_max, max_dist, ctl, filed, lab, best, x->d_gcounters);
        }
        {
            Prof pr(x, I_EXACT_DIST);
            hipLaunchKernelGGL(label_redo_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 4), 4096)), dim3(256), 0, x->stream, x->rows, n, x->dim,
                               d_prompts, P, max_dist, ctl, filed, lab, best, x->d_gcounters);
        }
        VQ_HIP(hipGetLastError());
        VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
        set_stats(x, STATS_GCOUNTERS);
    }
    if (tags) VQ_TRY(label_groups_run(x, lab, best, P, m, tags, votes, show, unl));
    return 0;
}

// ---- library clustering (knn_cluster.h) ----
static_assert(CL_MAX_P == LABEL_MAX_P, "knn_cluster.h: a cluster is a prompt of the label call");

struct ClusterBufs {
    int32_t* ctl; int32_t* prev; int32_t* lab; float* best; int32_t* list; int32_t* cnt; int32_t* off; int32_t* poff;
    int32_t* counts; int32_t* show;      // the host form's results
    ClusterPlan plan;
};

int cluster_reserve(vq_index* x, int P, ClusterBufs* b) {
    const int64_t n = x->size, nw = round_up(n, 4), pw = round_up((int64_t)P + 1, 4);
    b->plan = plan_cluster(n, x->dim, P);
    VQ_TRY(x->d_clw.reserve(CL_CTL_WORDS + 4 * nw + 5 * pw));
    VQ_TRY(x->d_cltab.reserve(b->plan.blocks * P));
    VQ_TRY(x->d_clsum.reserve(b->plan.max_pieces * x->dim));
    VQ_TRY(x->d_clkey.reserve(P));
    int32_t* w = x->d_clw;
    b->ctl = w; b->prev = w + CL_CTL_WORDS; b->lab = b->prev + nw; b->best = (float*)(b->lab + nw); b->list = b->lab + 2 * nw;
    b->cnt = b->list + nw; b->off = b->cnt + pw; b->poff = b->off + pw; b->counts = b->poff + pw; b->show = b->counts + pw;
    VQ_HIP(hipMemsetAsync(b->ctl, 0, CL_CTL_WORDS * 4, x->stream));
    return 0;
}

// The by-label row list of lab [n], its offsets and pieces; counts_out / changed_out (device addresses) or null.
void cluster_list(vq_index* x, const ClusterBufs& b, const int32_t* lab, int P, bool first, int32_t* counts_out, int32_t* changed_out) {
    const int64_t n = x->size;
    Prof pr(x, I_SELECT);
    hipLaunchKernelGGL(cluster_hist_kernel, dim3((unsigned)b.plan.blocks), dim3(256), 0, x->stream, lab, b.prev, n, P, first ? 1 : 0, x->d_cltab, b.ctl);
    hipLaunchKernelGGL(cluster_prefix_kernel, dim3(cdiv(P, 256)), dim3(256), 0, x->stream, x->d_cltab, b.plan.blocks, P, b.cnt);
    hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(1024), 0, x->stream, b.cnt, P, b.off, b.poff, (unsigned long long*)x->d_clkey.p, counts_out,
                       b.ctl, changed_out);
    hipLaunchKernelGGL(cluster_scatter_kernel, dim3((unsigned)b.plan.blocks), dim3(256), 0, x->stream, lab, n, P, x->d_cltab, b.off, b.list);
}

// C [P][dim] <- the update of the list's clusters, in place.  The pieces' sums are accounted under exact_dist_f64chain (fp64
// chains over the master), the finish under normalize_rows.
void cluster_update(vq_index* x, const ClusterBufs& b, int P, float* C) {
    {
        Prof pr(x, I_EXACT_DIST);
        hipLaunchKernelGGL(cluster_piece_kernel, dim3((unsigned)b.plan.max_pieces), dim3(b.plan.piece_threads), 0, x->stream, x->rows, x->dim, P, b.list,
                           b.off, b.poff, b.ctl, x->d_clsum);
    }
    Prof pr(x, I_NORMALIZE);
    hipLaunchKernelGGL(cluster_finish_kernel, dim3(P), dim3(256), 0, x->stream, x->d_clsum, x->dim, b.off, b.poff, C);
}

void cluster_show(vq_index* x, const ClusterBufs& b, int P, const float* best, int32_t* show) {
    const TieOrder tie = x->tie();
    Prof pr(x, I_SELECT);
    hipLaunchKernelGGL(cluster_show_kernel, dim3((unsigned)b.plan.max_pieces), dim3(256), 0, x->stream, b.list, b.off, b.poff, P, b.ctl, best, tie,
                       (unsigned long long*)x->d_clkey.p);
    hipLaunchKernelGGL(cluster_show_rows_kernel, dim3(cdiv(P, 256)), dim3(256), 0, x->stream, (const unsigned long long*)x->d_clkey.p, P, tie, show);
}

// Everything that can refuse a clustering call before any work is queued, the arguments aside: stale ranks (the show rows'
// ties), the mode, mode 2 where the label call refuses it.
int cluster_precheck(vq_index* x, const char* fn, int mode) {
    VQ_TRY(check_ranks(x, fn));
    return label_precheck(x, fn, mode, false);
}

int check_cluster_args(const char* fn, const vq_index* x, const void* init, const void* init_rows, int P, int iters, bool outputs) {
    VQ_CHECK(P >= 1 && P <= CL_MAX_P, "%s: P %d outside [1, %d]", fn, P, CL_MAX_P);
    VQ_CHECK(iters >= 1 && iters <= CL_MAX_ITER, "%s: %d iterations outside [1, %d]", fn, iters, CL_MAX_ITER);
    VQ_CHECK((init != nullptr) != (init_rows != nullptr), "%s: give exactly one of init and init_rows", fn);
    VQ_TRY(require_init());
    VQ_CHECK(x && outputs, "%s: bad argument", fn);
    return 0;
}

// C [P][dim] holds C_1 (device memory) and ends as C_T.  The host form (h_changed != null: the mapped counters) waits for the
// stream once per iteration and stops at a fixed point; the device form runs `iters` assignments and reads nothing back.
// lab / best: where the rows' answers go (the caller's arrays or the call's scratch).  *T: the iterations run.
int cluster_run(vq_index* x, const ClusterBufs& b, float* C, int P, int iters, int mode, bool force_exact, int32_t* lab, float* best,
                int32_t* counts, int32_t* show, int32_t* changed, int* T) {
    const bool host = changed != nullptr;
    const float inf = __builtin_inff();
    int t = 1;
    for (;; ++t) {
        VQ_TRY(label_run(x, C, P, mode, force_exact, inf, lab, best, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        cluster_list(x, b, lab, P, t == 1, counts, host ? x->h_clchanged.dev + (t - 1) : nullptr);
        VQ_HIP(hipGetLastError());
        if (host) {
            VQ_HIP(hipStreamSynchronize(x->stream));
            changed[t - 1] = x->h_clchanged[t - 1];
            if (t > 1 && changed[t - 1] == 0) break;
        }
        if (t == iters) break;
        cluster_update(x, b, P, C);
    }
    cluster_show(x, b, P, best, show);
    VQ_HIP(hipGetLastError());
    *T = t;
    return 0;
}

// ---- compound search (knn_compound.h) ----
// Everything that can refuse a compound search before any work is queued, the arguments aside: stale ranks, and mode 2 where the
// fp16 path does not exist.
int compound_precheck(vq_index* x, const char* fn, int k, int mode) {
    VQ_TRY(check_ranks(x, fn));
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    if (mode == 2) VQ_CHECK(scan_fp16_dim(x->dim) && x->near_unit && k <= CP_K_MAX, "%s: the fp16 path needs dim 256, 512 or 768, "
                            "k <= %d and near-unit rows (0.5 <= |row|^2 <= 2; rows added with normalize=0 are measured); mode 1 takes any call",
                            fn, CP_K_MAX);
    return 0;
}

// d_terms [m][dim], ids / dist [k], td [k][m] or null: all device memory.  Asynchronous on the index's stream.  force_exact: the
// host form found a term norm the fp16 bound does not cover.
int compound_run(vq_index* x, const float* d_terms, int m, const int32_t* clause_of, float margin, int k, int mode, bool force_exact,
                 int32_t* ids, float* dist, float* td) {
    const int64_t n = x->size;
    const CompoundPlan p = plan_compound(n, x->dim, m, clause_of, k, mode, x->near_unit);
    VQ_TRY(x->d_ctab.reserve((int64_t)m * p.ld));
    const TieOrder tie = x->tie();
    const bool one_wg = n <= SEL_SMALL_MAX_N;
    // the exact path's two ends; gate = null: the call's answer, else the redo behind the call's flag
    auto term_dists = [&](const unsigned long long* gate) {
        Prof pr(x, I_EXACT_DIST);
        hipLaunchKernelGGL(compound_dist_kernel, dim3(cdiv(n, 64)), dim3(256), 0, x->stream, x->rows, n, x->dim, d_terms, p.spec, margin,
                           x->d_ctab, p.ld, x->d_dist, gate);
    };
    auto finish = [&](const unsigned long long* gate) {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(compound_finish_kernel, dim3(1), dim3(256), 0, x->stream, ids, dist, k, x->d_ctab, p.ld, m, td, gate);
    };
    if (!p.fp16 || force_exact) {
        VQ_TRY(exact_topk(x, n, 1, k, one_wg, tie, ids, dist, [&](int, int, int64_t) { term_dists(nullptr); return 0; }));
        finish(nullptr);
        VQ_HIP(hipGetLastError());
        return 0;                                           // (exact_topk has set the stats: one call answered exactly)
    }
    const int nchunks = cdiv(n, SEL_CHUNK);
    VQ_TRY(x->d_q16.reserve((int64_t)CP_MAX_M * x->dim));
    VQ_TRY(x->d_keys.reserve(p.streams * 2));
    VQ_TRY(x->d_dist.reserve(p.ld));
    if (!one_wg) VQ_TRY(x->d_partial.reserve((int64_t)nchunks * k));
    VQ_TRY(ensure_gcounters(x));
    x->last_scan.valid = false;                             // the combined keys take the plain search's buffer
    const float eps_rows = scan_eps_unit(x->dim) * x->row_norm_max;
    unsigned long long* gc = x->d_gcounters;
    {
        Prof pr(x, I_TO_F16);
        hipLaunchKernelGGL(compound_terms_to_f16_kernel, dim3(CP_MAX_M), dim3(256), 0, x->stream, d_terms, p.lanes, x->dim, x->d_q16);
    }
    {
        Prof pr(x, I_MFMA_SCAN);
        auto scan = x->dim == 768 ? compound_scan_kernel<24> : x->dim == 512 ? compound_scan_kernel<16> : compound_scan_kernel<8>;
        hipLaunchKernelGGL(scan, dim3(cdiv(p.streams, 4)), dim3(256), 0, x->stream, x->d_q16, x->rows16, n, p.streams, p.lanes,
                           compound_veto_thr(eps_rows, margin), x->d_keys);
    }
    {
        Prof pr(x, I_RESCORE);
        hipLaunchKernelGGL(compound_rescore_kernel, dim3(1), dim3(256), 0, x->stream, x->d_keys, p.streams, x->rows, n, x->dim, d_terms, p.spec,
                           margin, k, p.pool, eps_rows, ids, dist, td, gc, tie);
    }
    // the redo: every kernel of it leaves at once unless the re-score set the flag
    term_dists(gc + 2);
    {
        Prof pr(x, I_SELECT);
        if (one_wg) {
            hipLaunchKernelGGL(select_small_kernel, dim3(1), dim3(256), 0, x->stream, x->d_dist, p.ld, n, k, ids, dist, tie, gc + 2, 0);
        } else {
            hipLaunchKernelGGL(select_chunk_kernel, dim3(1, nchunks), dim3(256), 0, x->stream, x->d_dist, p.ld, n, k, nchunks, x->d_partial, tie, gc + 2, 0);
            hipLaunchKernelGGL(merge_topk_kernel, dim3(1), dim3(256), 0, x->stream, x->d_partial, nchunks, k, ids, dist, tie, gc + 2, 0);
        }
    }
    finish(gc + 2);
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- shared-footage search (knn_match.h) ----
bool match_fp16_ok(const vq_index* x) { return scan_fp16_dim(x->dim) && x->size >= 1 && x->near_unit; }

MatchPlan match_plan_env(int64_t n, int64_t n_groups, int dim, int m, int mode, bool near_unit) {
    return plan_match(n, n_groups, dim, m, mode, near_unit, seq_env("VQ_AMD_MATCH_FILED_CAP"));      // tests only, read per call
}

// the bit table's stated bound
int match_check_bits(const char* fn, int m, int64_t n) {
    const int64_t bytes = (int64_t)m * ((std::max<int64_t>(n, 1) + 31) / 32) * 4;
    VQ_CHECK(bytes <= MATCH_BITS_BYTES, "%s: m = %d frames against %lld rows need a bit table of %lld bytes; m x ceil(n / 32) x 4 B must stay "
             "within %lld (send the clip in pieces)", fn, m, (long long)n, (long long)bytes, (long long)MATCH_BITS_BYTES);
    return 0;
}

// Everything that can refuse a shared-footage search before any work is queued.
int match_precheck(vq_index* x, const char* fn, int m, int mode, const FilterLabels& f) {
    VQ_TRY(match_check_bits(fn, m, x->size));
    VQ_TRY(seq_precheck(x, fn, f));
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    if (mode == 2) VQ_CHECK(match_fp16_ok(x), "%s: the tile path needs dim 256, 512 or 768 and near-unit rows (0.5 <= |row|^2 <= 2; rows "
                                              "added with normalize=0 are measured); mode 1 takes any call", fn);
    return 0;
}

// d_queries [m][dim]; o: the seven result arrays [k] each (match_outs), placed in device memory.  force_exact: the host form found
// a query outside the fp16 bound's range.  Asynchronous on the index's stream once the (position, tie) order is on the device.
int match_run(vq_index* x, const char* fn, const float* d_queries, int m, int k, float max_dist, int min_len, int max_miss, int mode,
              bool force_exact, const FilterLabels& f, int exclude, const Outs& o) {
    int32_t* const group = o.dev<int32_t>(0); int32_t* const hits = o.dev<int32_t>(1); int32_t* const span = o.dev<int32_t>(2);
    int32_t* const q_first = o.dev<int32_t>(3); int32_t* const row_first = o.dev<int32_t>(4); int32_t* const row_last = o.dev<int32_t>(5);
    float* const mean = o.dev<float>(6);
    FilterPlan fp;
    VQ_TRY(filter_prepare(x, fn, f, exclude, true, &fp));
    if (!fp.all && fp.m == 0) {                             // nothing allowed: every slot empty
        set_stats(x, STATS_HOST, 0, 0, 0);
        return outs_empty_placed(x, o);
    }
    VQ_TRY(seq_order_prepare(x));
    const uint32_t* allow = fp.all ? nullptr : fp.bits;
    const int64_t n = x->size, ld = round_up(n, 64);
    const int G = x->n_groups;
    const int nblocks = cdiv(G, GRP_BLOCK), kl = std::min(k, GRP_BLOCK);
    const MatchPlan p = match_plan_env(n, G, x->dim, m, mode, x->near_unit);
    const bool tile = p.fp16 && !force_exact;
    const int64_t W = p.words;
    const unsigned long long cap = (unsigned long long)p.filed_cap;
    const MatchKey key{p.key_m_bits, p.key_d_bits};
    VQ_TRY(x->d_mbits.reserve((int64_t)m * W));
    VQ_TRY(x->d_mw.reserve(2 + (int64_t)G));
    VQ_TRY(x->d_mqe.reserve((int64_t)m + k));
    VQ_TRY(x->d_sekey.reserve((int64_t)G + (int64_t)nblocks * kl));
    VQ_TRY(ensure_gcounters(x));
    MatchCtl* ctl = (MatchCtl*)x->d_mw.p;
    unsigned long long* gkey = (unsigned long long*)(x->d_mw.p + 2);
    float* qe = x->d_mqe; float* sel_dist = qe + m;                      // (the selection writes a distance per slot: unused here)
    uint64_t* ekey = x->d_sekey; uint64_t* partial = ekey + G;
    uint32_t* bits = x->d_mbits;
    const int32_t* sorder = x->d_seq;
    VQ_HIP(hipMemsetAsync(ctl, 0, sizeof(MatchCtl), x->stream));
    VQ_HIP(hipMemsetAsync(gkey, 0xff, (size_t)G * 8, x->stream));
    x->last_match.valid = false;
    if (!tile) {
        VQ_TRY(x->d_dist.reserve((int64_t)p.exact_chunk * ld));
        for (int q0 = 0; q0 < m; q0 += p.exact_chunk) {
            const int cur = std::min(p.exact_chunk, m - q0);
            VQ_TRY(exact_dist(x, false, d_queries + (int64_t)q0 * x->dim, cur, ld));       // always the tiled kernel
            Prof pr(x, I_SELECT);
            hipLaunchKernelGGL(match_threshold_kernel<true>, dim3(cdiv(n, 256), cur), dim3(256), 0, x->stream, x->d_dist, ld, x->rows, n, x->dim,
                               nullptr, max_dist, bits + (int64_t)q0 * W, W, nullptr);
        }
    } else {
        const int64_t q_pad = (int64_t)p.q_tiles * SCAN2_QT;
        VQ_TRY(x->d_q16.reserve(q_pad * x->dim));
        VQ_TRY(x->d_mfiled.reserve(std::min<int64_t>(p.filed_cap, (int64_t)m * n)));
        VQ_TRY(set_dyn_lds(x, (const void*)match_tile_kernel, MATCH_LDS_BYTES));
        const float T = (float)(1.0 - (double)max_dist);
        {
            Prof pr(x, I_RESCORE);
            hipLaunchKernelGGL(match_query_norm_kernel, dim3(m), dim3(64), 0, x->stream, d_queries, x->dim, scan_eps_unit(x->dim) * x->row_norm_max, qe, ctl);
        }
        queries_to_f16(x, d_queries, m, q_pad);
        {
            Prof pr(x, I_MFMA_SCAN);
            hipLaunchKernelGGL(match_tile_kernel, dim3((unsigned)p.tile_grid), dim3(G2_THREADS), MATCH_LDS_BYTES, x->stream, x->d_q16, x->rows16, x->dim, n,
                               p.q_tiles, p.ranges, cdiv(p.ranges, 4), m, T, qe, bits, W, ctl, (unsigned long long*)x->d_mfiled.p, cap);
        }
        {
            Prof pr(x, I_RESCORE);
            hipLaunchKernelGGL(match_patch_kernel, dim3(grid_for(std::min<int64_t>(p.filed_cap, (int64_t)m * n))), dim3(256), 0, x->stream, x->rows, x->dim,
                               d_queries, max_dist, ctl, (const unsigned long long*)x->d_mfiled.p, cap, bits, W);
        }
        {
            Prof pr(x, I_EXACT_DIST);                        // the redo: leaves at once unless the flag is 2
            hipLaunchKernelGGL(match_threshold_kernel<false>, dim3(cdiv(n, 256), m), dim3(256), 0, x->stream, nullptr, 0, x->rows, n, x->dim, d_queries,
                               max_dist, bits, W, ctl);
        }
        x->last_match = {true, m, W, n, (int64_t)cap};
    }
    {
        Prof pr(x, I_SEQ_DP);
        hipLaunchKernelGGL(match_run_kernel, dim3((unsigned)p.run_blocks), dim3(MATCH_RUN_THREADS), 0, x->stream, bits, W, m, x->d_goff, sorder, G,
                           p.diagonals, min_len, max_miss, key, allow, gkey);
    }
    {
        Prof pr(x, I_SELECT);
        hipLaunchKernelGGL(match_final_kernel, dim3(nblocks), dim3(256), 0, x->stream, gkey, G, key, ekey);
        hipLaunchKernelGGL(set_select_block_kernel, dim3(nblocks), dim3(256), 0, x->stream, ekey, G, kl, partial);
        hipLaunchKernelGGL(set_select_merge_kernel, dim3(1), dim3(256), 0, x->stream, partial, (int64_t)nblocks * kl, k, group, sel_dist, nullptr,
                           nullptr);
    }
    {
        Prof pr(x, I_EXACT_DIST);
        hipLaunchKernelGGL(match_score_kernel, dim3(k), dim3(256), 0, x->stream, group, gkey, key, m, bits, W, x->rows, x->dim, d_queries, x->d_goff,
                           sorder, hits, span, q_first, row_first, row_last, mean);
    }
    hipLaunchKernelGGL(match_stats_kernel, dim3(1), dim3(256), 0, x->stream, ekey, G, ctl, cap, p.fp16 && force_exact ? 1 : 0, x->d_gcounters);
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

// ---- library neighbours (knn_neighbors.h) ----
// $VQ_AMD_NEIGHBORS_CHUNK (tests): asked rows per chunk, read per call
int64_t neighbors_chunk_override() {
    const char* e = getenv("VQ_AMD_NEIGHBORS_CHUNK");
    return e ? std::max<int64_t>(0, atoll(e)) : 0;
}

// Refusals, before anything is queued; then the plan.
int neighbors_precheck(vq_index* x, const char* fn, const int64_t* rows, int64_t m, int k, int exclude, int mode, NeighborsPlan* p) {
    VQ_TRY(check_mode(fn, mode));
    VQ_TRY(check_ranks(x, fn));
    if (exclude) VQ_TRY(check_labels(x, fn));
    VQ_CHECK(rows || m == x->size, "%s: rows = NULL asks for every row: m must be the index's size %lld, not %lld", fn, (long long)x->size, (long long)m);
    if (rows)
        for (int64_t i = 0; i < m; ++i)
            VQ_CHECK(rows[i] >= 0 && rows[i] < x->size, "%s: rows[%lld] = %lld, the index holds rows 0 .. %lld", fn, (long long)i, (long long)rows[i],
                     (long long)x->size - 1);
    if (mode != 1) VQ_TRY(refresh_norm_range(x));
    *p = plan_neighbors(x->size, x->dim, m, k, mode, x->near_unit, neighbors_chunk_override());
    if (mode == 2) VQ_CHECK(p->fp16, "%s: the fp16 path needs dim 256, 512 or 768, k <= %d and near-unit rows (0.5 <= |row|^2 <= 2; rows added "
                                     "with normalize=0 are measured)", fn, RV_K_MAX);
    return 0;
}

// rows: host memory or null (every row); d_ids / d_out [m][k] device memory.  Asynchronous on the index's stream.
int neighbors_run(vq_index* x, const int64_t* rows, int64_t m, int k, int exclude, const NeighborsPlan& p, int32_t* d_ids, float* d_out) {
    const int64_t n = x->size;
    const int dim = x->dim;
    const int32_t* group_of = exclude ? x->d_group.p : nullptr;
    const int32_t* list = nullptr;
    if (rows) {                                          // the row list goes up through a pinned staging slot, like the filter lists
        VQ_TRY(x->d_nbrows.reserve(m));
        StageSlot* slot;
        VQ_TRY(stage_slot(x, m, &slot));
        int32_t* h = slot->h;
        for (int64_t i = 0; i < m; ++i) h[i] = (int32_t)rows[i];
        VQ_HIP(hipMemcpyAsync(x->d_nbrows, h, (size_t)m * 4, hipMemcpyHostToDevice, x->stream));
        VQ_HIP(hipEventRecord(slot->ev, x->stream));
        list = x->d_nbrows;
        VQ_TRY(x->d_nbq.reserve(p.chunk_rows * dim));
    }
    VQ_TRY(x->d_nbtag.reserve(p.chunk_rows));
    const EligTag elig{x->d_nbtag, group_of};
    auto rescore = rescore_verify_kernel_t<NB_RESCORE_QPW, RV_KEEP, RV_C, EligTag, NB_RESCAN>;
    if (p.fp16) {
        if (rows) VQ_TRY(x->d_q16.reserve(p.chunk_rows * dim));
        VQ_TRY(x->d_keys.reserve(p.streams * p.chunk_rows * 2));
        VQ_TRY(x->d_flags.reserve(p.chunk_rows));
        VQ_TRY(reserve_fallback(x, (int)p.chunk_rows, k));
        VQ_TRY(ensure_gcounters(x));
        VQ_HIP(hipMemsetAsync(x->d_gcounters, 0, 3 * sizeof(unsigned long long), x->stream));
        VQ_TRY(set_dyn_lds(x, (const void*)neighbors_tile_kernel, NB_LDS_BYTES));
        if (p.rescore == RESCORE_LARGE4) rescore = rescore_verify_kernel_t<NB_RESCORE_QPW, RVL_KEEP, RVL_C, EligTag, NB_RESCAN>;
        if (p.rescore == RESCORE_XLARGE4) rescore = rescore_verify_kernel_t<NB_RESCORE_QPW, RVX_KEEP, RVX_C, EligTag, NB_RESCAN_XL>;
        x->last_scan.valid = false;                      // d_keys is taken
    }
    const float eps_rows = scan_eps_unit(dim) * x->row_norm_max;
    const int rb = 2;                                    // 4 ranges x 8 resident tiles per block of 32 workgroups (knn_scan_fold.h)
    const int range_groups = (p.ranges + (1 << rb) - 1) >> rb;
    const bool one_wg = n <= SEL_SMALL_MAX_N && k <= 256;
    for (int64_t q0 = 0; q0 < m; q0 += p.chunk_rows) {
        const int cur = (int)std::min<int64_t>(p.chunk_rows, m - q0);
        const int64_t qpad = round_up(cur, NB_ROW_TILE);
        const int qt = (int)(qpad / NB_ROW_TILE);
        int32_t* ids0 = d_ids + q0 * k;
        float* out0 = d_out + q0 * k;
        {
            Prof pr(x, I_TO_F16);
            hipLaunchKernelGGL(neighbors_prepare_kernel, dim3((unsigned)std::min<int64_t>(cdiv(qpad, 4), 4096)), dim3(256), 0, x->stream, list, q0, cur,
                               qpad, group_of, x->rows.p, x->rows16.p, dim, x->d_nbtag.p, x->d_nbq.p, p.fp16 && rows ? x->d_q16.p : nullptr);
        }
        const float* qp = rows ? x->d_nbq.p : x->rows + q0 * dim;           // the re-score's and the redo's queries: the fp32 masters
        if (!p.fp16) {
            VQ_TRY(exact_topk(x, n, cur, k, one_wg, x->tie(), ids0, out0, [&](int s0, int c, int64_t ld) {
                VQ_TRY(exact_dist(x, false, qp + (int64_t)s0 * dim, c, ld));
                Prof pr(x, I_SELECT);
                hipLaunchKernelGGL(neighbors_strike_kernel, dim3(c), dim3(256), 0, x->stream, x->d_dist.p, ld, x->d_nbtag + s0,
                                   exclude ? x->d_goff : nullptr, exclude ? x->d_grows : nullptr);
                return 0;
            }));
            Prof pr(x, I_SELECT);
            hipLaunchKernelGGL(neighbors_fix_kernel, dim3(grid_for((int64_t)cur * k)), dim3(256), 0, x->stream, ids0, out0, (int64_t)cur * k);
            continue;
        }
        const uint16_t* a16 = rows ? x->d_q16.p : x->rows16 + q0 * dim;     // every row: the scan copy itself is the resident operand
        {
            Prof pr(x, I_MFMA_SCAN);
            const int qb = 32 >> rb;
            hipLaunchKernelGGL(neighbors_tile_kernel, dim3(range_groups * ((qt + qb - 1) / qb) * 32), dim3(G2_THREADS), NB_LDS_BYTES, x->stream, a16,
                               x->d_nbtag.p, x->rows16.p, group_of, dim, n, cur, qt, p.ranges, range_groups, x->d_keys.p, rb);
        }
        {
            Prof pr(x, I_RESCORE);
            hipLaunchKernelGGL(rescore, dim3(cdiv(cur, p.rescore_qpw)), dim3(256), 0, x->stream, x->d_keys.p, p.streams, qpad, x->rows.p, n, dim, qp, cur, k,
                               ids0, out0, x->d_flags.p, 2, eps_rows, x->tie(), elig);
        }
        // the rows the proof left open are redone exactly under the same eligibility, sized on the device (search_fp16 says how)
        hipLaunchKernelGGL(collect_flags_kernel, dim3(1), dim3(1024), 0, x->stream, x->d_flags.p, cur, x->d_slots.p, x->d_counters.p);
        launch_fallback(x, qp, cur, k, ids0, out0, x->d_counters.p, nullptr, elig);
        hipLaunchKernelGGL(neighbors_stats_kernel, dim3(1), dim3(64), 0, x->stream, x->d_counters.p, x->d_gcounters.p);
        VQ_HIP(hipGetLastError());
        x->last_scan = {true, 2, 2, cur, p.streams, q0};    // the chunk's keys stay in d_keys: the re-score and the redo only read them
    }
    VQ_HIP(hipGetLastError());
    if (!p.fp16) { set_stats(x, STATS_HOST, 0, 0, m); return 0; }
    VQ_HIP(hipMemcpyAsync(x->h_gcounters, x->d_gcounters, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    set_stats(x, STATS_GCOUNTERS);
    return 0;
}

int check_neighbors_args(const char* fn, const vq_index* x, int64_t m, int k, int exclude, int mode, bool arrays) {
    VQ_TRY(require_init());
    VQ_CHECK(x && m >= 0 && m < ((int64_t)1 << 31) && (exclude == 0 || exclude == 1) && (m == 0 || arrays), "%s: bad argument", fn);
    VQ_CHECK(k >= 1 && k <= (mode == 2 ? RV_K_MAX : NB_K_EXACT_MAX), "%s: k = %d, takes 1 <= k <= %d (mode 2: %d)", fn, k, NB_K_EXACT_MAX, RV_K_MAX);
    return 0;
}

// ---- what the search entry points share ----
// One argument check per shape of call.  arrays: every array the call reads or writes is there.
int check_batch_args(const char* fn, const vq_index* x, int nq, int k, bool arrays) {
    VQ_TRY(require_init());
    VQ_CHECK(x && nq >= 0 && k > 0 && k <= 1024 && (nq == 0 || arrays), "%s: bad argument", fn);
    return 0;
}
int check_filtered_args(const char* fn, const vq_index* x, int nq, int k, const int32_t* groups, int32_t n_sel, int exclude, bool arrays) {
    VQ_TRY(require_init());
    VQ_CHECK(x && nq >= 0 && k > 0 && k <= 1024 && n_sel >= 0 && (n_sel == 0 || groups) && (exclude == 0 || exclude == 1) && (nq == 0 || arrays),
             "%s: bad argument", fn);
    return 0;
}
int check_set_args(const char* fn, const vq_index* x, int m, int k, const int32_t* groups, int32_t n_sel, int exclude, bool arrays) {
    VQ_TRY(require_init());
    VQ_CHECK(x && m >= 1 && m <= SET_MAX_M && k > 0 && k <= 1024 && n_sel >= 0 && (n_sel == 0 || groups) && (exclude == 0 || exclude == 1) && arrays,
             "%s: bad argument (1 <= m <= %d, 1 <= k <= 1024)", fn, SET_MAX_M);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_distinct_args(const char* fn, const vq_index* x, int nq, int k, int64_t min_gap, bool arrays) {
    VQ_CHECK(k > 0 && k <= 1024, "%s: k %d outside [1, 1024]", fn, k);
    VQ_CHECK(min_gap >= 0, "%s: min_gap %lld is negative", fn, (long long)min_gap);
    return check_batch_args(fn, x, nq, k, arrays);
}

// (the arguments are judged before the library is asked for its device)
int check_diverse_args(const char* fn, const vq_index* x, int nq, int k, float min_dist, bool arrays) {
    VQ_CHECK(k >= 1 && k <= DIV_MAX_K, "%s: k %d outside [1, %d]", fn, k, DIV_MAX_K);
    VQ_CHECK(min_dist == min_dist, "%s: min_dist is NaN", fn);
    VQ_CHECK(min_dist >= 0.0f, "%s: min_dist %g is negative", fn, (double)min_dist);
    VQ_CHECK(nq >= 1, "%s: nq %d is below 1", fn, nq);
    return check_batch_args(fn, x, nq, k, arrays);
}

int check_sequence_args(const char* fn, const vq_index* x, int m, int k, int64_t min_gap, int64_t max_gap, const int32_t* groups,
                        int32_t n_sel, int exclude, bool arrays) {
    VQ_CHECK(m >= 1 && m <= SEQ_MAX_M && k > 0 && k <= 1024, "%s: bad argument (1 <= m <= %d, 1 <= k <= 1024)", fn, SEQ_MAX_M);
    VQ_CHECK(min_gap >= 1 && min_gap <= max_gap, "%s: the gaps must satisfy 1 <= min_gap <= max_gap (got %lld, %lld)", fn,
             (long long)min_gap, (long long)max_gap);
    VQ_TRY(require_init());
    VQ_CHECK(x && n_sel >= 0 && (n_sel == 0 || groups) && (exclude == 0 || exclude == 1) && arrays, "%s: bad argument", fn);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_span_args(const char* fn, const vq_index* x, int nq, int k, float max_dist, int64_t max_gap, int64_t max_span,
                    const int32_t* groups, int32_t n_sel, int exclude, bool arrays) {
    VQ_CHECK(nq >= 1 && nq <= SPAN_MAX_Q, "%s: nq %d outside [1, %d]", fn, nq, SPAN_MAX_Q);
    VQ_CHECK(k >= 1 && k <= 1024, "%s: k %d outside [1, 1024]", fn, k);
    VQ_CHECK(max_dist == max_dist, "%s: max_dist is NaN", fn);
    VQ_CHECK(max_gap >= 0 && max_span >= 0, "%s: max_gap %lld or max_span %lld is negative", fn, (long long)max_gap, (long long)max_span);
    VQ_CHECK(n_sel >= 0 && (n_sel == 0 || groups) && (exclude == 0 || exclude == 1), "%s: bad filter (n_sel >= 0, exclude 0 or 1)", fn);
    VQ_CHECK(arrays, "%s: a required array is null", fn);
    VQ_TRY(require_init());
    VQ_CHECK(x, "%s: bad argument", fn);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_align_args(const char* fn, const vq_index* x, int m, int k, float max_dist, const int32_t* groups, int32_t n_sel, int exclude,
                     bool arrays) {
    VQ_CHECK(m >= 1 && m <= ALIGN_MAX_M, "%s: m %d outside [1, %d]", fn, m, ALIGN_MAX_M);
    VQ_CHECK(k >= 1 && k <= 1024, "%s: k %d outside [1, 1024]", fn, k);
    VQ_CHECK(max_dist == max_dist, "%s: max_dist is NaN (+inf: no limit)", fn);
    VQ_CHECK(n_sel >= 0 && (n_sel == 0 || groups) && (exclude == 0 || exclude == 1), "%s: bad filter (n_sel >= 0, exclude 0 or 1)", fn);
    VQ_CHECK(arrays, "%s: a required array is null", fn);
    VQ_TRY(require_init());
    VQ_CHECK(x, "%s: bad argument", fn);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_match_args(const char* fn, const vq_index* x, int m, int k, float max_dist, int min_len, int max_miss, int mode,
                     const int32_t* groups, int32_t n_sel, int exclude, bool arrays) {
    VQ_CHECK(m >= 1 && m <= MATCH_MAX_M, "%s: m %d outside [1, %d]", fn, m, MATCH_MAX_M);
    VQ_CHECK(k >= 1 && k <= 1024, "%s: k %d outside [1, 1024]", fn, k);
    VQ_CHECK(max_dist == max_dist, "%s: max_dist is NaN (+inf: every cell hits)", fn);
    VQ_CHECK(min_len >= 1, "%s: min_len %d is below 1", fn, min_len);
    VQ_CHECK(max_miss >= 0, "%s: max_miss %d is negative", fn, max_miss);
    VQ_TRY(check_mode(fn, mode));
    VQ_CHECK(n_sel >= 0 && (n_sel == 0 || groups) && (exclude == 0 || exclude == 1), "%s: bad filter (n_sel >= 0, exclude 0 or 1)", fn);
    VQ_TRY(require_init());
    VQ_CHECK(x && arrays, "%s: bad argument", fn);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_summary_args(const char* fn, const vq_index* x, const int32_t* groups, int32_t n_sel, int k, float max_radius, bool arrays) {
    VQ_CHECK(k >= 1 && k <= SUM_MAX_K && n_sel >= 1, "%s: bad argument (1 <= k <= %d, n_sel >= 1)", fn, SUM_MAX_K);
    VQ_CHECK(max_radius == max_radius, "%s: max_radius is NaN (-inf: no early stop)", fn);
    VQ_TRY(require_init());
    VQ_CHECK(x && groups && arrays, "%s: bad argument", fn);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_compound_args(const char* fn, const vq_index* x, int m, const int32_t* clause_of, float margin, int k, int mode, bool arrays) {
    VQ_CHECK(m >= 1 && m <= CP_MAX_M, "%s: m %d outside [1, %d]", fn, m, CP_MAX_M);
    VQ_CHECK(k >= 1 && k <= 1024, "%s: k %d outside [1, 1024]", fn, k);
    VQ_CHECK(margin == margin, "%s: margin is NaN (-inf: the veto terms strike nothing)", fn);
    VQ_TRY(check_mode(fn, mode));
    VQ_CHECK(clause_of, "%s: clause_of is null", fn);
    int next = 0;                                           // the first clause number not seen yet
    for (int j = 0; j < m; ++j) {
        const int c = clause_of[j];
        if (c == -1) continue;
        VQ_CHECK(c >= 0 && c < m, "%s: clause_of[%d] = %d is neither a clause number in [0, m) nor -1", fn, j, c);
        VQ_CHECK(c >= next - 1, "%s: clause_of[%d] = %d after clause %d: the clause numbers must not decrease", fn, j, c, next - 1);
        VQ_CHECK(c <= next, "%s: clause_of[%d] = %d leaves a gap: clause %d has no term", fn, j, c, next);
        if (c == next) ++next;
    }
    VQ_CHECK(next >= 1, "%s: clause_of holds veto terms only: there is nothing to rank by", fn);
    VQ_TRY(require_init());
    VQ_CHECK(x && arrays, "%s: bad argument", fn);
    return 0;
}

// (the arguments are judged before the library is asked for its device)
int check_segment_args(const char* fn, const vq_index* x, const int32_t* groups, int32_t n_sel, int k, float penalty, int64_t max_len, bool arrays) {
    VQ_CHECK(n_sel >= 1, "%s: n_sel %d: at least one group must be listed", fn, (int)n_sel);
    VQ_CHECK(k >= 1 && k <= SEG_MAX_K, "%s: k %d outside [1, %d]", fn, k, SEG_MAX_K);
    VQ_CHECK(penalty == penalty && penalty >= 0.0f, "%s: penalty must be >= 0 and not NaN", fn);
    VQ_CHECK(max_len >= 0, "%s: max_len %lld is negative (0: no limit)", fn, (long long)max_len);
    VQ_TRY(require_init());
    VQ_CHECK(x && groups && arrays, "%s: bad argument", fn);
    return 0;
}

// ---- the families' call sequences ----
// One function per family, run by both of its entry points: the argument check, the lock, the empty index's answer (no
// candidates: hnsw.py:243-244 returns []), the filter's labels, the family's precheck, the run.  The entry points say where the
// arrays are (Form) and nothing else; what only a host form does is marked `host`.  The output lists name each array's empty value.
OutField out_ids(void* p, int64_t count) { return {p, count, 4, OUT_NONE}; }                    // rows or groups: -1
OutField out_dist(void* p, int64_t count) { return {p, count, 4, OUT_INF}; }                    // distances: +inf
OutField out_zero(void* p, int64_t count, int width = 4) { return {p, count, width, OUT_ZERO}; }  // counts, lengths, masses
OutField out_owned(void* p, int64_t count) { return {p, count, 4, OUT_ZERO, true}; }             // copied back from memory the call names

// vq_index_search's small calls — the reference caller's (one query, k * 2 results: video_search_system.py:297) and small
// batches: the query goes up from pinned staging, the kernels write ids | distances straight into pinned, device-mapped host
// memory, and the ONE wait below is the only host/device round trip — no copy-back commands, no fallback launches unless a
// query was flagged.  (Larger results: scattered 4-byte stores across PCIe lose to one copy.)
bool host_fast_fits(const vq_index* x, int nq, int k) {
    static const bool host_fast = !(getenv("VQ_AMD_HOST_FAST") && atoi(getenv("VQ_AMD_HOST_FAST")) == 0);      // A/B switch
    return host_fast && (int64_t)nq * x->dim * 4 <= ((int64_t)256 << 10) && (int64_t)nq * k * 8 <= ((int64_t)16 << 10);
}
int search_host_fast(vq_index* x, const float* queries, int nq, int k, int mode, int32_t* ids, float* dist) {
    const int64_t count = (int64_t)nq * k;
    VQ_TRY(host_results(x, count * 8));
    VQ_TRY(stage_queries(x, queries, nq));
    int32_t* r_ids = (int32_t*)x->h_res.dev;
    float* r_dist = (float*)(x->h_res.dev + count * 4);
    VQ_TRY(search_dispatch(x, x->d_q, nq, k, mode, r_ids, r_dist, true));
    VQ_HIP(hipStreamSynchronize(x->stream));
    if (x->stats_at == STATS_DEFERRED) {
        stats_from_counters(x);
        if (x->h_counters[0] > 0) {                      // some proof did not close: the exact redo, then one more wait
            launch_fallback(x, x->d_q, nq, k, r_ids, r_dist, x->h_counters.dev);
            VQ_HIP(hipGetLastError());
            VQ_HIP(hipStreamSynchronize(x->stream));
        }
    }
    std::memcpy(ids, x->h_res, (size_t)count * 4);
    std::memcpy(dist, x->h_res + count * 4, (size_t)count * 4);
    return 0;
}

int search_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, int mode, void* ids, void* dist) {
    VQ_TRY(check_batch_args(fn, x, nq, k, queries && ids && dist));
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{2, {out_ids(ids, count), out_dist(dist, count)}};
    if (x->size == 0) return outs_empty(x, form, o);
    if (form != ON_DEVICE && host_fast_fits(x, nq, k)) return search_host_fast(x, (const float*)queries, nq, k, mode, (int32_t*)ids, (float*)dist);
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_dispatch(x, dq, nq, k, mode, o.dev<int32_t>(0), o.dev<float>(1));
    });
}

int grouped_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, int mode, void* groups, void* rows, void* dist) {
    VQ_TRY(check_batch_args(fn, x, nq, k, queries && groups && rows && dist));
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{3, {out_ids(groups, count), out_ids(rows, count), out_dist(dist, count)}};
    if (x->size == 0) return outs_empty(x, form, o);
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_grouped_dispatch(x, dq, nq, k, mode, o.dev<int32_t>(0), o.dev<int32_t>(1), o.dev<float>(2));
    });
}

int distinct_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, int mode, int64_t min_gap, void* ids, void* dist) {
    VQ_TRY(check_distinct_args(fn, x, nq, k, min_gap, queries && ids && dist));
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{2, {out_ids(ids, count), out_dist(dist, count)}};
    if (x->size == 0) return outs_empty(x, form, o);
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_distinct_dispatch(x, dq, nq, k, mode, min_gap, o.dev<int32_t>(0), o.dev<float>(1));
    });
}

int diverse_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, int mode, float min_dist, void* ids, void* dist) {
    const bool host = form != ON_DEVICE;
    VQ_TRY(check_diverse_args(fn, x, nq, k, min_dist, queries && ids && dist));
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{2, {out_ids(ids, count), out_dist(dist, count)}};
    if (x->size == 0) return outs_empty(x, form, o);
    if (host) {                                             // refuse before staging anything
        VQ_TRY(check_mode(fn, mode));
        VQ_TRY(check_ranks(x, fn));
    }
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_diverse_dispatch(x, dq, nq, k, mode, min_dist, o.dev<int32_t>(0), o.dev<float>(1));
    });
}

// the two filtered searches: their host forms' results come back through the pinned buffer
int filtered_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, int mode, const int32_t* groups, int32_t n_sel,
                  int exclude, void* ids, void* dist) {
    const bool host = form != ON_DEVICE;
    VQ_TRY(check_filtered_args(fn, x, nq, k, groups, n_sel, exclude, queries && ids && dist));
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{2, {out_ids(ids, count), out_dist(dist, count)}, COPY_PINNED_FIELDS};
    if (x->size == 0) return outs_empty(x, form, o);
    if (host) VQ_TRY(filter_precheck(x, fn, nq, k, mode, n_sel, exclude));      // refuse before staging anything
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_filtered_dispatch(x, dq, nq, k, mode, groups, n_sel, exclude, o.dev<int32_t>(0), o.dev<float>(1));
    });
}

int grouped_filtered_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, int mode, const int32_t* groups,
                          int32_t n_sel, int exclude, void* groups_out, void* rows, void* dist) {
    const bool host = form != ON_DEVICE;
    VQ_TRY(check_filtered_args(fn, x, nq, k, groups, n_sel, exclude, queries && groups_out && rows && dist));
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{3, {out_ids(groups_out, count), out_ids(rows, count), out_dist(dist, count)}, COPY_PINNED_BLOCK};
    if (x->size == 0) return outs_empty(x, form, o);
    if (host) VQ_TRY(filter_precheck(x, fn, nq, k, mode, n_sel, exclude));      // refuse before staging anything
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_grouped_filtered_dispatch(x, dq, nq, k, mode, groups, n_sel, exclude, o.dev<int32_t>(0), o.dev<int32_t>(1), o.dev<float>(2));
    });
}

int set_call(vq_index* x, const char* fn, Form form, const void* queries, int m, int k, int mode, const int32_t* groups, int32_t n_sel,
             int exclude, void* groups_out, void* dist_out, void* match_rows) {
    VQ_TRY(check_set_args(fn, x, m, k, groups, n_sel, exclude, queries && groups_out && dist_out));
    std::lock_guard<std::mutex> lk(x->mu);
    Outs o{3, {out_ids(groups_out, k), out_dist(dist_out, k), out_ids(match_rows, (int64_t)k * m)}};
    if (x->size == 0) return outs_empty(x, form, o);
    const FilterLabels f = filter_labels(x, groups, n_sel);
    VQ_TRY(set_precheck(x, fn, mode, f));
    return run_form(x, form, (const float*)queries, m, &o, [&](const float* dq) { return search_set_run(x, fn, dq, m, k, mode, f, exclude, o); });
}

int sequence_call(vq_index* x, const char* fn, Form form, const void* steps, int m, int k, int64_t min_gap, int64_t max_gap,
                  const int32_t* groups, int32_t n_sel, int exclude, void* groups_out, void* dist_out, void* chain_rows) {
    VQ_TRY(check_sequence_args(fn, x, m, k, min_gap, max_gap, groups, n_sel, exclude, steps && groups_out && dist_out));
    std::lock_guard<std::mutex> lk(x->mu);
    Outs o{3, {out_ids(groups_out, k), out_dist(dist_out, k), out_ids(chain_rows, (int64_t)k * m)}};
    if (x->size == 0) return outs_empty(x, form, o);
    const FilterLabels f = filter_labels(x, groups, n_sel);
    VQ_TRY(seq_precheck(x, fn, f));
    return run_form(x, form, (const float*)steps, m, &o, [&](const float* dq) {
        return search_sequence_run(x, fn, dq, m, k, min_gap, max_gap, f, exclude, o);
    });
}

int spans_call(vq_index* x, const char* fn, Form form, const void* queries, int nq, int k, float max_dist, int64_t max_gap, int64_t max_span,
               const int32_t* groups, int32_t n_sel, int exclude, void* groups_out, void* dist_out, void* mass_out, void* len_out, void* rows_out) {
    VQ_TRY(check_span_args(fn, x, nq, k, max_dist, max_gap, max_span, groups, n_sel, exclude, queries && groups_out && dist_out));
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)nq * k;
    Outs o{5, {out_ids(groups_out, count), out_dist(dist_out, count), out_zero(mass_out, count, 8), out_zero(len_out, count), out_ids(rows_out, 3 * count)}};
    if (x->size == 0) return outs_empty(x, form, o);
    const FilterLabels f = filter_labels(x, groups, n_sel);
    VQ_TRY(seq_precheck(x, fn, f));
    return run_form(x, form, (const float*)queries, nq, &o, [&](const float* dq) {
        return search_spans_run(x, fn, dq, nq, k, max_dist, max_gap, max_span, f, exclude, o);
    });
}

int align_call(vq_index* x, const char* fn, Form form, const void* clip, int m, int k, float max_dist, const int32_t* groups, int32_t n_sel,
               int exclude, void* groups_out, void* dist_out, void* cost_out, void* rows_out, void* align_out) {
    VQ_TRY(check_align_args(fn, x, m, k, max_dist, groups, n_sel, exclude, clip && groups_out && dist_out));
    std::lock_guard<std::mutex> lk(x->mu);
    Outs o{5, {out_ids(groups_out, k), out_dist(dist_out, k), out_zero(cost_out, k, 8), out_ids(rows_out, 2 * (int64_t)k),
               out_ids(align_out, 2 * (int64_t)k * m)}};
    if (x->size == 0) return outs_empty(x, form, o);
    const FilterLabels f = filter_labels(x, groups, n_sel);
    VQ_TRY(seq_precheck(x, fn, f));
    const AlignShape shape = align_shape(x, f, exclude);
    if (align_out)
        VQ_CHECK((int64_t)m * shape.largest * 4 <= ALIGN_TABLE_MAX_BYTES, "%s: align_out needs m x (rows of the largest allowed group) x 4 B "
                 "<= 1 GiB (m %d, %lld rows): align the clip in pieces", fn, m, (long long)shape.largest);
    return run_form(x, form, (const float*)clip, m, &o, [&](const float* dq) {
        return align_clip_run(x, fn, dq, m, k, max_dist, f, exclude, shape, o);
    });
}

int summarize_call(vq_index* x, const char* fn, Form form,const int32_t* groups, int32_t n_sel, int k, float max_radius, void* rows_out,
                   void* radius_out, void* members_out) {
    VQ_TRY(check_summary_args(fn, x, groups, n_sel, k, max_radius, rows_out && radius_out));
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t count = (int64_t)n_sel * k;
    Outs o{3, {out_ids(rows_out, count), out_dist(radius_out, count), out_zero(members_out, count)}};
    if (x->size == 0) return outs_empty(x, form, o);
    VQ_TRY(sum_precheck(x, fn, groups, n_sel));
    return run_form(x, form, nullptr, 0, &o, [&](const float*) {
        return summarize_run(x, fn, groups, n_sel, k, max_radius, o.dev<int32_t>(0), o.dev<float>(1), o.dev<int32_t>(2));
    });
}

int segment_call(vq_index* x, const char* fn, Form form, const int32_t* groups, int32_t n_sel, int k, float penalty, int64_t max_len,
                 void* count_out, void* first_out, void* last_out, void* len_out, void* spread_out, void* show_out, void* mean_spread_out) {
    VQ_TRY(check_segment_args(fn, x, groups, n_sel, k, penalty, max_len, count_out && first_out && last_out && len_out && spread_out));
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t slots = (int64_t)n_sel * k;
    Outs o{7, {out_zero(count_out, n_sel), out_ids(first_out, slots), out_ids(last_out, slots), out_zero(len_out, slots), out_dist(spread_out, slots),
               out_ids(show_out, slots), out_dist(mean_spread_out, n_sel)}};
    if (x->size == 0) return outs_empty(x, form, o);
    std::vector<int64_t> len;
    VQ_TRY(seg_precheck(x, fn, groups, n_sel, k, max_len, &len));
    return run_form(x, form, nullptr, 0, &o, [&](const float*) {
        return segment_run(x, fn, groups, n_sel, len, k, penalty, max_len, o.dev<int32_t>(0), o.dev<int32_t>(1), o.dev<int32_t>(2), o.dev<int32_t>(3),
                           o.dev<float>(4), o.dev<int32_t>(5), o.dev<float>(6));
    });
}

// An empty index: the labelling and clustering calls return 0 and write nothing.  The host form's row answers come back from
// where label_run left them (its scratch in d_lw), not from a piece of the block.
int label_call(vq_index* x, const char* fn, Form form, const void* prompts, int P, int mode, float max_dist, void* row_label, void* row_dist, int m,
               void* group_tags, void* group_votes, void* group_show_rows, void* group_unlabelled) {
    const bool host = form != ON_DEVICE, groups = group_tags != nullptr;
    VQ_TRY(check_label_args(fn, x, prompts, P, max_dist, m, groups, group_votes && group_show_rows && group_unlabelled));
    std::lock_guard<std::mutex> lk(x->mu);
    bool in_range = true;                                   // every |p|^2 inside what the fp16 bound covers
    if (host) VQ_TRY(queries_in_range(fn, "prompt", (const float*)prompts, P, x->dim, &in_range));
    if (x->size == 0) {
        set_stats(x, STATS_HOST, 0, 0, 0);
        return 0;
    }
    VQ_TRY(label_precheck(x, fn, mode, groups));
    const int64_t n = x->size, G = groups ? x->n_groups : 0, gm = G * m;
    Outs o{6, {out_owned(row_label, n), out_owned(row_dist, n), out_ids(group_tags, gm), out_zero(groups ? group_votes : nullptr, gm),
               out_ids(groups ? group_show_rows : nullptr, gm), out_zero(groups ? group_unlabelled : nullptr, G)}};
    return run_form(x, form, (const float*)prompts, P, &o, [&](const float* dq) {
        int32_t* lab; float* best;
        VQ_TRY(label_run(x, dq, P, mode, !in_range, max_dist, o.dev<int32_t>(0), o.dev<float>(1), m, o.dev<int32_t>(2), o.dev<int32_t>(3),
                         o.dev<int32_t>(4), o.dev<int32_t>(5), &lab, &best));
        o.f[0].dev = lab; o.f[1].dev = best;
        return 0;
    });
}

// The host form's results all live in memory the call has anyway: the centroids in d_q, as the label call's prompts do, the
// rest in the cluster scratch.  It also reports the iterations it ran and their changed counts, which the device form never reads.
int cluster_call(vq_index* x, const char* fn, Form form, const void* init, const int32_t* init_rows, int P, int iters, int mode, void* centroids,
                 void* row_label, void* row_dist, void* counts, void* show_rows, int* iterations, int32_t* changed) {
    const bool host = form != ON_DEVICE;
    VQ_TRY(check_cluster_args(fn, x, init, init_rows, P, iters, centroids && counts && show_rows && (iterations || !host)));
    std::lock_guard<std::mutex> lk(x->mu);
    bool in_range = true;                                   // every |c|^2 inside what the fp16 bound covers
    if (host && init) VQ_TRY(queries_in_range(fn, "initial centroid", (const float*)init, P, x->dim, &in_range));
    if (x->size == 0) {
        set_stats(x, STATS_HOST, 0, 0, 0);
        return 0;
    }
    const int64_t n = x->size, words = (int64_t)P * x->dim;
    VQ_CHECK(P <= n, "%s: %d clusters for an index of %lld rows", fn, P, (long long)n);
    if (host && init_rows)
        for (int j = 0; j < P; ++j)
            VQ_CHECK(init_rows[j] >= 0 && init_rows[j] < n, "%s: init_rows[%d] = %d outside [0, %lld)", fn, j, (int)init_rows[j], (long long)n);
    VQ_TRY(cluster_precheck(x, fn, mode));
    ClusterBufs b;
    VQ_TRY(cluster_reserve(x, P, &b));
    if (host && x->h_clchanged.cap < iters) {               // (the device form never writes there: nothing in flight uses it)
        VQ_HIP(hipStreamSynchronize(x->stream));
        VQ_TRY(x->h_clchanged.reserve(iters, CL_MAX_ITER));
    }
    if (host) VQ_TRY(x->d_q.reserve(words));
    float* const C = host ? x->d_q.p : (float*)centroids;
    if (host && init) {
        VQ_TRY(stage_queries(x, (const float*)init, P));
    } else if (init) {
        if (init != centroids) VQ_HIP(hipMemcpyAsync(C, init, (size_t)words * 4, hipMemcpyDeviceToDevice, x->stream));
    } else {
        if (host) {                                         // the row list goes up into b.show (free until the show rows are written)
            StageSlot* slot;
            VQ_TRY(stage_slot(x, P, &slot));
            std::memcpy(slot->h, init_rows, (size_t)P * 4);
            VQ_HIP(hipMemcpyAsync(b.show, slot->h.p, (size_t)P * 4, hipMemcpyHostToDevice, x->stream));
            VQ_HIP(hipEventRecord(slot->ev, x->stream));
            init_rows = b.show;
        }
        hipLaunchKernelGGL(cluster_gather_kernel, dim3(P), dim3(256), 0, x->stream, x->rows, n, x->dim, init_rows, C);
    }
    Outs o{5, {out_owned(centroids, words), out_owned(row_label, n), out_owned(row_dist, n), out_owned(counts, P), out_owned(show_rows, P)}};
    o.f[0].dev = C;
    o.f[1].dev = host || !row_label ? b.lab : row_label;
    o.f[2].dev = host || !row_dist ? (void*)b.best : row_dist;
    o.f[3].dev = host ? b.counts : counts;
    o.f[4].dev = host ? b.show : show_rows;
    std::vector<int32_t> ch(host ? (size_t)iters : 0);
    int T = 0;
    VQ_TRY(cluster_run(x, b, C, P, iters, mode, !in_range, o.dev<int32_t>(1), o.dev<float>(2), o.dev<int32_t>(3), o.dev<int32_t>(4),
                       host ? ch.data() : nullptr, &T));
    VQ_TRY(outs_return(x, form, o));
    if (host) {
        *iterations = T;
        if (changed) std::copy(ch.begin(), ch.begin() + T, changed);
    }
    return 0;
}

int compound_call(vq_index* x, const char* fn, Form form, const void* terms, int m, const int32_t* clause_of, float margin, int k, int mode,
                  void* ids, void* dist, void* term_dist) {
    VQ_TRY(check_compound_args(fn, x, m, clause_of, margin, k, mode, terms && ids && dist));
    std::lock_guard<std::mutex> lk(x->mu);
    bool in_range = true;                                   // every |q|^2 inside what the fp16 bound covers
    if (form != ON_DEVICE) VQ_TRY(queries_in_range(fn, "term", (const float*)terms, m, x->dim, &in_range));
    Outs o{3, {out_ids(ids, k), out_dist(dist, k), out_dist(term_dist, (int64_t)k * m)}};
    if (x->size == 0) return outs_empty(x, form, o);
    VQ_TRY(compound_precheck(x, fn, k, mode));
    return run_form(x, form, (const float*)terms, m, &o, [&](const float* dq) {
        return compound_run(x, dq, m, clause_of, margin, k, mode, !in_range, o.dev<int32_t>(0), o.dev<float>(1), o.dev<float>(2));
    });
}

// the seven result arrays of a shared-footage search, [k] each
int match_call(vq_index* x, const char* fn, Form form, const void* queries, int m, int k, float max_dist, int min_len, int max_miss, int mode,
               const int32_t* groups, int32_t n_sel, int exclude, void* groups_out, void* hits_out, void* span_out, void* q_first_out,
               void* row_first_out, void* row_last_out, void* mean_dist_out) {
    Outs o{7, {out_ids(groups_out, k), out_zero(hits_out, k), out_zero(span_out, k), out_ids(q_first_out, k), out_ids(row_first_out, k),
               out_ids(row_last_out, k), out_dist(mean_dist_out, k)}};
    VQ_TRY(check_match_args(fn, x, m, k, max_dist, min_len, max_miss, mode, groups, n_sel, exclude, queries && o.given(7)));
    std::lock_guard<std::mutex> lk(x->mu);
    if (x->size == 0) return outs_empty(x, form, o);
    const FilterLabels f = filter_labels(x, groups, n_sel);
    VQ_TRY(match_precheck(x, fn, m, mode, f));
    // (a query outside the range is not refused here; the sum as the device takes it matters only at the range's very edge,
    //  where either path is exact)
    bool in_range = true;
    if (form != ON_DEVICE) VQ_TRY(queries_in_range(fn, nullptr, (const float*)queries, m, x->dim, &in_range));
    return run_form(x, form, (const float*)queries, m, &o, [&](const float* dq) {
        return match_run(x, fn, dq, m, k, max_dist, min_len, max_miss, mode, !in_range, f, exclude, o);
    });
}

int neighbors_call(vq_index* x, const char* fn, Form form, const int64_t* rows, int64_t m, int k, int exclude, int mode, void* ids, void* dist) {
    VQ_TRY(check_neighbors_args(fn, x, m, k, exclude, mode, ids && dist));
    std::lock_guard<std::mutex> lk(x->mu);
    NeighborsPlan p;
    VQ_TRY(neighbors_precheck(x, fn, rows, m, k, exclude, mode, &p));
    if (m == 0) return 0;
    Outs o{2, {out_ids(ids, m * k), out_dist(dist, m * k)}};
    return run_form(x, form, nullptr, 0, &o, [&](const float*) { return neighbors_run(x, rows, m, k, exclude, p, o.dev<int32_t>(0), o.dev<float>(1)); });
}

}  // namespace

// vq_comm.hip: this rank's part of a row-sharded search, on the index's stream (returned so that the exchange is
// enqueued behind it).
namespace vq {
hipStream_t index_stream(vq_index* x) {
    std::lock_guard<std::mutex> lk(x->mu);
    return x->stream;
}
int index_search_local(vq_index* x, const float* d_queries, int nq, int k, int mode, int32_t* d_ids, float* d_dist,
                       hipStream_t* stream_out, int64_t* size_out) {
    std::lock_guard<std::mutex> lk(x->mu);
    *stream_out = x->stream;
    *size_out = x->size;
    if (x->size == 0) return fill_empty(x, (int64_t)nq * k, d_ids, nullptr, d_dist);
    return search_dispatch(x, d_queries, nq, k, mode, d_ids, d_dist);
}
}  // namespace vq

extern "C" {

int vq_index_create(int dim, vq_index** out) {
    VQ_TRY(require_init());
    VQ_CHECK(out && dim > 0 && dim % 4 == 0 && dim <= 4096, "vq_index_create: dim %d must be a positive multiple of 4", dim);
    vq_index* x = new vq_index();
    x->dim = dim;
    x->scan_switches = scan_switches_from_env();
    // a scan kind this build does not carry is refused here, not at the first search (an A/B run against the wrong library)
    const ScanPlan probe = plan_scan(dim, 1, 1, 1, x->scan_switches, SCAN_DIAG_BUILD, SCAN_EXPERIMENTS_BUILD);
    if (probe.err) { delete x; return fail(probe.err, "vq_index_create: %s", probe.msg); }
    hipError_t e = hipStreamCreateWithFlags(&x->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete x; return fail(VQ_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e)); }
    x->stream = x->own_stream;
    *out = x;
    return 0;
}

// plan_scan's answer for this build and this process's environment; needs no device
int vq_debug_scan_plan(int dim, int64_t n, int nq, int k, int force_scan, vq_scan_plan* out) {
    VQ_CHECK(out && dim > 0 && dim % GEMM_BK == 0 && n >= 1 && n < ((int64_t)1 << 31) && nq >= 1 && k >= 1 && k <= RV_K_MAX,
             "vq_debug_scan_plan: the fp16 search takes dim %% %d == 0, 1 <= n < 2^31, nq >= 1, 1 <= k <= %d", GEMM_BK, RV_K_MAX);
    ScanSwitches sw = scan_switches_from_env();
    if (force_scan) sw.scan = (force_scan == 1 || force_scan == 2 || force_scan == 4 || (force_scan >= 51 && force_scan <= 53)) ? force_scan : SCAN_FOLD;
    const ScanPlan p = plan_scan(dim, n, nq, k, sw, SCAN_DIAG_BUILD, SCAN_EXPERIMENTS_BUILD);
    if (p.err) return fail(p.err, "%s", p.msg);
    const int cur = (int)std::min<int64_t>(p.q_chunk, nq);
    const ScanGrid g = scan_grid(p, cur);
    *out = vq_scan_plan{p.scan, p.QT, p.RANGE, p.n_pad, p.streams, p.ranges, p.q_chunk, n_chunks(p, nq), p.nqg, p.fused_q, p.rb, p.scan_lds,
                        p.rescore, p.rescore_qpw, p.rescore_lds, p.layout, p.rescore_files_flags, q_pad(p, cur), q_tiles(p, cur), g.x, g.y,
                        rescore_grid(p, cur)};
    return 0;
}

int64_t vq_debug_scan_row_of(int layout, int64_t stream, int local) {
    if (stream < 0 || local < 0 || local >= SCAN_STREAM_ROWS) return -1;
    return layout == 1 ? scan_row_of(stream, local) : layout == 2 ? scan2_row_of(stream, local) : layout == 3 ? scan3_row_of(stream, local) : -1;
}

// the last chunk's keys, [cur][streams][2], gathered on the host through the offset functions the re-score kernels read them with
int vq_index_debug_read_scan_keys(vq_index* x, int64_t* info, uint32_t* keys, int64_t capacity) {
    VQ_CHECK(x && info, "vq_index_debug_read_scan_keys: null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    const vq_index::LastScan& s = x->last_scan;
    if (!s.valid) return fail(VQ_ERR_STATE, "vq_index_debug_read_scan_keys: no fp16 search has run on this handle since its rows last changed");
    info[0] = s.q0; info[1] = s.cur; info[2] = s.layout; info[3] = s.streams; info[4] = s.masked;
    if (!keys) return 0;
    const int64_t want = (int64_t)s.cur * s.streams * 2;
    VQ_CHECK(capacity >= want, "vq_index_debug_read_scan_keys: %lld words for %d queries x %lld streams x 2", (long long)capacity, s.cur, (long long)s.streams);
    // every layout keeps a query's keys inside the first round_up(cur, 16) query slots
    const int64_t words = round_up((int64_t)s.cur, 16) * s.streams * 2;
    VQ_CHECK(words <= x->d_keys.cap, "vq_index_debug_read_scan_keys: the key buffer holds %lld words, the last scan wrote %lld", (long long)x->d_keys.cap, (long long)words);
    std::vector<uint32_t> raw((size_t)words);
    VQ_HIP(hipStreamSynchronize(x->stream));
    VQ_HIP(hipMemcpy(raw.data(), x->d_keys, (size_t)words * 4, hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < s.cur; ++q)
        for (int64_t st = 0; st < s.streams; ++st) {
            const size_t at = s.layout == 3 ? scan3_key_index(st, q, s.streams) : batch_key_index(st, q, s.streams);
            keys[(q * s.streams + st) * 2] = raw[at];
            keys[(q * s.streams + st) * 2 + 1] = raw[at + 1];
        }
    return 0;
}

// Pass 2 alone, on a key table the caller wrote: the plan and the launch_rescore call of search_fp16, nothing in front of them
// (no conversion, no scan) and nothing behind (no collect_flags_kernel, no fallback).  The table goes into d_keys through the
// offset functions vq_index_debug_read_scan_keys gathers through; the query slots from nq to q_pad hold "no row".
int vq_index_debug_rescore(vq_index* x, const float* queries, int nq, int k, const uint32_t* keys, int64_t capacity, int32_t* ids,
                           float* dist, int32_t* flags) {
    static const char* fn = "vq_index_debug_rescore";
    VQ_TRY(check_batch_args(fn, x, nq, k, queries && keys && ids && dist && flags));
    VQ_CHECK(nq >= 1, "%s: no query", fn);
    std::lock_guard<std::mutex> lk(x->mu);
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(refresh_norm_range(x));
    VQ_CHECK(x->dim % GEMM_BK == 0 && k <= RV_K_MAX && x->size >= 1 && x->near_unit, "%s: the fp16 search needs dim %% 64 == 0, k <= %d, "
             "a non-empty index and near-unit rows (0.5 <= |row|^2 <= 2)", fn, RV_K_MAX);
    const ScanPlan p = plan_scan(x->dim, x->size, nq, k, x->scan_switches, SCAN_DIAG_BUILD, SCAN_EXPERIMENTS_BUILD);
    if (p.err) return fail(p.err, "%s", p.msg);
    VQ_CHECK(nq <= p.q_chunk, "%s: %d queries do not fit one chunk of %lld", fn, nq, (long long)p.q_chunk);
    const int64_t want = (int64_t)nq * p.streams * 2, count = (int64_t)nq * k;
    VQ_CHECK(capacity >= want, "%s: %lld words for %d queries x %lld streams x 2", fn, (long long)capacity, nq, (long long)p.streams);
    const int64_t qpad = q_pad(p, nq), words = qpad * p.streams * 2;      // every layout: q_pad query slots of streams key pairs (q_pad % 16 == 0)
    VQ_TRY(x->d_keys.reserve(p.streams * p.q_chunk * 2));
    VQ_CHECK(words <= x->d_keys.cap, "%s: the key buffer holds %lld words, the table takes %lld", fn, (long long)x->d_keys.cap, (long long)words);
    VQ_TRY(x->d_flags.reserve(qpad));
    VQ_TRY(x->d_slots.reserve(round_up(nq, 1024)));
    VQ_TRY(ensure_counters(x));
    Outs o{3, {out_ids(ids, count), out_dist(dist, count), out_owned(flags, nq)}};
    VQ_TRY(outs_place(x, HOST_PINNED, &o));
    o.f[2].dev = x->d_flags.p;
    const float no_row = -3.0e38f;                                       // what the scans write for a row past the end
    std::vector<uint32_t> raw((size_t)words, __builtin_bit_cast(uint32_t, no_row));
    for (int64_t q = 0; q < nq; ++q)
        for (int64_t st = 0; st < p.streams; ++st) {
            const size_t at = p.layout == 3 ? scan3_key_index(st, q, p.streams) : batch_key_index(st, q, p.streams);
            raw[at] = keys[(q * p.streams + st) * 2];
            raw[at + 1] = keys[(q * p.streams + st) * 2 + 1];
        }
    x->last_scan.valid = false;
    VQ_HIP(hipStreamSynchronize(x->stream));
    VQ_HIP(hipMemcpy(x->d_keys, raw.data(), (size_t)words * 4, hipMemcpyHostToDevice));
    VQ_TRY(stage_queries(x, queries, nq));
    x->last_scan = {true, false, p.layout, nq, p.streams, 0};
    VQ_TRY(launch_rescore(x, p, x->d_q, nq, k, o.dev<int32_t>(0), o.dev<float>(1), x->d_flags, x->d_counters));
    VQ_HIP(hipGetLastError());
    return outs_return(x, HOST_PINNED, o);
}

// fallback_plan's answer; needs no device
int vq_debug_fallback_plan(int64_t n, int nq, int k, int64_t* out) {
    VQ_CHECK(out && n >= 1 && n < ((int64_t)1 << 31) && nq >= 1 && k >= 1 && k <= FB_KMAX,
             "vq_debug_fallback_plan: the exact redo takes 1 <= n < 2^31, nq >= 1, 1 <= k <= %d", FB_KMAX);
    const FallbackPlan f = fallback_plan(n, nq, k);
    out[0] = f.fast_splits; out[1] = f.fast_rows; out[2] = f.splits; out[3] = f.rows; out[4] = f.round_q; out[5] = f.partial;
    return 0;
}

// Pass 3 alone, on flags the caller wrote: collect_flags_kernel and the launch_fallback call of search_fp16, nothing in front of
// them (no scan, no re-score: the caller's ids / dist stand in for the fast path's answer).  With a filter, the masked kernel
// under the bitmap filter_prepare builds for the masked fp16 path.
int vq_index_debug_fallback(vq_index* x, const float* queries, int nq, int k, const int32_t* flags, const int32_t* groups, int32_t n_sel,
                            int exclude, int32_t* ids, float* dist, int32_t* counters) {
    static const char* fn = "vq_index_debug_fallback";
    VQ_TRY(check_batch_args(fn, x, nq, k, queries && flags && ids && dist && counters));
    VQ_CHECK(nq >= 1, "%s: no query", fn);
    VQ_CHECK(!groups ? n_sel == 0 : n_sel >= 0 && (exclude == 0 || exclude == 1), "%s: bad filter (%d labels, exclude %d)", fn, (int)n_sel, exclude);
    std::lock_guard<std::mutex> lk(x->mu);
    VQ_TRY(check_ranks(x, fn));
    VQ_TRY(refresh_norm_range(x));
    VQ_CHECK(x->dim % GEMM_BK == 0 && k <= RV_K_MAX && x->size >= 1 && x->near_unit, "%s: the fp16 search needs dim %% 64 == 0, k <= %d, "
             "a non-empty index and near-unit rows (0.5 <= |row|^2 <= 2)", fn, RV_K_MAX);
    const int64_t count = (int64_t)nq * k;
    VQ_TRY(x->d_flags.reserve(nq));
    VQ_TRY(reserve_fallback(x, nq, k));
    Outs o{3, {out_ids(ids, count), out_dist(dist, count), out_owned(counters, FB_NCOUNTERS)}};
    VQ_TRY(outs_place(x, HOST_PINNED, &o));
    o.f[2].dev = x->d_counters.p;
    GroupMask gm{};
    bool masked = false;
    if (groups) {
        FilterPlan p;
        VQ_TRY(filter_prepare(x, fn, filter_labels(x, groups, n_sel), exclude, true, &p));
        VQ_CHECK(p.all || p.m > 0, "%s: the filter allows no row", fn);
        masked = !p.all;                                                  // an empty exclude list: the unmasked kernel, as the search takes it
        gm = GroupMask{x->d_group, x->d_sgroup, p.bits};
    }
    VQ_HIP(hipMemcpyAsync(o.f[0].dev, ids, (size_t)count * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipMemcpyAsync(o.f[1].dev, dist, (size_t)count * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipMemcpyAsync(x->d_flags, flags, (size_t)nq * 4, hipMemcpyHostToDevice, x->stream));
    VQ_TRY(stage_queries(x, queries, nq));
    hipLaunchKernelGGL(collect_flags_kernel, dim3(1), dim3(1024), 0, x->stream, x->d_flags, nq, x->d_slots, x->d_counters);
    launch_fallback(x, x->d_q, nq, k, o.dev<int32_t>(0), o.dev<float>(1), x->d_counters, masked ? &gm : nullptr);
    VQ_HIP(hipGetLastError());
    return outs_return(x, HOST_PINNED, o);
}

int vq_index_debug_read_group_best(vq_index* x, int64_t* info, float* best, int64_t capacity) {
    VQ_CHECK(x && info, "vq_index_debug_read_group_best: null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    const vq_index::LastGroupScan& s = x->last_gscan;
    if (!s.valid) return fail(VQ_ERR_STATE, "vq_index_debug_read_group_best: no fp16 grouped search has run on this handle since its rows last changed");
    info[0] = s.q0; info[1] = s.cur; info[2] = s.n_groups;
    if (!best) return 0;
    const int64_t want = (int64_t)s.cur * s.n_groups;
    VQ_CHECK(capacity >= want, "vq_index_debug_read_group_best: %lld floats for %d queries x %d groups", (long long)capacity, s.cur, (int)s.n_groups);
    VQ_CHECK(want <= x->d_gbest.cap, "vq_index_debug_read_group_best: the buffer holds %lld words, the last scan wrote %lld", (long long)x->d_gbest.cap, (long long)want);
    std::vector<uint32_t> raw((size_t)want);
    VQ_HIP(hipStreamSynchronize(x->stream));
    VQ_HIP(hipMemcpy(raw.data(), x->d_gbest, (size_t)want * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < want; ++i) best[i] = key_score(raw[(size_t)i]);      // key 0 = no row seen -> NaN (all bits set)
    return 0;
}

// which group-max scan left the record vq_index_debug_read_group_best hands out: info = {kind, chunks, tile_chunks} (LastGroupScan)
int vq_index_debug_group_scan_kind(vq_index* x, int64_t* info) {
    VQ_CHECK(x && info, "vq_index_debug_group_scan_kind: null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    const vq_index::LastGroupScan& s = x->last_gscan;
    if (!s.valid) return fail(VQ_ERR_STATE, "vq_index_debug_group_scan_kind: no fp16 group-max scan has run on this handle since its rows last changed");
    info[0] = s.kind; info[1] = s.chunks; info[2] = s.tile_chunks;
    return 0;
}

// label_tile_kernel's parts [ranges][5][n_pad] as it wrote them
int vq_index_debug_read_label_parts(vq_index* x, int64_t* info, uint32_t* parts, int64_t capacity) {
    static const char* fn = "vq_index_debug_read_label_parts";
    VQ_CHECK(x && info, "%s: null argument", fn);
    std::lock_guard<std::mutex> lk(x->mu);
    const vq_index::LastLabel& s = x->last_label;
    if (!s.valid) return fail(VQ_ERR_STATE, "%s: no labelling call has taken the tile path on this handle since its rows last changed", fn);
    int32_t ctl[4];
    VQ_HIP(hipStreamSynchronize(x->stream));
    VQ_HIP(hipMemcpy(ctl, x->d_lw, sizeof ctl, hipMemcpyDeviceToHost));
    if (ctl[1] != 0) return fail(VQ_ERR_STATE, "%s: the last labelling call was flagged (a prompt outside the bound's range): the redo answered it", fn);
    info[0] = s.n; info[1] = s.n_pad; info[2] = s.ranges; info[3] = s.P;
    if (!parts) return 0;
    const int64_t want = (int64_t)s.ranges * LABEL_PART_WORDS * s.n_pad;
    VQ_CHECK(capacity >= want, "%s: %lld words for %d ranges x %d x %lld rows", fn, (long long)capacity, s.ranges, LABEL_PART_WORDS, (long long)s.n_pad);
    VQ_CHECK(want <= x->d_lparts.cap, "%s: the buffer holds %lld words, the last call wrote %lld", fn, (long long)x->d_lparts.cap, (long long)want);
    VQ_HIP(hipMemcpy(parts, x->d_lparts, (size_t)want * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the final bit table [m][W], the first min(cursor, cap) filed pairs ((query << 32) | row) and the control words of the last
// shared-footage call that took the tile path
int vq_index_debug_read_match_bits(vq_index* x, int64_t* info, uint32_t* bits, int64_t bits_capacity, uint64_t* filed, int64_t filed_capacity) {
    static const char* fn = "vq_index_debug_read_match_bits";
    VQ_CHECK(x && info, "%s: null argument", fn);
    std::lock_guard<std::mutex> lk(x->mu);
    const vq_index::LastMatch& s = x->last_match;
    if (!s.valid) return fail(VQ_ERR_STATE, "%s: no shared-footage call has taken the tile path on this handle since its rows last changed", fn);
    MatchCtl ctl;
    VQ_HIP(hipStreamSynchronize(x->stream));
    VQ_HIP(hipMemcpy(&ctl, x->d_mw, sizeof ctl, hipMemcpyDeviceToHost));
    info[0] = s.m; info[1] = s.W; info[2] = s.n; info[3] = (int64_t)ctl.cursor; info[4] = ctl.flag; info[5] = s.cap;
    const int64_t nbits = (int64_t)s.m * s.W, nfiled = std::min<int64_t>((int64_t)ctl.cursor, s.cap);
    if (bits) {
        VQ_CHECK(bits_capacity >= nbits, "%s: %lld words for %d queries x %lld words", fn, (long long)bits_capacity, s.m, (long long)s.W);
        VQ_CHECK(nbits <= x->d_mbits.cap, "%s: the bit table holds %lld words, the last call wrote %lld", fn, (long long)x->d_mbits.cap, (long long)nbits);
        VQ_HIP(hipMemcpy(bits, x->d_mbits, (size_t)nbits * 4, hipMemcpyDeviceToHost));
    }
    if (filed && nfiled > 0) {
        VQ_CHECK(filed_capacity >= nfiled, "%s: %lld entries for %lld filed pairs", fn, (long long)filed_capacity, (long long)nfiled);
        VQ_CHECK(nfiled <= x->d_mfiled.cap, "%s: the filed list holds %lld entries, the last call filed %lld", fn, (long long)x->d_mfiled.cap, (long long)nfiled);
        VQ_HIP(hipMemcpy(filed, x->d_mfiled, (size_t)nfiled * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

int vq_index_destroy(vq_index* x) {
    if (!x) return 0;
    if (x->stream) (void)hipStreamSynchronize(x->stream);
    if (x->own_stream) (void)hipStreamDestroy(x->own_stream);
    for (auto& ev : x->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (auto ev : x->pool) (void)hipEventDestroy(ev);
    delete x;
    return 0;
}

int vq_index_size(vq_index* x, int64_t* n) {
    VQ_CHECK(x && n, "vq_index_size: null argument");
    *n = x->size;
    return 0;
}

int vq_index_clear(vq_index* x) {
    VQ_CHECK(x, "vq_index_clear: null handle");
    std::lock_guard<std::mutex> lk(x->mu);
    x->size = 0;
    x->rows_changed();
    if (x->d_norm_range) VQ_TRY(init_norm_range(x));
    x->norm_dirty = false; x->near_unit = true; x->row_norm_max = 1.0f;
    x->rank_n = 0;
    x->group_n = 0; x->n_groups = 0; x->h_goff.clear();
    x->pos_n = 0; x->seq_n = 0;
    return 0;
}

int vq_index_set_id_ranks(vq_index* x, const int32_t* rank_of_row, int64_t n) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || rank_of_row), "vq_index_set_id_ranks: bad argument");
    std::lock_guard<std::mutex> lk(x->mu);
    x->seq_n = 0;                                                // the (position, tie) order follows the ties
    if (n == 0) { x->rank_n = 0; return 0; }                     // back to row order
    VQ_CHECK(n == x->size, "vq_index_set_id_ranks: %lld ranks for an index of %lld rows", (long long)n, (long long)x->size);
    // a permutation of 0..n-1, checked here: the kernels index two arrays with these values
    std::vector<int32_t> inv((size_t)n, -1);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t t = rank_of_row[r];
        VQ_CHECK(t >= 0 && t < n && inv[(size_t)t] < 0, "vq_index_set_id_ranks: rank_of_row is not a permutation of 0..%lld "
                 "(row %lld holds %d)", (long long)n - 1, (long long)r, (int)t);
        inv[(size_t)t] = (int32_t)r;
    }
    if (2 * n > x->d_rank.cap) {                                    // rank [cap] | rank_inv [cap]
        VQ_HIP(hipStreamSynchronize(x->stream));                   // a search in flight may still read the old arrays
        x->d_rank.release(); x->d_rank_inv = nullptr; x->rank_n = 0;
        const int64_t cap = round_up(std::max<int64_t>(n, x->cap), 1024);
        hipError_t e = hipMalloc((void**)&x->d_rank.p, (size_t)cap * 8);
        if (e != hipSuccess) return fail(VQ_ERR_OOM, "vq_index_set_id_ranks: hipMalloc failed: %s", hipGetErrorString(e));
        x->d_rank_inv = x->d_rank + cap;
        x->d_rank.cap = 2 * cap;
    }
    VQ_HIP(hipMemcpyAsync(x->d_rank, rank_of_row, (size_t)n * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipMemcpyAsync(x->d_rank_inv, inv.data(), (size_t)n * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));                       // `inv` is this frame's, `rank_of_row` the caller's
    x->rank_n = n;
    return 0;
}

int vq_index_set_groups(vq_index* x, const int32_t* group_of_row, int64_t n, int32_t n_groups) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || group_of_row), "vq_index_set_groups: bad argument");
    std::lock_guard<std::mutex> lk(x->mu);
    x->seq_n = 0;
    if (n == 0) { x->group_n = 0; x->n_groups = 0; x->h_goff.clear(); return 0; }
    VQ_CHECK(n == x->size, "vq_index_set_groups: %lld labels for an index of %lld rows", (long long)n, (long long)x->size);
    VQ_CHECK(n_groups >= 1 && n_groups <= n, "vq_index_set_groups: n_groups %d outside [1, %lld]", (int)n_groups, (long long)n);
    // dense labels, checked here: the kernels index per-group arrays with them.  By-group row list: a stable counting sort.
    std::vector<int32_t> off((size_t)n_groups + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int32_t g = group_of_row[r];
        VQ_CHECK(g >= 0 && g < n_groups, "vq_index_set_groups: row %lld has label %d outside [0, %d)", (long long)r, (int)g, (int)n_groups);
        ++off[(size_t)g + 1];
    }
    for (int32_t g = 0; g < n_groups; ++g)
        VQ_CHECK(off[(size_t)g + 1] > 0, "vq_index_set_groups: group %d has no rows (labels must be dense in [0, %d))", (int)g, (int)n_groups);
    for (int32_t g = 0; g < n_groups; ++g) off[(size_t)g + 1] += off[(size_t)g];
    const int64_t n_pad = round_up(n, SCAN_STREAM_ROWS), streams = n_pad / SCAN_STREAM_ROWS;
    // one host block mirrors the device layout: labels [n_pad] (-1 past n) | goff [n_groups + 1] | grows [n] | stream label [streams]
    const int64_t total = n_pad + n_groups + 1 + n + streams;
    std::vector<int32_t> h((size_t)total);
    int32_t* lab = h.data(); int32_t* goff = lab + n_pad; int32_t* grows = goff + n_groups + 1; int32_t* sg = grows + n;
    std::memcpy(lab, group_of_row, (size_t)n * 4);
    std::fill(lab + n, lab + n_pad, -1);
    std::memcpy(goff, off.data(), off.size() * 4);
    for (int64_t r = 0; r < n; ++r) grows[off[(size_t)lab[r]]++] = (int32_t)r;
    for (int64_t s = 0; s < streams; ++s) {
        const int32_t* l = lab + s * SCAN_STREAM_ROWS;
        bool same = l[0] >= 0;
        for (int i = 1; i < SCAN_STREAM_ROWS && same; ++i) same = l[i] == l[0];
        sg[s] = same ? l[0] : -1;
    }
    if (total > x->d_group.cap) {
        VQ_HIP(hipStreamSynchronize(x->stream));                   // a search in flight may still read the old arrays
        x->d_group.release(); x->group_n = 0; x->n_groups = 0;
        const int64_t cap = total + total / 4 + 1024;
        hipError_t e = hipMalloc((void**)&x->d_group.p, (size_t)cap * 4);
        if (e != hipSuccess) return fail(VQ_ERR_OOM, "vq_index_set_groups: hipMalloc failed: %s", hipGetErrorString(e));
        x->d_group.cap = cap;
    }
    VQ_HIP(hipMemcpyAsync(x->d_group, h.data(), (size_t)total * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));                       // `h` is this frame's
    x->d_goff = x->d_group + n_pad; x->d_grows = x->d_goff + n_groups + 1; x->d_sgroup = x->d_grows + n;
    x->h_goff.assign(goff, goff + n_groups + 1);
    x->group_n = n; x->n_groups = n_groups;
    return 0;
}

int vq_index_set_positions(vq_index* x, const int32_t* pos_of_row, int64_t n) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || pos_of_row), "vq_index_set_positions: bad argument");
    std::lock_guard<std::mutex> lk(x->mu);
    x->seq_n = 0;
    if (n == 0) { x->pos_n = 0; return 0; }
    VQ_CHECK(n == x->size, "vq_index_set_positions: %lld positions for an index of %lld rows", (long long)n, (long long)x->size);
    if (n > x->d_pos.cap) {
        VQ_HIP(hipStreamSynchronize(x->stream));                   // a search in flight may still read the old array
        x->pos_n = 0;
        VQ_TRY(x->d_pos.reserve(round_up(std::max<int64_t>(n, x->cap), 1024)));
    }
    VQ_HIP(hipMemcpyAsync(x->d_pos, pos_of_row, (size_t)n * 4, hipMemcpyHostToDevice, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));                       // `pos_of_row` is the caller's
    x->pos_n = n;
    return 0;
}

int vq_index_add(vq_index* x, const float* rows, int64_t n, int normalize) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || rows), "vq_index_add: bad argument");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    VQ_CHECK(x->size + n < ((int64_t)1 << 31), "vq_index_add: more than 2^31 rows");
    VQ_TRY(reserve_rows(x, x->size + n));
    VQ_HIP(hipMemcpyAsync(x->rows + x->size * x->dim, rows, (size_t)n * x->dim * 4, hipMemcpyHostToDevice, x->stream));
    VQ_TRY(finish_add(x, n, normalize));
    VQ_TRY(refresh_norm_range(x));                // this call blocks anyway: searches that follow need not
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

int vq_index_add_device(vq_index* x, const void* d_rows, int64_t n, int normalize) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || d_rows), "vq_index_add_device: bad argument");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    VQ_CHECK(x->size + n < ((int64_t)1 << 31), "vq_index_add_device: more than 2^31 rows");
    VQ_TRY(reserve_rows(x, x->size + n));
    VQ_HIP(hipMemcpyAsync(x->rows + x->size * x->dim, d_rows, (size_t)n * x->dim * 4, hipMemcpyDeviceToDevice, x->stream));
    return finish_add(x, n, normalize);
}

int vq_index_update_rows(vq_index* x, const float* rows, const int64_t* row_numbers, int64_t n, int normalize) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || (rows && row_numbers)), "vq_index_update_rows: bad argument");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    // the reference assigns in call order (hnsw.py:160), so the LAST update of a row is the one that stays: keep that one
    std::vector<int64_t> keep;            // indices into rows / row_numbers, in order
    {
        std::vector<std::pair<int64_t, int64_t>> last;          // (row number, index of its last update)
        last.reserve((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            VQ_CHECK(row_numbers[i] >= 0 && row_numbers[i] < x->size, "vq_index_update_rows: row %lld outside [0, %lld)",
                     (long long)row_numbers[i], (long long)x->size);
            last.emplace_back(row_numbers[i], i);
        }
        std::stable_sort(last.begin(), last.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t i = 0; i < last.size(); ++i)
            if (i + 1 == last.size() || last[i + 1].first != last[i].first) keep.push_back(last[i].second);
        std::sort(keep.begin(), keep.end());
    }
    const int64_t m = (int64_t)keep.size();
    const int64_t row_bytes = (int64_t)x->dim * 4;
    x->rows_changed();
    VQ_TRY(x->d_upd.reserve(m * x->dim + m * 2 + 4));
    int64_t* d_rn = (int64_t*)(x->d_upd + round_up(m * x->dim, 2));       // 8-byte aligned behind the rows
    std::vector<int64_t> rn((size_t)m);
    StreamDrain drain{x->stream};          // `rn` and the caller's `rows` feed asynchronous copies
    if (m == n) {
        VQ_HIP(hipMemcpyAsync(x->d_upd, rows, (size_t)(n * row_bytes), hipMemcpyHostToDevice, x->stream));
        for (int64_t i = 0; i < m; ++i) rn[(size_t)i] = row_numbers[i];
    } else {
        for (int64_t i = 0; i < m; ++i) {
            VQ_HIP(hipMemcpyAsync(x->d_upd + i * x->dim, rows + keep[(size_t)i] * x->dim, (size_t)row_bytes, hipMemcpyHostToDevice, x->stream));
            rn[(size_t)i] = row_numbers[keep[(size_t)i]];
        }
    }
    VQ_HIP(hipMemcpyAsync(d_rn, rn.data(), (size_t)m * 8, hipMemcpyHostToDevice, x->stream));
    {
        Prof p(x, I_NORMALIZE);
        // not normalised: measured, not trusted (finish_add); the range only widens, so a replaced row's old norm stays covered
        if (normalize) hipLaunchKernelGGL(normalize_rows_kernel, dim3(cdiv(m, NORM_ROWS)), dim3(NORM_ROWS), 0, x->stream, x->d_upd, m, x->dim);
        else VQ_TRY(measure_norm_range(x, x->d_upd, m));
    }
    {
        Prof p(x, I_TO_F16);
        const int64_t count4 = m * x->dim / 4;
        hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid_for(count4)), dim3(256), 0, x->stream, x->d_upd, d_rn, m, x->dim, x->rows, x->rows16);
    }
    VQ_HIP(hipGetLastError());
    VQ_TRY(refresh_norm_range(x));
    VQ_HIP(hipStreamSynchronize(x->stream));      // `rows`, `rn` are the caller's / this frame's
    return 0;
}

int vq_index_remove_rows(vq_index* x, const int64_t* row_numbers, int64_t n) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || row_numbers), "vq_index_remove_rows: bad argument");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t size = x->size;
    std::vector<int64_t> rm(row_numbers, row_numbers + n);
    for (int64_t i = 0; i < n; ++i)
        VQ_CHECK(rm[(size_t)i] >= 0 && rm[(size_t)i] < size, "vq_index_remove_rows: row %lld outside [0, %lld)",
                 (long long)rm[(size_t)i], (long long)size);
    std::sort(rm.begin(), rm.end());
    rm.erase(std::unique(rm.begin(), rm.end()), rm.end());      // a row named twice is removed once
    const int64_t m = (int64_t)rm.size(), n_new = size - m, r0 = rm[0], moved = n_new - r0;
    x->rows_changed();
    const bool ranks = x->rank_n == size, groups = x->group_n == size;      // labels / ranks that cover the index stay valid
    const int32_t G = groups ? x->n_groups : 0;
    const int64_t n_pad = round_up(size, SCAN_STREAM_ROWS), streams = n_pad / SCAN_STREAM_ROWS;
    // scratch words: removed rows (int64) | newrow [size] | src_of [moved] | prefix sums [size + 1] | tile sums | group keep/scan
    // [G + 1] | new rank_inv [n_new] | new label block (bounded by the old one's size)
    auto words = [](int64_t c) { return round_up(std::max<int64_t>(c, 1), 4); };
    const int64_t w_rm = words(2 * m), w_map = words(size), w_src = words(moved), w_S = words(size + 1),
                  w_tiles = words(cdiv(size, RM_SCAN_TILE) + 2), w_K = words((int64_t)G + 1), w_rinv = ranks ? words(n_new) : 0,
                  w_grp = groups ? words(n_pad + G + 1 + size + streams) : 0;
    VQ_TRY(x->d_rmw.reserve(w_rm + w_map + w_src + w_S + w_tiles + w_K + w_rinv + w_grp));
    int64_t* d_rm = (int64_t*)x->d_rmw.p;
    int32_t* newrow = x->d_rmw + w_rm;
    int32_t* src_of = newrow + w_map;
    int32_t* S = src_of + w_src;
    int32_t* tiles = S + w_S;
    int32_t* K = tiles + w_tiles;
    int32_t* rinv_new = K + w_K;
    int32_t* grp = rinv_new + w_rinv;
    StreamDrain drain{x->stream};          // `rm` feeds an asynchronous copy
    VQ_HIP(hipMemcpyAsync(d_rm, rm.data(), (size_t)m * 8, hipMemcpyHostToDevice, x->stream));
    hipLaunchKernelGGL(remove_row_map_kernel, dim3(grid_for(size)), dim3(256), 0, x->stream, d_rm, m, size, r0, newrow, src_of);
    VQ_HIP(hipGetLastError());
    // rows: only survivors at or after the first removed row move, all of them down.  Chunk by chunk in ascending order: gather
    // into scratch, then store back with the fp16 copy re-derived.  A chunk's sources lie at or above its destinations, and the
    // destinations lie below every later chunk's sources, so stream order alone makes this safe.
    if (moved > 0) {
        const int64_t chunk = std::min<int64_t>(moved, std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)x->dim * 4)));   // <= 256 MiB
        VQ_TRY(x->d_upd.reserve(chunk * x->dim));
        for (int64_t d0 = 0; d0 < moved; d0 += chunk) {
            const int64_t cnt = std::min<int64_t>(chunk, moved - d0);
            const int64_t count4 = cnt * x->dim / 4, dst = (r0 + d0) * x->dim;
            hipLaunchKernelGGL(remove_gather_rows_kernel, dim3(grid_for(count4)), dim3(256), 0, x->stream, x->rows, x->dim, src_of + d0,
                               cnt, x->d_upd);
            if (x->dim % 8 == 0) {
                hipLaunchKernelGGL(remove_store_rows_kernel, dim3(grid_for(count4 / 2)), dim3(256), 0, x->stream, x->d_upd, count4 / 2,
                                   x->rows + dst, x->rows16 + dst);
            } else {
                VQ_HIP(hipMemcpyAsync(x->rows + dst, x->d_upd, (size_t)count4 * 16, hipMemcpyDeviceToDevice, x->stream));
                hipLaunchKernelGGL(rows_to_f16_kernel, dim3(grid_for(count4)), dim3(256), 0, x->stream, x->rows + dst, x->rows16 + dst, count4);
            }
            VQ_HIP(hipGetLastError());
        }
    }
    // the scans read whole 1024 / 2048-row ranges: the fp16 rows past the new size go back to zeros, as in a fresh allocation
    VQ_HIP(hipMemsetAsync(x->rows16 + n_new * x->dim, 0, (size_t)m * x->dim * 2, x->stream));
    // id ranks: a stable compaction of the rank order
    if (ranks && n_new > 0) {
        hipLaunchKernelGGL(remove_survivor_flags_kernel, dim3(grid_for(size)), dim3(256), 0, x->stream, x->d_rank_inv, newrow, size, S);
        VQ_TRY(rm_exclusive_scan(x, S, size, tiles));
        hipLaunchKernelGGL(remove_renumber_ranks_kernel, dim3(grid_for(size)), dim3(256), 0, x->stream, x->d_rank_inv, newrow, S, size,
                           x->d_rank, rinv_new);
        VQ_HIP(hipMemcpyAsync(x->d_rank_inv, rinv_new, (size_t)n_new * 4, hipMemcpyDeviceToDevice, x->stream));
        VQ_HIP(hipGetLastError());
        x->rank_n = n_new;
    } else {
        x->rank_n = 0;
    }
    // group labels: drop emptied groups, renumber the rest in their old order, filter the by-group row list
    int32_t G_new = 0;
    if (groups && n_new > 0) {
        hipLaunchKernelGGL(remove_survivor_flags_kernel, dim3(grid_for(size)), dim3(256), 0, x->stream, x->d_grows, newrow, size, S);
        VQ_TRY(rm_exclusive_scan(x, S, size, tiles));
        hipLaunchKernelGGL(remove_group_keep_kernel, dim3(grid_for(G)), dim3(256), 0, x->stream, x->d_goff, S, G, K);
        VQ_TRY(rm_exclusive_scan(x, K, G, tiles));
        VQ_HIP(hipMemcpyAsync(&G_new, K + G, 4, hipMemcpyDeviceToHost, x->stream));
        VQ_HIP(hipStreamSynchronize(x->stream));                     // the new layout's offsets depend on the group count
        const int64_t n_pad_new = round_up(n_new, SCAN_STREAM_ROWS), streams_new = n_pad_new / SCAN_STREAM_ROWS;
        int32_t* lab_new = grp;
        int32_t* goff_new = lab_new + n_pad_new;
        int32_t* grows_new = goff_new + G_new + 1;
        int32_t* sg_new = grows_new + n_new;
        hipLaunchKernelGGL(remove_rebuild_groups_kernel, dim3(grid_for(std::max<int64_t>(size, G))), dim3(256), 0, x->stream, x->d_group,
                           x->d_goff, x->d_grows, newrow, S, K, size, G, n_new, n_pad_new, lab_new, goff_new, grows_new);
        hipLaunchKernelGGL(remove_stream_labels_kernel, dim3(grid_for(streams_new)), dim3(256), 0, x->stream, lab_new, streams_new, sg_new);
        const int64_t total_new = n_pad_new + G_new + 1 + n_new + streams_new;
        VQ_HIP(hipMemcpyAsync(x->d_group, grp, (size_t)total_new * 4, hipMemcpyDeviceToDevice, x->stream));
        VQ_HIP(hipGetLastError());
        x->d_goff = x->d_group + n_pad_new; x->d_grows = x->d_goff + G_new + 1; x->d_sgroup = x->d_grows + n_new;
        x->h_goff.resize((size_t)G_new + 1);                         // the host mirror of goff: read back, waited for below
        VQ_HIP(hipMemcpyAsync(x->h_goff.data(), goff_new, ((size_t)G_new + 1) * 4, hipMemcpyDeviceToHost, x->stream));
        x->group_n = n_new; x->n_groups = G_new;
    } else {
        x->group_n = 0; x->n_groups = 0; x->h_goff.clear();
    }
    // the |row|^2 range stays as it is: it still covers every survivor (conservative, as in vq_index_update_rows)
    x->size = n_new;
    x->pos_n = 0; x->seq_n = 0;                    // positions are not compacted: set them again
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

int vq_index_search_device(vq_index* x, const void* d_queries, int nq, int k, int mode, void* d_ids, void* d_dist) {
    return search_call(x, "vq_index_search_device", ON_DEVICE, d_queries, nq, k, mode, d_ids, d_dist);
}

int vq_index_search(vq_index* x, const float* queries, int nq, int k, int mode, int32_t* ids, float* dist) {
    return search_call(x, "vq_index_search", HOST_PAGEABLE, queries, nq, k, mode, ids, dist);
}

int vq_index_search_grouped_device(vq_index* x, const void* d_queries, int nq, int k, int mode, void* d_groups, void* d_rows, void* d_dist) {
    return grouped_call(x, "vq_index_search_grouped_device", ON_DEVICE, d_queries, nq, k, mode, d_groups, d_rows, d_dist);
}

int vq_index_search_grouped(vq_index* x, const float* queries, int nq, int k, int mode, int32_t* groups, int32_t* rows, float* dist) {
    return grouped_call(x, "vq_index_search_grouped", HOST_PAGEABLE, queries, nq, k, mode, groups, rows, dist);
}

int vq_index_search_distinct_device(vq_index* x, const void* d_queries, int nq, int k, int mode, int64_t min_gap, void* d_ids, void* d_dist) {
    return distinct_call(x, "vq_index_search_distinct_device", ON_DEVICE, d_queries, nq, k, mode, min_gap, d_ids, d_dist);
}

int vq_index_search_distinct(vq_index* x, const float* queries, int nq, int k, int mode, int64_t min_gap, int32_t* ids, float* dist) {
    return distinct_call(x, "vq_index_search_distinct", HOST_PAGEABLE, queries, nq, k, mode, min_gap, ids, dist);
}

// plan_distinct's answer for this process's environment; needs no device
int vq_debug_distinct_plan(int64_t n, int nq, int k, int64_t min_gap, int mode, int64_t* depth, int* producer, int* redo_slices) {
    VQ_CHECK(depth && producer && redo_slices && n >= 1 && n < ((int64_t)1 << 31) && nq >= 1 && k >= 1 && k <= 1024 && min_gap >= 0 &&
             mode >= 0 && mode <= 2, "vq_debug_distinct_plan: takes 1 <= n < 2^31, nq >= 1, 1 <= k <= 1024, min_gap >= 0, mode 0..2");
    const DistinctPlan p = plan_distinct(n, nq, k, min_gap, mode, distinct_depth_override());
    *depth = p.depth; *producer = p.producer; *redo_slices = p.slices;
    return 0;
}

int vq_index_search_diverse_device(vq_index* x, const void* d_queries, int nq, int k, int mode, float min_dist, void* d_ids, void* d_dist) {
    return diverse_call(x, "vq_index_search_diverse_device", ON_DEVICE, d_queries, nq, k, mode, min_dist, d_ids, d_dist);
}

int vq_index_search_diverse(vq_index* x, const float* queries, int nq, int k, int mode, float min_dist, int32_t* ids, float* dist) {
    return diverse_call(x, "vq_index_search_diverse", HOST_PAGEABLE, queries, nq, k, mode, min_dist, ids, dist);
}

// plan_diverse's answer for this process's environment; needs no device
int vq_debug_diverse_plan(int64_t n, int nq, int k, float min_dist, int mode, int64_t* depth, int* producer, int64_t* pair_bytes,
                          int* redo_slices, int* launches) {
    VQ_CHECK(depth && producer && pair_bytes && redo_slices && launches && n >= 1 && n < ((int64_t)1 << 31) && nq >= 1 && k >= 1 &&
             k <= DIV_MAX_K && min_dist >= 0.0f && mode >= 0 && mode <= 2,
             "vq_debug_diverse_plan: takes 1 <= n < 2^31, nq >= 1, 1 <= k <= %d, min_dist >= 0 (not NaN), mode 0..2", DIV_MAX_K);
    const DiversePlan p = plan_diverse(n, nq, k, min_dist, mode, diverse_depth_override());
    *depth = p.depth; *producer = p.producer; *pair_bytes = p.pair_bytes; *redo_slices = p.slices; *launches = p.launches;
    return 0;
}

int vq_index_search_filtered_device(vq_index* x, const void* d_queries, int nq, int k, int mode, const int32_t* groups, int32_t n_sel,
                                    int exclude, void* d_ids, void* d_dist) {
    return filtered_call(x, "vq_index_search_filtered_device", ON_DEVICE, d_queries, nq, k, mode, groups, n_sel, exclude, d_ids, d_dist);
}

int vq_index_search_filtered(vq_index* x, const float* queries, int nq, int k, int mode, const int32_t* groups, int32_t n_sel, int exclude,
                             int32_t* ids, float* dist) {
    return filtered_call(x, "vq_index_search_filtered", HOST_PINNED, queries, nq, k, mode, groups, n_sel, exclude, ids, dist);
}

int vq_index_search_grouped_filtered_device(vq_index* x, const void* d_queries, int nq, int k, int mode, const int32_t* groups,
                                            int32_t n_sel, int exclude, void* d_groups, void* d_rows, void* d_dist) {
    return grouped_filtered_call(x, "vq_index_search_grouped_filtered_device", ON_DEVICE, d_queries, nq, k, mode, groups, n_sel, exclude, d_groups,
                                 d_rows, d_dist);
}

int vq_index_search_grouped_filtered(vq_index* x, const float* queries, int nq, int k, int mode, const int32_t* groups, int32_t n_sel,
                                     int exclude, int32_t* groups_out, int32_t* rows, float* dist) {
    return grouped_filtered_call(x, "vq_index_search_grouped_filtered", HOST_PINNED, queries, nq, k, mode, groups, n_sel, exclude, groups_out, rows,
                                 dist);
}

int vq_index_search_set_device(vq_index* x, const void* d_queries, int m, int k, int mode, const int32_t* groups, int32_t n_sel,
                               int exclude, void* d_groups_out, void* d_dist_out, void* d_match_rows) {
    return set_call(x, "vq_index_search_set_device", ON_DEVICE, d_queries, m, k, mode, groups, n_sel, exclude, d_groups_out, d_dist_out, d_match_rows);
}

int vq_index_search_set(vq_index* x, const float* queries, int m, int k, int mode, const int32_t* groups, int32_t n_sel, int exclude,
                        int32_t* groups_out, float* dist_out, int32_t* match_rows) {
    return set_call(x, "vq_index_search_set", HOST_PINNED, queries, m, k, mode, groups, n_sel, exclude, groups_out, dist_out, match_rows);
}

int vq_index_search_sequence_device(vq_index* x, const void* d_steps, int m, int k, int64_t min_gap, int64_t max_gap, const int32_t* groups,
                                    int32_t n_sel, int exclude, void* d_groups_out, void* d_dist_out, void* d_chain_rows) {
    return sequence_call(x, "vq_index_search_sequence_device", ON_DEVICE, d_steps, m, k, min_gap, max_gap, groups, n_sel, exclude, d_groups_out,
                         d_dist_out, d_chain_rows);
}

int vq_index_search_sequence(vq_index* x, const float* steps, int m, int k, int64_t min_gap, int64_t max_gap, const int32_t* groups,
                             int32_t n_sel, int exclude, int32_t* groups_out, float* dist_out, int32_t* chain_rows) {
    return sequence_call(x, "vq_index_search_sequence", HOST_PINNED, steps, m, k, min_gap, max_gap, groups, n_sel, exclude, groups_out, dist_out,
                         chain_rows);
}

int vq_index_search_spans_device(vq_index* x, const void* d_queries, int nq, int k, float max_dist, int64_t max_gap, int64_t max_span,
                                 const int32_t* groups, int32_t n_sel, int exclude, void* d_groups_out, void* d_dist_out, void* d_mass_out,
                                 void* d_len_out, void* d_rows_out) {
    return spans_call(x, "vq_index_search_spans_device", ON_DEVICE, d_queries, nq, k, max_dist, max_gap, max_span, groups, n_sel, exclude,
                      d_groups_out, d_dist_out, d_mass_out, d_len_out, d_rows_out);
}

int vq_index_search_spans(vq_index* x, const float* queries, int nq, int k, float max_dist, int64_t max_gap, int64_t max_span,
                          const int32_t* groups, int32_t n_sel, int exclude, int32_t* groups_out, float* dist_out, int64_t* mass_out,
                          int32_t* len_out, int32_t* rows_out) {
    return spans_call(x, "vq_index_search_spans", HOST_PINNED, queries, nq, k, max_dist, max_gap, max_span, groups, n_sel, exclude, groups_out,
                      dist_out, mass_out, len_out, rows_out);
}

// plan_spans' answer for this process's environment; needs no device
int vq_debug_span_plan(int64_t n, int64_t n_groups, int64_t largest_group, int nq, int* query_chunks, int* lds_rows, int64_t* lds_bytes,
                       int* groups_global_form, int64_t* scratch_bytes) {
    VQ_CHECK(query_chunks && lds_rows && lds_bytes && groups_global_form && scratch_bytes && n >= 1 && n < ((int64_t)1 << 31) &&
             n_groups >= 1 && n_groups <= n && largest_group >= 1 && largest_group <= n && nq >= 1 && nq <= SPAN_MAX_Q,
             "vq_debug_span_plan: takes 1 <= largest_group <= n < 2^31, 1 <= n_groups <= n, 1 <= nq <= %d", SPAN_MAX_Q);
    const SpanPlan p = span_plan_env(n, n_groups, largest_group, nq);
    *query_chunks = p.query_chunks; *lds_rows = p.lds_rows; *lds_bytes = p.lds_bytes; *groups_global_form = p.global_form;
    *scratch_bytes = p.scratch_bytes;
    return 0;
}

int vq_index_align_clip_device(vq_index* x, const void* d_clip, int m, int k, float max_dist, const int32_t* groups, int32_t n_sel, int exclude,
                               void* d_groups_out, void* d_dist_out, void* d_cost_out, void* d_rows_out, void* d_align_out) {
    return align_call(x, "vq_index_align_clip_device", ON_DEVICE, d_clip, m, k, max_dist, groups, n_sel, exclude, d_groups_out, d_dist_out,
                      d_cost_out, d_rows_out, d_align_out);
}

int vq_index_align_clip(vq_index* x, const float* clip, int m, int k, float max_dist, const int32_t* groups, int32_t n_sel, int exclude,
                        int32_t* groups_out, float* dist_out, int64_t* cost_out, int32_t* rows_out, int32_t* align_out) {
    return align_call(x, "vq_index_align_clip", HOST_PINNED, clip, m, k, max_dist, groups, n_sel, exclude, groups_out, dist_out, cost_out,
                      rows_out, align_out);
}

// plan_align's answer for this process's environment; needs no device.  largest_group: the largest allowed group; the winners
// are min(k, n_groups).
int vq_debug_align_plan(int64_t n, int64_t n_groups, int64_t largest_group, int m, int k, int with_align, int* clip_chunks, int* lds_rows,
                        int64_t* lds_bytes, int* groups_global_form, int64_t* scratch_bytes, int* winner_batches) {
    VQ_CHECK(clip_chunks && lds_rows && lds_bytes && groups_global_form && scratch_bytes && winner_batches && n >= 1 &&
             n < ((int64_t)1 << 31) && n_groups >= 1 && n_groups <= n && largest_group >= 1 && largest_group <= n && m >= 1 &&
             m <= ALIGN_MAX_M && k >= 1 && k <= 1024,
             "vq_debug_align_plan: takes 1 <= largest_group <= n < 2^31, 1 <= n_groups <= n, 1 <= m <= %d, 1 <= k <= 1024", ALIGN_MAX_M);
    VQ_CHECK(!with_align || (int64_t)m * largest_group * 4 <= ALIGN_TABLE_MAX_BYTES, "vq_debug_align_plan: align_out needs m x "
             "largest_group x 4 B <= 1 GiB (m %d, %lld rows)", m, (long long)largest_group);
    const AlignPlan p = align_plan_env(n, largest_group, m, (int)std::min<int64_t>(k, n_groups), with_align != 0);
    *clip_chunks = p.frame_chunks; *lds_rows = p.lds_rows; *lds_bytes = p.lds_bytes; *groups_global_form = p.global_form;
    *scratch_bytes = p.state_bytes; *winner_batches = p.winner_batches;
    return 0;
}

// plan_sequence's answer for this process's environment; needs no device
int vq_debug_sequence_plan(int64_t n, int64_t largest_group, int m, int k, int* step_chunks, int* lds_rows, int* groups_global_form,
                           int64_t* lds_bytes, int* chain_table, int* chain_slices) {
    VQ_CHECK(step_chunks && lds_rows && groups_global_form && lds_bytes && chain_table && chain_slices && n >= 1 && n < ((int64_t)1 << 31) &&
             largest_group >= 1 && largest_group <= n && m >= 1 && m <= SEQ_MAX_M && k >= 1 && k <= 1024,
             "vq_debug_sequence_plan: takes 1 <= largest_group <= n < 2^31, 1 <= m <= %d, 1 <= k <= 1024", SEQ_MAX_M);
    const SequencePlan p = seq_plan_env(n, largest_group, m);
    *step_chunks = p.step_chunks; *lds_rows = p.lds_rows; *groups_global_form = p.global_form; *lds_bytes = p.lds_bytes;
    *chain_table = p.bp_table; *chain_slices = p.bp_slices;
    return 0;
}

int vq_index_summarize_groups_device(vq_index* x, const int32_t* groups, int32_t n_sel, int k, float max_radius, void* d_rows_out,
                                     void* d_radius_out, void* d_members_out) {
    return summarize_call(x, "vq_index_summarize_groups_device", ON_DEVICE, groups, n_sel, k, max_radius, d_rows_out, d_radius_out, d_members_out);
}

int vq_index_summarize_groups(vq_index* x, const int32_t* groups, int32_t n_sel, int k, float max_radius, int32_t* rows_out,
                              float* radius_out, int32_t* members_out) {
    return summarize_call(x, "vq_index_summarize_groups", HOST_PINNED, groups, n_sel, k, max_radius, rows_out, radius_out, members_out);
}

// plan_summary's answer for this process's environment; needs no device
int vq_debug_summary_plan(int64_t n, int64_t largest_group, int dim, int k, int* lds_rows, int64_t* lds_bytes, int* groups_wide_form,
                          int* launches) {
    VQ_CHECK(lds_rows && lds_bytes && groups_wide_form && launches && n >= 1 && n < ((int64_t)1 << 31) && largest_group >= 1 &&
             largest_group <= n && dim > 0 && dim % 4 == 0 && dim <= 4096 && k >= 1 && k <= SUM_MAX_K,
             "vq_debug_summary_plan: takes 1 <= largest_group <= n < 2^31, a dim vq_index_create takes, 1 <= k <= %d", SUM_MAX_K);
    const SummaryPlan p = sum_plan_env(largest_group, dim, k);
    *lds_rows = p.lds_rows; *lds_bytes = p.lds_bytes; *groups_wide_form = p.wide_form; *launches = p.launches;
    return 0;
}

int vq_index_label_rows_device(vq_index* x, const void* d_prompts, int P, int mode, float max_dist, void* d_row_label, void* d_row_dist,
                               int m, void* d_group_tags, void* d_group_votes, void* d_group_show_rows, void* d_group_unlabelled) {
    return label_call(x, "vq_index_label_rows_device", ON_DEVICE, d_prompts, P, mode, max_dist, d_row_label, d_row_dist, m, d_group_tags,
                      d_group_votes, d_group_show_rows, d_group_unlabelled);
}

int vq_index_label_rows(vq_index* x, const float* prompts, int P, int mode, float max_dist, int32_t* row_label, float* row_dist, int m,
                        int32_t* group_tags, int32_t* group_votes, int32_t* group_show_rows, int32_t* group_unlabelled) {
    return label_call(x, "vq_index_label_rows", HOST_PINNED, prompts, P, mode, max_dist, row_label, row_dist, m, group_tags, group_votes,
                      group_show_rows, group_unlabelled);
}

// plan_label's answer for near-unit rows; needs no device
int vq_debug_label_plan(int64_t n, int dim, int P, int mode, int64_t largest_group, int* fp16_path, int* exact_chunk, int* exact_chunks,
                        int64_t* exact_bytes, int* prompt_tiles, int* prompt_ranges, int64_t* row_tiles, int64_t* part_bytes, float* eps,
                        int* group_split_rows, int* group_piece_rows, int64_t* largest_group_pieces) {
    VQ_CHECK(fp16_path && exact_chunk && exact_chunks && exact_bytes && prompt_tiles && prompt_ranges && row_tiles && part_bytes && eps &&
             group_split_rows && group_piece_rows && largest_group_pieces && largest_group >= 0 && largest_group <= n && n >= 1 && n < ((int64_t)1 << 31) && dim > 0 && dim % 4 == 0 && dim <= 4096 && P >= 1 && P <= LABEL_MAX_P && mode >= 0 && mode <= 2,
             "vq_debug_label_plan: takes 0 <= largest_group <= n, 1 <= n < 2^31, a dim vq_index_create takes, 1 <= P <= %d, mode 0, 1 or 2", LABEL_MAX_P);
    VQ_CHECK(mode != 2 || scan_fp16_dim(dim), "vq_debug_label_plan: the fp16 path needs dim 256, 512 or 768");
    const LabelPlan p = plan_label(n, dim, P, mode, true, largest_group);
    *fp16_path = p.fp16; *exact_chunk = p.exact_chunk; *exact_chunks = p.exact_chunks; *exact_bytes = p.exact_bytes;
    *prompt_tiles = p.prompt_tiles; *prompt_ranges = p.prompt_ranges; *row_tiles = p.row_tiles; *part_bytes = p.part_bytes; *eps = p.eps;
    *group_split_rows = p.group_split_rows; *group_piece_rows = p.group_piece_rows; *largest_group_pieces = p.largest_group_pieces;
    return 0;
}

int vq_index_cluster_device(vq_index* x, const void* d_init, const void* d_init_rows, int P, int iters, int mode, void* d_centroids,
                            void* d_row_label, void* d_row_dist, void* d_counts, void* d_show_rows) {
    return cluster_call(x, "vq_index_cluster_device", ON_DEVICE, d_init, (const int32_t*)d_init_rows, P, iters, mode, d_centroids, d_row_label,
                        d_row_dist, d_counts, d_show_rows, nullptr, nullptr);
}

int vq_index_cluster(vq_index* x, const float* init, const int32_t* init_rows, int P, int max_iter, int mode, float* centroids,
                     int32_t* row_label, float* row_dist, int32_t* counts, int32_t* show_rows, int* iterations, int32_t* changed) {
    return cluster_call(x, "vq_index_cluster", HOST_PINNED, init, init_rows, P, max_iter, mode, centroids, row_label, row_dist, counts, show_rows,
                        iterations, changed);
}

// The update alone, on labels the caller writes (tests/test_cluster.py): centroids_out = the update of centroids_in under
// labels [n] (each in [0, P)), counts [P] the clusters' rows.
int vq_index_debug_cluster_update(vq_index* x, const int32_t* labels, int P, const float* centroids_in, float* centroids_out, int32_t* counts) {
    static const char* fn = "vq_index_debug_cluster_update";
    VQ_CHECK(P >= 1 && P <= CL_MAX_P, "%s: P %d outside [1, %d]", fn, P, CL_MAX_P);
    VQ_TRY(require_init());
    VQ_CHECK(x && labels && centroids_in && centroids_out && counts, "%s: bad argument", fn);
    std::lock_guard<std::mutex> lk(x->mu);
    const int64_t n = x->size;
    VQ_CHECK(n >= 1, "%s: the index is empty", fn);
    for (int64_t r = 0; r < n; ++r) VQ_CHECK(labels[r] >= 0 && labels[r] < P, "%s: labels[%lld] = %d outside [0, %d)", fn, (long long)r, (int)labels[r], P);
    ClusterBufs b;
    VQ_TRY(cluster_reserve(x, P, &b));
    VQ_TRY(stage_queries(x, centroids_in, P));
    StreamDrain drain{x->stream};                           // `labels` is the caller's pageable memory
    VQ_HIP(hipMemcpyAsync(b.lab, labels, (size_t)n * 4, hipMemcpyHostToDevice, x->stream));
    cluster_list(x, b, b.lab, P, true, b.counts, nullptr);
    cluster_update(x, b, P, x->d_q);
    VQ_HIP(hipGetLastError());
    VQ_HIP(hipMemcpyAsync(centroids_out, x->d_q, (size_t)P * x->dim * 4, hipMemcpyDeviceToHost, x->stream));
    VQ_HIP(hipMemcpyAsync(counts, b.counts, (size_t)P * 4, hipMemcpyDeviceToHost, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

// plan_cluster's answer; needs no device
int vq_debug_cluster_plan(int64_t n, int dim, int P, int* piece_rows, int64_t* max_pieces, int64_t* list_blocks, int64_t* table_bytes,
                          int64_t* sum_bytes, int64_t* scratch_bytes, int* piece_threads, int* launches) {
    VQ_CHECK(piece_rows && max_pieces && list_blocks && table_bytes && sum_bytes && scratch_bytes && piece_threads && launches && n >= 1 &&
             n < ((int64_t)1 << 31) && dim > 0 && dim % 4 == 0 && dim <= 4096 && P >= 1 && P <= CL_MAX_P && P <= n,
             "vq_debug_cluster_plan: takes 1 <= n < 2^31, a dim vq_index_create takes, 1 <= P <= min(%d, n)", CL_MAX_P);
    const ClusterPlan p = plan_cluster(n, dim, P);
    *piece_rows = p.piece_rows; *max_pieces = p.max_pieces; *list_blocks = p.blocks; *table_bytes = p.table_bytes; *sum_bytes = p.sum_bytes;
    *scratch_bytes = p.scratch_bytes; *piece_threads = p.piece_threads; *launches = p.launches;
    return 0;
}

int vq_index_search_compound_device(vq_index* x, const void* d_terms, int m, const int32_t* clause_of, float margin, int k, int mode,
                                    void* d_ids, void* d_dist, void* d_term_dist) {
    return compound_call(x, "vq_index_search_compound_device", ON_DEVICE, d_terms, m, clause_of, margin, k, mode, d_ids, d_dist, d_term_dist);
}

int vq_index_search_compound(vq_index* x, const float* terms, int m, const int32_t* clause_of, float margin, int k, int mode, int32_t* ids,
                             float* dist, float* term_dist) {
    return compound_call(x, "vq_index_search_compound", HOST_PINNED, terms, m, clause_of, margin, k, mode, ids, dist, term_dist);
}

// plan_compound's answer for near-unit rows; needs no device
int vq_debug_compound_plan(int64_t n, int dim, int m, int k, int mode, int* fp16_path, int64_t* streams, int* rescore_pool,
                           int64_t* exact_bytes, float* eps) {
    VQ_CHECK(fp16_path && streams && rescore_pool && exact_bytes && eps && n >= 1 && n < ((int64_t)1 << 31) && dim > 0 && dim % 4 == 0 &&
             dim <= 4096 && m >= 1 && m <= CP_MAX_M && k >= 1 && k <= 1024 && mode >= 0 && mode <= 2,
             "vq_debug_compound_plan: takes 1 <= n < 2^31, a dim vq_index_create takes, 1 <= m <= %d, 1 <= k <= 1024, mode 0, 1 or 2", CP_MAX_M);
    VQ_CHECK(mode != 2 || (scan_fp16_dim(dim) && k <= CP_K_MAX), "vq_debug_compound_plan: the fp16 path needs dim 256, 512 or 768 and k <= %d",
             CP_K_MAX);
    const CompoundPlan p = plan_compound(n, dim, m, nullptr, k, mode, true);
    *fp16_path = p.fp16; *streams = p.streams; *rescore_pool = p.pool; *exact_bytes = p.exact_bytes; *eps = p.eps;
    return 0;
}

int vq_index_segment_groups_device(vq_index* x, const int32_t* groups, int32_t n_sel, int k, float penalty, int64_t max_len, void* d_count_out,
                                   void* d_first_out, void* d_last_out, void* d_len_out, void* d_spread_out, void* d_show_out,
                                   void* d_mean_spread_out) {
    return segment_call(x, "vq_index_segment_groups_device", ON_DEVICE, groups, n_sel, k, penalty, max_len, d_count_out, d_first_out, d_last_out,
                        d_len_out, d_spread_out, d_show_out, d_mean_spread_out);
}

int vq_index_segment_groups(vq_index* x, const int32_t* groups, int32_t n_sel, int k, float penalty, int64_t max_len, int32_t* count_out,
                            int32_t* first_out, int32_t* last_out, int32_t* len_out, float* spread_out, int32_t* show_out, float* mean_spread_out) {
    return segment_call(x, "vq_index_segment_groups", HOST_PINNED, groups, n_sel, k, penalty, max_len, count_out, first_out, last_out, len_out,
                        spread_out, show_out, mean_spread_out);
}

// plan_segment's answer for this process's environment; needs no device
int vq_debug_segment_plan(const int64_t* lengths, int32_t n_sel, int dim, int k, int64_t max_len, int* batches, int64_t* table_bytes, int* lds_rows,
                          int64_t* lds_bytes, int* global_form, int* launches, int64_t* pairs) {
    static const char* fn = "vq_debug_segment_plan";
    VQ_CHECK(lengths && batches && table_bytes && lds_rows && lds_bytes && global_form && launches && pairs && n_sel >= 1 && dim > 0 &&
             dim % 4 == 0 && dim <= 4096 && k >= 1 && k <= SEG_MAX_K && max_len >= 0,
             "%s: takes n_sel >= 1 group lengths, a dim vq_index_create takes, 1 <= k <= %d, max_len >= 0", fn, SEG_MAX_K);
    for (int32_t i = 0; i < n_sel; ++i) {
        VQ_CHECK(lengths[i] >= 0 && lengths[i] < ((int64_t)1 << 31), "%s: lengths[%d] = %lld outside [0, 2^31)", fn, (int)i, (long long)lengths[i]);
        VQ_TRY(seg_check_pairs(fn, i, lengths[i], max_len));
    }
    const SegmentPlan p = seg_plan_env(lengths, n_sel, dim, k, max_len, true);
    *batches = p.batches; *table_bytes = p.table_bytes; *lds_rows = p.lds_rows; *lds_bytes = p.lds_bytes; *global_form = p.global_form;
    *launches = p.launches; *pairs = p.pairs;
    return 0;
}

int vq_index_match_runs_device(vq_index* x, const void* d_queries, int m, int k, float max_dist, int min_len, int max_miss, int mode,
                               const int32_t* groups, int32_t n_sel, int exclude, void* d_groups_out, void* d_hits_out, void* d_span_out,
                               void* d_q_first_out, void* d_row_first_out, void* d_row_last_out, void* d_mean_dist_out) {
    return match_call(x, "vq_index_match_runs_device", ON_DEVICE, d_queries, m, k, max_dist, min_len, max_miss, mode, groups, n_sel, exclude,
                      d_groups_out, d_hits_out, d_span_out, d_q_first_out, d_row_first_out, d_row_last_out, d_mean_dist_out);
}

int vq_index_match_runs(vq_index* x, const float* queries, int m, int k, float max_dist, int min_len, int max_miss, int mode,
                        const int32_t* groups, int32_t n_sel, int exclude, int32_t* groups_out, int32_t* hits_out, int32_t* span_out,
                        int32_t* q_first_out, int32_t* row_first_out, int32_t* row_last_out, float* mean_dist_out) {
    return match_call(x, "vq_index_match_runs", HOST_PINNED, queries, m, k, max_dist, min_len, max_miss, mode, groups, n_sel, exclude, groups_out,
                      hits_out, span_out, q_first_out, row_first_out, row_last_out, mean_dist_out);
}

// plan_match's answer for near-unit rows and this process's environment; needs no device
int vq_debug_match_plan(int64_t n, int64_t n_groups, int dim, int m, int mode, int* fp16_path, int64_t* bits_bytes, int* exact_chunk,
                        int* exact_chunks, int* q_tiles, int* ranges, int64_t* tile_grid, int64_t* filed_cap, int* key_bits,
                        int64_t* run_blocks, int* launches) {
    static const char* fn = "vq_debug_match_plan";
    VQ_CHECK(fp16_path && bits_bytes && exact_chunk && exact_chunks && q_tiles && ranges && tile_grid && filed_cap && key_bits && run_blocks &&
             launches && n >= 1 && n < ((int64_t)1 << 31) && n_groups >= 1 && n_groups <= n && dim > 0 && dim % 4 == 0 && dim <= 4096 &&
             m >= 1 && m <= MATCH_MAX_M && mode >= 0 && mode <= 2,
             "%s: takes 1 <= n_groups <= n < 2^31, a dim vq_index_create takes, 1 <= m <= %d, mode 0, 1 or 2", fn, MATCH_MAX_M);
    VQ_CHECK(mode != 2 || scan_fp16_dim(dim), "%s: the tile path needs dim 256, 512 or 768", fn);
    VQ_TRY(match_check_bits(fn, m, n));
    const MatchPlan p = match_plan_env(n, n_groups, dim, m, mode, true);
    *fp16_path = p.fp16; *bits_bytes = p.bits_bytes; *exact_chunk = p.exact_chunk; *exact_chunks = p.exact_chunks; *q_tiles = p.q_tiles;
    *ranges = p.ranges; *tile_grid = p.tile_grid; *filed_cap = p.filed_cap; *key_bits = 3 * p.key_m_bits + p.key_d_bits;
    *run_blocks = p.run_blocks; *launches = p.launches;
    return 0;
}

int vq_index_neighbors_device(vq_index* x, const int64_t* rows, int64_t m, int k, int exclude, int mode, void* d_ids, void* d_dist) {
    return neighbors_call(x, "vq_index_neighbors_device", ON_DEVICE, rows, m, k, exclude, mode, d_ids, d_dist);
}

int vq_index_neighbors(vq_index* x, const int64_t* rows, int64_t m, int k, int exclude, int mode, int32_t* ids, float* dist) {
    return neighbors_call(x, "vq_index_neighbors", HOST_PINNED, rows, m, k, exclude, mode, ids, dist);
}

// plan_neighbors' answer for near-unit rows; needs no device
int vq_debug_neighbors_plan(int64_t n, int dim, int64_t m, int k, int exclude, int mode, int* fp16_path, int64_t* chunk_rows, int64_t* chunks,
                            int64_t* key_bytes, int* rescore_kind, float* eps) {
    static const char* fn = "vq_debug_neighbors_plan";
    VQ_CHECK(fp16_path && chunk_rows && chunks && key_bytes && rescore_kind && eps && n >= 1 && n < ((int64_t)1 << 31) && dim > 0 && dim % 4 == 0 &&
             dim <= 4096 && m >= 1 && m < ((int64_t)1 << 31) && (exclude == 0 || exclude == 1) && mode >= 0 && mode <= 2,
             "%s: takes 1 <= n < 2^31, a dim vq_index_create takes, 1 <= m < 2^31, exclude 0 or 1, mode 0, 1 or 2", fn);
    VQ_CHECK(k >= 1 && k <= (mode == 2 ? RV_K_MAX : NB_K_EXACT_MAX), "%s: k = %d, takes 1 <= k <= %d (mode 2: %d)", fn, k, NB_K_EXACT_MAX, RV_K_MAX);
    VQ_CHECK(mode != 2 || scan_fp16_dim(dim), "%s: the fp16 path needs dim 256, 512 or 768", fn);
    const NeighborsPlan p = plan_neighbors(n, dim, m, k, mode, true, neighbors_chunk_override());
    *fp16_path = p.fp16; *chunk_rows = p.chunk_rows; *chunks = p.chunks; *key_bytes = p.key_bytes; *rescore_kind = p.rescore; *eps = p.eps;
    return 0;
}

int vq_index_synchronize(vq_index* x) {
    VQ_CHECK(x, "vq_index_synchronize: null handle");
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

int vq_index_set_stream(vq_index* x, void* hip_stream) {
    VQ_CHECK(x, "vq_index_set_stream: null handle");
    std::lock_guard<std::mutex> lk(x->mu);
    VQ_HIP(hipStreamSynchronize(x->stream));
    x->stream = hip_stream ? (hipStream_t)hip_stream : x->own_stream;
    return 0;
}

int vq_index_export(vq_index* x, float* rows) {
    VQ_TRY(require_init());
    VQ_CHECK(x && (x->size == 0 || rows), "vq_index_export: null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    if (x->size == 0) return 0;
    VQ_HIP(hipMemcpyAsync(rows, x->rows, (size_t)x->size * x->dim * 4, hipMemcpyDeviceToHost, x->stream));
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

int vq_index_read_rows(vq_index* x, const int64_t* row_numbers, int64_t n, float* out) {
    VQ_TRY(require_init());
    VQ_CHECK(x && n >= 0 && (n == 0 || (row_numbers && out)), "vq_index_read_rows: bad argument");
    std::lock_guard<std::mutex> lk(x->mu);
    for (int64_t i = 0; i < n; ++i) {
        VQ_CHECK(row_numbers[i] >= 0 && row_numbers[i] < x->size, "vq_index_read_rows: row %lld outside [0, %lld)",
                 (long long)row_numbers[i], (long long)x->size);
        VQ_HIP(hipMemcpyAsync(out + i * x->dim, x->rows + row_numbers[i] * x->dim, (size_t)x->dim * 4, hipMemcpyDeviceToHost, x->stream));
    }
    VQ_HIP(hipStreamSynchronize(x->stream));
    return 0;
}

int vq_index_profile_begin(vq_index* x) {
    VQ_CHECK(x, "vq_index_profile_begin: null handle");
    std::lock_guard<std::mutex> lk(x->mu);
    VQ_HIP(hipStreamSynchronize(x->stream));
    for (auto& ev : x->events) { x->pool.push_back(ev.a); x->pool.push_back(ev.b); }
    x->events.clear();
    x->profiling = true;
    return 0;
}

int vq_index_profile_end(vq_index* x, float* ms, int* launches) {
    VQ_CHECK(x && ms && launches, "vq_index_profile_end: null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    x->profiling = false;
    VQ_HIP(hipStreamSynchronize(x->stream));
    for (int i = 0; i < VQ_IDX_NCLASS; ++i) { ms[i] = 0.f; launches[i] = 0; }
    for (auto& ev : x->events) {
        float t = 0.f;
        VQ_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
        ms[ev.cls] += t; launches[ev.cls] += 1;
        x->pool.push_back(ev.a); x->pool.push_back(ev.b);
    }
    x->events.clear();
    return 0;
}

const char* vq_index_profile_class_name(int cls) {
    return (cls >= 0 && cls < VQ_IDX_NCLASS) ? kIdxClassNames[cls] : "";
}

int vq_index_last_search_stats(vq_index* x, int64_t* stats) {
    VQ_CHECK(x && stats, "vq_index_last_search_stats: null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    if (x->stats_at == STATS_COUNTERS) {           // the fp16 path's counters follow the search on its stream
        VQ_HIP(hipStreamSynchronize(x->stream));
        stats_from_counters(x);
    } else if (x->stats_at == STATS_GCOUNTERS) {   // ... and so do the grouped fp16 path's
        VQ_HIP(hipStreamSynchronize(x->stream));
        set_stats(x, STATS_HOST, (int64_t)x->h_gcounters[0], (int64_t)x->h_gcounters[1], (int64_t)x->h_gcounters[2]);
    }
    for (int i = 0; i < 3; ++i) stats[i] = x->stats[i];
    return 0;
}

}  // extern "C"

#ifdef VQ_GEMM_TOWER_STAMPS
// `make STAMPS=1` only: the phase boundaries rescore_verify_small_kernel's workgroup 0 stamped in its last launch (scripts/rescore_stamps.py)
extern "C" int vq_debug_dump_rescore_stamps(void) {
    unsigned long long h[16];
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(vq::g_rs_stamps), sizeof(h));
    static const char* names[9] = {"keys pass A: thread maxima", "wave 8th largest, |q|^2, barrier", "keys pass B: collect, rank", "first-pass rows -> LDS", "query -> LDS, barrier",
                                   "fp64 chains, k-th distance (+ 2nd pass)", "verdict", "rescans", "top-k out"};
    for (int i = 0; i < 9; ++i) fprintf(stderr, "RS_STAMP %-32s %8llu cycles\n", names[i], h[i + 1] - h[i]);
    fprintf(stderr, "RS_STAMP %-32s %8llu cycles\n", "total", h[9] - h[0]);
    return 0;
}
#endif
