// libvq_amd — frame preprocessing handle: Pillow-exact resize on the GPU in front of the encoder, the
// frame extractor's quality statistics, scene-change scores and fused post-processing.  preproc_plan.h decides what is launched.
#include "vq_common.h"
#include "preproc_kernels.h"
#include "preproc_plan.h"
#include "host_buffers.h"
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

namespace vq {
int require_init();
static_assert(RP_PRECISION_BITS == RS_PRECISION_BITS && RP_THREADS == RS_THREADS && RP_ROWS == RSH_ROWS && RP_SC_TILE == SC_TILE &&
              RP_SC_CHUNK_FRAMES == SC_CHUNK_FRAMES && CV_FORM_COPY == PP_COPY && CV_FORM_HALF == PP_HALF && CV_FORM_LINEAR == PP_LINEAR,
              "preproc_plan.h computes with the kernels' geometry");
static_assert(RP_HX_ROW_BYTES == 64 * sizeof(uint4) && RP_HX_KW == 4, "resample_hx_kernel: one uint4 per lane and row, int kw[4] per thread");
}  // namespace vq

using namespace vq;

struct vq_resampler {
    static constexpr const char* TAG = "vq_resampler: ";
    std::mutex mu;
    hipStream_t stream = nullptr, own_stream = nullptr;
    // staged host frames | horizontal intermediate / scene partials | resized frames | statistics and verdicts | compacted survivors
    DevBuf<uint8_t> src{TAG}, tmp{TAG}, dst{TAG}, acc{TAG}, post{TAG};
    DevBuf<int> coef{TAG};       // the four tables of `uploaded`: d_bh | d_kh | d_bv | d_kv (CV_LINEAR: xofs | wx | yofs | wy)
    ResampleTables tables;       // their host copy: what the plan reads
    TableKey uploaded;
    const int *d_bh = nullptr, *d_kh = nullptr, *d_bv = nullptr, *d_kv = nullptr;
    bool dyn_lds_raised = false; // the horizontal kernels' dynamic-LDS limits, on this handle's device
    int64_t out_bytes = 0;
    void* out_ptr = nullptr;     // what vq_resampler_device_output hands out: dst, or post after a compaction
};

namespace {

// launch(std::integral_constant<., V>) for the V of Vs that equals v: a template argument chosen at run time, the launch written once
template <auto... Vs, class T, class F> void dispatch(T v, F&& launch) {
    (void)((v == Vs ? (launch(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
}
int align16(const void* p) { return (int)((uintptr_t)p & 15); }
const ResampleSwitches& process_switches() { static const ResampleSwitches sw = resample_switches_from_env(); return sw; }
size_t env_bytes(const char* name, size_t dflt) {            // the per-call byte budgets: tests set them
    if (const char* e = getenv(name)) { const long long v = atoll(e); if (v > 0) return (size_t)v; }
    return dflt;
}
// a buffer that queued work may still read: wait if and only if it must move
template <class T> int grow(vq_resampler* r, DevBuf<T>& b, size_t n) {
    if ((int64_t)n > b.cap) VQ_HIP(hipStreamSynchronize(r->stream));
    return b.reserve((int64_t)n);
}
int fetch(vq_resampler* r, void* host, const void* dev, size_t bytes) {
    VQ_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, r->stream));
    VQ_HIP(hipStreamSynchronize(r->stream));
    return 0;
}
// the tables of `key` on the device and in r->tables
int ensure_tables(vq_resampler* r, const TableKey& key) {
    if (r->uploaded == key) return 0;
    VQ_HIP(hipStreamSynchronize(r->stream));                 // earlier launches still read the old tables
    r->uploaded = TableKey{};
    build_tables(key, r->tables);
    const std::vector<int>* part[4] = {&r->tables.ch.bounds, &r->tables.ch.kk, &r->tables.cv.bounds, &r->tables.cv.kk};
    const int** d[4] = {&r->d_bh, &r->d_kh, &r->d_bv, &r->d_kv};
    VQ_TRY(r->coef.reserve((int64_t)(part[0]->size() + part[1]->size() + part[2]->size() + part[3]->size())));
    int* at = r->coef.p;
    for (int i = 0; i < 4; at += part[i++]->size()) {
        *d[i] = at;
        VQ_HIP(hipMemcpyAsync(at, part[i]->data(), part[i]->size() * sizeof(int), hipMemcpyHostToDevice, r->stream));
    }
    VQ_HIP(hipStreamSynchronize(r->stream));                 // the host vectors are rebuilt by the next geometry
    r->uploaded = key;
    return 0;
}
int check_frames(const char* who, int n, int h, int w) {
    VQ_CHECK((int64_t)h * w < (int64_t)1 << 30, "%s: frame of %dx%d pixels is too large", who, h, w);
    VQ_CHECK(n <= 65535, "%s: at most 65535 frames per call", who);
    return 0;
}
// one resize: the frames and the filter (the tables' key), and the window of the resized frame that is produced
struct Geometry : TableKey { int crop_top, crop_left, crop_h, crop_w; };
int check_geometry(const char* who, int n, const Geometry& g) {
    VQ_CHECK(n >= 0 && g.h > 0 && g.w > 0 && g.out_h > 0 && g.out_w > 0, "%s: sizes must be positive (n=%d h=%d w=%d out=%dx%d)", who, n, g.h, g.w, g.out_h, g.out_w);
    VQ_CHECK(g.filter == VQ_RESAMPLE_BILINEAR || g.filter == VQ_RESAMPLE_BICUBIC || g.filter == VQ_RESAMPLE_CV_LINEAR,
             "%s: filter %d is not BILINEAR(2), BICUBIC(3) or CV_LINEAR(100)", who, g.filter);
    VQ_CHECK(g.crop_h > 0 && g.crop_w > 0 && g.crop_top >= 0 && g.crop_left >= 0 && g.crop_top + g.crop_h <= g.out_h && g.crop_left + g.crop_w <= g.out_w,
             "%s: crop %dx%d at (%d,%d) does not fit the %dx%d resized frame", who, g.crop_h, g.crop_w, g.crop_top, g.crop_left, g.out_h, g.out_w);
    VQ_TRY(check_frames(who, n, g.h, g.w));
    VQ_CHECK(g.crop_h <= 65535 && g.h <= 65535 * RSH_ROWS, "%s: at most 65535 frames per call and 65535 output rows", who);
    return 0;
}
// n frames of one size: a list of host pointers, or contiguous frames at `base` on the host or on the device
struct Frames { const uint8_t* const* list; const uint8_t* base; bool on_device; bool any() const { return list || base; } };
int check_list(const char* who, const Frames& f, int n) {
    if (f.list) for (int i = 0; i < n; ++i) VQ_CHECK(f.list[i], "%s: frame %d is null", who, i);
    return 0;
}
// run(d_src, first, m) over the frames in slices of `slice` (device-resident frames: one slice, where they are).  Host frames are
// staged in r->src (the caller has waited: it may move) behind `lead` frame slots the caller keeps, contiguous frames in one copy.
// wait: the host waits after each slice, because what run() writes per slice is reused by the next.
template <class F>
int for_each_slice(vq_resampler* r, const Frames& f, int n, size_t frame_bytes, int slice, int lead, bool wait, F&& run) {
    if (!f.on_device) VQ_TRY(r->src.reserve((int64_t)((size_t)(slice + lead) * frame_bytes)));
    uint8_t* stage = f.on_device ? nullptr : r->src.p + (size_t)lead * frame_bytes;
    auto at = [&](int i) { return f.list ? f.list[i] : f.base + (size_t)i * frame_bytes; };
    for (int i = 0; i < n; i += slice) {
        const int m = std::min(slice, n - i);
        for (int a = 0, b; !f.on_device && a < m; a = b) {
            for (b = a + 1; b < m && at(i + b) == at(i + b - 1) + frame_bytes;) ++b;
            VQ_HIP(hipMemcpyAsync(stage + (size_t)a * frame_bytes, at(i + a), (size_t)(b - a) * frame_bytes, hipMemcpyHostToDevice, r->stream));
        }
        VQ_TRY(run(f.on_device ? f.base : (const uint8_t*)stage, i, m));
        if (wait) VQ_HIP(hipStreamSynchronize(r->stream));
    }
    return 0;
}

// cv2.resize(frame, (out_w, out_h)) — INTER_LINEAR — of n device-resident frames; d_dst gets [n][crop_h][crop_w][3]
int run_device_cv(vq_resampler* r, const uint8_t* d_src, int n, const Geometry& g, uint8_t* d_dst) {
    const dim3 grid(cdiv(g.crop_w * 3, RS_THREADS), g.crop_h, n);
    const CvForm form = cv_form(g.h, g.w, g.out_h, g.out_w, g.crop_top == 0 && g.crop_left == 0 && g.crop_h == g.h && g.crop_w == g.w);
    if (form == CV_FORM_COPY) {
        VQ_HIP(hipMemcpyAsync(d_dst, d_src, (size_t)n * g.h * g.w * 3, hipMemcpyDeviceToDevice, r->stream));
    } else if (form == CV_FORM_HALF) {
        hipLaunchKernelGGL(cv_resize_half_kernel, grid, dim3(RS_THREADS), 0, r->stream, d_src, d_dst, g.h, g.w, g.crop_top, g.crop_left,
                           g.crop_h, g.crop_w);
    } else {
        VQ_TRY(ensure_tables(r, g));
        hipLaunchKernelGGL(cv_resize_linear_kernel, grid, dim3(RS_THREADS), 0, r->stream, d_src, d_dst, r->d_bh, r->d_kh, r->d_bv,
                           r->d_kv, g.h, g.w, g.crop_top, g.crop_left, g.crop_h, g.crop_w);
    }
    VQ_HIP(hipGetLastError());
    return 0;
}

// both passes for n device-resident frames; d_dst gets [n][crop_h][crop_w][3]
int run_device(vq_resampler* r, const uint8_t* d_src, int n, const Geometry& g, uint8_t* d_dst) {
    if (g.filter == VQ_RESAMPLE_CV_LINEAR) return run_device_cv(r, d_src, n, g, d_dst);
    VQ_TRY(ensure_tables(r, g));
    ResamplePlan p = plan_resample(r->tables, n, g.crop_top, g.crop_left, g.crop_h, g.crop_w, process_switches());
    if (p.err) return fail(p.err, "%s", p.msg);
    VQ_TRY(grow(r, r->tmp, p.tmp_bytes));                    // queued passes still use the old workspace
    if (!r->dyn_lds_raised) {                                // per device, so per handle (under its lock)
        const std::pair<const void*, size_t> limits[] = {{(const void*)resample_h_kernel<true>, RP_SEG_LDS_MAX}, {(const void*)resample_h_kernel<false>, RP_SEG_LDS_MAX},
                                                         {(const void*)resample_hx_kernel<true>, RP_HX_LDS_MAX}, {(const void*)resample_hx_kernel<false>, RP_HX_LDS_MAX}};
        for (const auto& l : limits) VQ_HIP(hipFuncSetAttribute(l.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.second));
        r->dyn_lds_raised = true;
    }
    uint8_t* tmp = r->tmp.p; const int ksize = r->tables.ch.ksize;
    const dim3 hgrid(p.hgrid[0], p.hgrid[1], p.hgrid[2]);
    dispatch<true, false>(p.dword_store, [&](auto D) {
        constexpr bool DWORD = decltype(D)::value;
        if (p.hx)
            hipLaunchKernelGGL(resample_hx_kernel<DWORD>, hgrid, dim3(RS_THREADS), p.lds, r->stream, d_src, tmp, r->d_bh, r->d_kh, ksize,
                               g.h, g.w, p.row_first, p.rows_needed, g.crop_left, g.crop_w, p.oc, p.pitch_dw, p.tile_pitch, p.spw);
        else
            hipLaunchKernelGGL(resample_h_kernel<DWORD>, hgrid, dim3(RS_THREADS), p.lds, r->stream, d_src, tmp, r->d_bh, r->d_kh, ksize,
                               g.h, g.w, p.row_first, p.rows_needed, g.crop_left, g.crop_w, p.oc, p.pitch_dw, p.tile_pitch);
    });
    VQ_HIP(hipGetLastError());
    plan_vertical(p, g.crop_h, n, align16(tmp), align16(d_dst));
    dispatch<16, 4, 1>(p.vvec, [&](auto V) {
        hipLaunchKernelGGL(resample_v_kernel<decltype(V)::value>, dim3(p.vgrid[0], p.vgrid[1], p.vgrid[2]), dim3(RS_THREADS), 0, r->stream,
                           (const uint8_t*)tmp, d_dst, r->d_bv, r->d_kv, r->tables.cv.ksize, p.rows_needed, p.row_bytes, g.crop_top,
                           g.crop_h, p.row_first);
    });
    VQ_HIP(hipGetLastError());
    return 0;
}

// Scene-change partials + finalise for m device-resident frames; d_res gets [m][3] = {mse, chi, score} per pair
// (pair i = (frame i - 1, frame i); pair 0 = (d_prev, frame 0), or zeros when d_prev is null).  Frames go through in batches whose
// histogram partials fit the scratch budget ($VQ_AMD_SCENE_SCRATCH_BYTES, read per call); a batch's predecessor is the frame before it.
int scene_run_device(vq_resampler* r, const uint8_t* d_frames, int m, int h, int w, const uint8_t* d_prev, double* d_res) {
    const int npix = h * w, tiles = cdiv(npix, SC_TILE);
    const size_t frame_bytes = (size_t)npix * 3;
    const SceneBatch sb = plan_scene_batch(m, tiles, env_bytes("VQ_AMD_SCENE_SCRATCH_BYTES", RP_SCENE_SCRATCH_BYTES));
    VQ_TRY(grow(r, r->tmp, sb.hist_bytes + sb.ssd_bytes));   // queued passes still use the old workspace
    uint32_t *d_hist = (uint32_t*)r->tmp.p, *d_ssd = (uint32_t*)(r->tmp.p + sb.hist_bytes);
    // 16-byte loads need every frame to start on a 16-byte boundary; anything else takes the byte-load kernel
    const bool wide = frame_bytes % 16 == 0 && align16(d_frames) == 0 && align16(d_prev) == 0;
    for (int i = 0; i < m; i += sb.batch) {
        const int mm = std::min(sb.batch, m - i);
        const uint8_t* f = d_frames + (size_t)i * frame_bytes;
        const uint8_t* pv = i == 0 ? d_prev : f - frame_bytes;
        dispatch<true, false>(wide, [&](auto W) {
            hipLaunchKernelGGL(scene_partials_kernel<decltype(W)::value>, dim3(tiles, cdiv(mm, SC_CHUNK_FRAMES)), dim3(RS_THREADS), 0,
                               r->stream, f, pv, d_hist, d_ssd, mm, npix);
        });
        VQ_HIP(hipGetLastError());
        hipLaunchKernelGGL(scene_finalise_kernel, dim3(mm), dim3(256), 0, r->stream, (const uint32_t*)d_hist, (const uint32_t*)d_ssd,
                           d_res + (size_t)i * 3, tiles, npix, pv ? 1 : 0);
        VQ_HIP(hipGetLastError());
    }
    return 0;
}

// fused post-processing (preproc_kernels.h): m device-resident frames -> d_dst [m][out_h][out_w][3] and, in r->acc, the verdict's results (PostLayout)
int post_run_device(vq_resampler* r, const uint8_t* d_src, int m, const Geometry& g, int quality_filter,
                    uint8_t* d_dst, const PostLayout& lay, int band_rows, int n_bands, int fused) {
    const int h = g.h, w = g.w, out_h = g.out_h, out_w = g.out_w;
    uint8_t* acc = r->acc.p; long long* d_part = (long long*)(acc + lay.partials);
    if (fused) {
        const PostFusedPlan f = plan_post_fused(h, w, out_h, out_w, band_rows, align16(d_src), align16(d_dst));
        if (f.mode == PP_LINEAR) VQ_TRY(ensure_tables(r, g));
        const size_t lds = (size_t)pp_lds_bytes(f.lrows - 2, out_w);
        dispatch<PP_COPY, PP_HALF, PP_LINEAR>(f.mode, [&](auto M) { dispatch<true, false>(f.wide_src, [&](auto W) {
            constexpr int MODE = decltype(M)::value;
            constexpr bool WIDE = MODE == PP_COPY && decltype(W)::value;     // 16-byte source loads: copies only
            hipLaunchKernelGGL((postproc_fused_kernel<MODE, WIDE>), dim3(n_bands, m), dim3(RS_THREADS), lds, r->stream, d_src, d_dst, d_part,
                               r->d_bh, r->d_kh, r->d_bv, r->d_kv, h, w, out_h, out_w, band_rows, f.lrows, f.store_vec);
        }); });
        VQ_HIP(hipGetLastError());
    } else {
        VQ_TRY(run_device_cv(r, d_src, m, g, d_dst));      // a row too wide for the LDS plan: resize, then frame_quality_kernel (one partial per frame)
        VQ_HIP(hipMemsetAsync(d_part, 0, (size_t)m * 3 * sizeof(long long), r->stream));
        const int wgs = std::min(cdiv((int64_t)out_h * out_w, RS_THREADS), 1024);
        hipLaunchKernelGGL(frame_quality_kernel, dim3(wgs, m), dim3(RS_THREADS), 0, r->stream, (const uint8_t*)d_dst, d_part, out_h, out_w);
        VQ_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(postproc_verdict_kernel, dim3(1), dim3(RS_THREADS), 0, r->stream, (const long long*)d_part, m, n_bands,
                       (long long)out_h * out_w, quality_filter, (long long*)(acc + lay.res), acc + lay.keep, (int*)(acc + lay.prefix));
    VQ_HIP(hipGetLastError());
    return 0;
}

int postprocess(const char* who, vq_resampler* r, const Frames& f, int n, int h, int w, int out_h, int out_w, int quality_filter,
                uint8_t* out, int64_t* n_kept, uint8_t* keep, int64_t* sums) {
    VQ_TRY(require_init());
    VQ_CHECK(r && n >= 0 && h > 0 && w > 0 && out_h >= 0 && out_w >= 0 && (out_h == 0) == (out_w == 0) && n_kept &&
             (n == 0 || (f.any() && keep)), "%s: bad argument", who);
    if (out_h == 0) { out_h = h; out_w = w; }
    VQ_CHECK((int64_t)out_h * out_w <= PP_MAX_PIXELS, "%s: output of %dx%d pixels is too large (at most 2^21 pixels: the integer "
             "verdict must stay inside int64)", who, out_h, out_w);
    const Geometry g{{h, w, VQ_RESAMPLE_CV_LINEAR, out_h, out_w}, 0, 0, out_h, out_w};
    VQ_TRY(check_geometry(who, n, g));
    *n_kept = 0;
    if (n == 0) return 0;
    VQ_TRY(check_list(who, f, n));
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t frame_bytes = (size_t)h * w * 3, ob = (size_t)out_h * out_w * 3;
    int band_rows, n_bands, fused; pp_plan(out_h, out_w, &band_rows, &n_bands, &fused);
    const bool need_stats = quality_filter || sums;
    const int slice = f.on_device ? n : slice_frames(n, frame_bytes, env_bytes("VQ_AMD_POSTPROC_SLICE_BYTES", RP_SLICE_BYTES));
    const bool single = slice >= n;
    VQ_HIP(hipStreamSynchronize(r->stream));                 // the buffers below may move; an earlier result may still be read
    r->out_ptr = nullptr; r->out_bytes = 0;                  // a call that fails half way leaves no result behind
    VQ_TRY(r->dst.reserve((int64_t)((size_t)slice * ob)));
    if (!single) VQ_TRY(r->post.reserve((int64_t)((size_t)n * ob)));
    const PostLayout lay(slice, n_bands);
    if (need_stats) VQ_TRY(r->acc.reserve((int64_t)lay.total));
    std::vector<long long> res(1 + (size_t)slice * 3);
    int64_t kept_total = 0;
    void* result = r->dst.p;
    VQ_TRY(for_each_slice(r, f, n, frame_bytes, slice, 0, true, [&](const uint8_t* d_src, int i, int m) {
        if (!need_stats) {                                   // nothing to decide: the resize alone, straight into its final place
            uint8_t* target = single ? r->dst.p : r->post.p + (size_t)i * ob;
            VQ_TRY(run_device_cv(r, d_src, m, g, target));
            memset(keep + i, 1, (size_t)m);
            result = single ? r->dst.p : r->post.p;
            kept_total += m;
            return 0;
        }
        VQ_TRY(post_run_device(r, d_src, m, g, quality_filter, r->dst.p, lay, band_rows, n_bands, fused));
        VQ_HIP(hipMemcpyAsync(res.data(), r->acc.p + lay.res, (1 + (size_t)m * 3) * sizeof(long long), hipMemcpyDeviceToHost, r->stream));
        VQ_HIP(hipMemcpyAsync(keep + i, r->acc.p + lay.keep, (size_t)m, hipMemcpyDeviceToHost, r->stream));
        VQ_HIP(hipStreamSynchronize(r->stream));             // the host needs the count to place the next slice's survivors
        const int64_t kept = res[0];
        if (sums) memcpy(sums + (size_t)i * 3, res.data() + 1, (size_t)m * 3 * sizeof(long long));
        if (single && kept == m) {
            result = r->dst.p;                               // everything kept: the resized buffer is the result
        } else {
            if (single) VQ_TRY(grow(r, r->post, (size_t)kept * ob));
            result = r->post.p;
            if (kept > 0) {
                uint8_t* target = r->post.p + (size_t)kept_total * ob;
                const bool wide = ob % 16 == 0;              // hipMalloc'd bases are 16-byte aligned, and so is every frame slot then
                const dim3 grid(std::max(1, std::min(cdiv((int64_t)(wide ? ob / 16 : ob), RS_THREADS), 64)), m);
                dispatch<true, false>(wide, [&](auto W) {
                    hipLaunchKernelGGL(postproc_gather_kernel<decltype(W)::value>, grid, dim3(RS_THREADS), 0, r->stream, (const uint8_t*)r->dst.p,
                                       target, (const uint8_t*)(r->acc.p + lay.keep), (const int*)(r->acc.p + lay.prefix), ob);
                });
                VQ_HIP(hipGetLastError());
            }
        }
        kept_total += kept;
        return 0;
    }));
    r->out_ptr = result;
    r->out_bytes = (int64_t)((size_t)kept_total * ob);
    if (out && kept_total > 0) VQ_TRY(fetch(r, out, result, (size_t)kept_total * ob));
    *n_kept = kept_total;
    return 0;
}

// host frames in; the result in r->dst and, with `out`, on the host
int resize_host(const char* who, vq_resampler* r, const Frames& f, int n, const Geometry& g, uint8_t* out) {
    VQ_TRY(require_init());
    VQ_CHECK(r && (n <= 0 || f.any()), "%s: null argument", who);
    VQ_TRY(check_geometry(who, n, g));
    if (n == 0) return 0;
    VQ_TRY(check_list(who, f, n));
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t frame_bytes = (size_t)g.h * g.w * 3, ob_frame = (size_t)g.crop_h * g.crop_w * 3;
    VQ_HIP(hipStreamSynchronize(r->stream));
    VQ_TRY(r->dst.reserve((int64_t)((size_t)n * ob_frame)));
    r->out_bytes = (int64_t)((size_t)n * ob_frame); r->out_ptr = r->dst.p;
    VQ_TRY(for_each_slice(r, f, n, frame_bytes, slice_frames(n, frame_bytes, RP_SLICE_BYTES), 0, true, [&](const uint8_t* d_src, int i, int m) {
        return run_device(r, d_src, m, g, r->dst.p + (size_t)i * ob_frame);
    }));
    return out ? fetch(r, out, r->dst.p, (size_t)n * ob_frame) : 0;
}

}  // namespace

extern "C" {

int vq_resampler_create(vq_resampler** out) {
    VQ_TRY(require_init());
    VQ_CHECK(out, "vq_resampler_create: null argument");
    vq_resampler* r = new vq_resampler();
    hipError_t e = hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete r; return fail(VQ_ERR_HIP, "vq_resampler_create: stream: %s", hipGetErrorString(e)); }
    r->stream = r->own_stream;
    *out = r;
    return 0;
}

int vq_resampler_destroy(vq_resampler* r) {
    if (!r) return 0;
    (void)hipStreamSynchronize(r->stream);
    const hipStream_t own = r->own_stream;
    delete r;                                                // frees the buffers
    if (own) (void)hipStreamDestroy(own);
    return 0;
}

int vq_resampler_set_stream(vq_resampler* r, void* hip_stream) {
    VQ_CHECK(r, "vq_resampler_set_stream: null handle");
    std::lock_guard<std::mutex> lk(r->mu);
    VQ_HIP(hipStreamSynchronize(r->stream));
    r->stream = hip_stream ? (hipStream_t)hip_stream : r->own_stream;
    return 0;
}

int vq_resampler_synchronize(vq_resampler* r) {
    VQ_CHECK(r, "vq_resampler_synchronize: null handle");
    hipStream_t s;
    { std::lock_guard<std::mutex> lk(r->mu); s = r->stream; }    // set_stream writes it under the lock; the wait itself is outside
    VQ_HIP(hipStreamSynchronize(s));
    return 0;
}

int vq_resampler_run_u8_device(vq_resampler* r, const uint8_t* d_frames, int n, int h, int w, int filter,
                               int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, uint8_t* d_out) {
    VQ_TRY(require_init());
    VQ_CHECK(r && (n == 0 || d_frames), "vq_resampler_run_u8_device: null argument");
    const Geometry g{{h, w, filter, out_h, out_w}, crop_top, crop_left, crop_h, crop_w};
    VQ_TRY(check_geometry("vq_resampler_run_u8_device", n, g));
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t ob = (size_t)n * crop_h * crop_w * 3;
    if (!d_out) {
        VQ_TRY(grow(r, r->dst, ob));                         // a reader of the old buffer may be queued
        r->out_ptr = d_out = r->dst.p;
        r->out_bytes = (int64_t)ob;
    }
    return run_device(r, d_frames, n, g, d_out);
}

int vq_resampler_run_u8_list(vq_resampler* r, const uint8_t* const* frames, int n, int h, int w, int filter,
                             int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, uint8_t* out) {
    return resize_host("vq_resampler_run_u8_list", r, Frames{frames, nullptr, false}, n, {{h, w, filter, out_h, out_w}, crop_top, crop_left, crop_h, crop_w}, out);
}

int vq_resampler_run_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int filter,
                        int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, uint8_t* out) {
    return resize_host("vq_resampler_run_u8", r, Frames{nullptr, frames, false}, n, {{h, w, filter, out_h, out_w}, crop_top, crop_left, crop_h, crop_w}, out);
}

int vq_resampler_device_output(vq_resampler* r, void** d_ptr, int64_t* bytes) {
    VQ_CHECK(r && d_ptr, "vq_resampler_device_output: null argument");
    std::lock_guard<std::mutex> lk(r->mu);
    *d_ptr = r->out_ptr ? r->out_ptr : r->dst.p;
    if (bytes) *bytes = r->out_bytes;
    return 0;
}

int vq_clip_processor_geometry(int h, int w, int size, int crop, int* resized_h, int* resized_w, int* crop_top, int* crop_left) {
    VQ_CHECK(h > 0 && w > 0 && size > 0 && crop > 0 && crop <= size && resized_h && resized_w && crop_top && crop_left,
             "vq_clip_processor_geometry: bad argument");
    // transformers image_transforms.py:295-299: the short edge becomes `size`, the long one int(size * long / short)
    const int shrt = w <= h ? w : h, lng = w <= h ? h : w;
    const int new_long = (int)((int64_t)size * lng / shrt);
    *resized_h = w <= h ? new_long : size;
    *resized_w = w <= h ? size : new_long;
    *crop_top = (*resized_h - crop) / 2;
    *crop_left = (*resized_w - crop) / 2;
    return 0;
}

int vq_frame_quality_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int on_device,
                        double* mean_brightness, double* laplacian_var) {
    VQ_TRY(require_init());
    VQ_CHECK(r && n >= 0 && h > 0 && w > 0 && (n == 0 || (frames && mean_brightness && laplacian_var)), "vq_frame_quality_u8: bad argument");
    VQ_TRY(check_frames("vq_frame_quality_u8", n, h, w));
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t frame_bytes = (size_t)h * w * 3;
    VQ_HIP(hipStreamSynchronize(r->stream));
    VQ_TRY(r->acc.reserve((int64_t)((size_t)n * 3 * sizeof(long long))));
    long long* d_acc = (long long*)r->acc.p;
    VQ_HIP(hipMemsetAsync(d_acc, 0, (size_t)n * 3 * sizeof(long long), r->stream));
    const int wgs = std::min(cdiv((int64_t)h * w, RS_THREADS), 1024);
    const int slice = on_device ? n : slice_frames(n, frame_bytes, RP_SLICE_BYTES);
    VQ_TRY(for_each_slice(r, Frames{nullptr, frames, on_device != 0}, n, frame_bytes, slice, 0, !on_device, [&](const uint8_t* d, int i, int m) {
        hipLaunchKernelGGL(frame_quality_kernel, dim3(wgs, m), dim3(RS_THREADS), 0, r->stream, d, d_acc + (size_t)i * 3, h, w);
        VQ_HIP(hipGetLastError());
        return 0;
    }));
    std::vector<long long> acc((size_t)n * 3);
    VQ_TRY(fetch(r, acc.data(), d_acc, acc.size() * sizeof(long long)));
    const double npix = (double)h * w;
    for (int i = 0; i < n; ++i) {
        mean_brightness[i] = (double)acc[3 * i] / (npix * 3.0);
        // var = E[L^2] - E[L]^2 from exact integer sums: (N*S2 - S1^2) / N^2
        const __int128 num = (__int128)((int64_t)h * w) * acc[3 * i + 2] - (__int128)acc[3 * i + 1] * acc[3 * i + 1];
        laplacian_var[i] = (double)((long double)num / ((long double)npix * (long double)npix));
    }
    return 0;
}

int vq_frame_scene_scores_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int on_device,
                             const uint8_t* prev_frame, double* score, double* mse, double* hist_diff) {
    VQ_TRY(require_init());
    VQ_CHECK(r && n >= 0 && h > 0 && w > 0 && (n == 0 || (frames && score)), "vq_frame_scene_scores_u8: bad argument");
    VQ_CHECK((int64_t)h * w <= (int64_t)1 << 24, "vq_frame_scene_scores_u8: frame of %dx%d pixels is too large (at most 2^24 pixels: "
             "histogram counts must stay exact in float32)", h, w);
    VQ_TRY(check_frames("vq_frame_scene_scores_u8", n, h, w));
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    const size_t frame_bytes = (size_t)h * w * 3;
    VQ_HIP(hipStreamSynchronize(r->stream));
    VQ_TRY(r->acc.reserve((int64_t)((size_t)n * 3 * sizeof(double))));
    double* d_res = (double*)r->acc.p;
    if (on_device) {
        VQ_TRY(scene_run_device(r, frames, n, h, w, prev_frame, d_res));
    } else {
        // the staging buffer's leading slot holds the frame before the slice (the caller's prev_frame, then each slice's last
        // frame, carried device to device).  No wait between slices: nothing but the staging buffer is reused.
        const int slice = slice_frames(n, frame_bytes, env_bytes("VQ_AMD_SCENE_SLICE_BYTES", RP_SLICE_BYTES));
        bool have_prev = prev_frame != nullptr;
        VQ_TRY(for_each_slice(r, Frames{nullptr, frames, false}, n, frame_bytes, slice, 1, false, [&](const uint8_t* d, int i, int m) {
            uint8_t* lead = r->src.p;
            if (i == 0 && have_prev) VQ_HIP(hipMemcpyAsync(lead, prev_frame, frame_bytes, hipMemcpyHostToDevice, r->stream));
            VQ_TRY(scene_run_device(r, d, m, h, w, have_prev ? lead : nullptr, d_res + (size_t)i * 3));
            if (i + m < n) {
                VQ_HIP(hipMemcpyAsync(lead, d + (size_t)(m - 1) * frame_bytes, frame_bytes, hipMemcpyDeviceToDevice, r->stream));
                have_prev = true;
            }
            return 0;
        }));
    }
    std::vector<double> res((size_t)n * 3);
    VQ_TRY(fetch(r, res.data(), d_res, res.size() * sizeof(double)));
    for (int i = 0; i < n; ++i) {
        if (mse) mse[i] = res[3 * (size_t)i];
        if (hist_diff) hist_diff[i] = res[3 * (size_t)i + 1];
        score[i] = res[3 * (size_t)i + 2];
    }
    return 0;
}

int vq_frame_postprocess_plan(int out_h, int out_w, int* band_rows, int* n_bands, int* fused) {
    VQ_CHECK(out_h > 0 && out_w > 0 && band_rows && n_bands && fused, "vq_frame_postprocess_plan: bad argument");
    VQ_CHECK((int64_t)out_h * out_w <= PP_MAX_PIXELS, "vq_frame_postprocess_plan: output of %dx%d pixels is too large (at most 2^21)", out_h, out_w);
    pp_plan(out_h, out_w, band_rows, n_bands, fused);
    return 0;
}

int vq_frame_postprocess_u8_list(vq_resampler* r, const uint8_t* const* frames, int n, int h, int w, int out_h, int out_w,
                                 int quality_filter, uint8_t* out, int64_t* n_kept, uint8_t* keep, int64_t* sums) {
    return postprocess("vq_frame_postprocess_u8_list", r, Frames{frames, nullptr, false}, n, h, w, out_h, out_w, quality_filter, out, n_kept, keep, sums);
}

int vq_frame_postprocess_u8(vq_resampler* r, const uint8_t* frames, int n, int h, int w, int on_device, int out_h, int out_w,
                            int quality_filter, uint8_t* out, int64_t* n_kept, uint8_t* keep, int64_t* sums) {
    return postprocess("vq_frame_postprocess_u8", r, Frames{nullptr, frames, on_device != 0}, n, h, w, out_h, out_w, quality_filter, out, n_kept, keep, sums);
}

// ---- the plans as values, on a machine without a device (tests/test_preproc_plan_cpu.py) ------------------
int vq_debug_resample_plan(int h, int w, int filter, int out_h, int out_w, int crop_top, int crop_left, int crop_h, int crop_w, int n,
                           int tmp_align, int dst_align, int force_seg, int lds_kb, int spw, vq_resample_plan* out) {
    VQ_CHECK(out && n >= 1 && (filter == VQ_RESAMPLE_BILINEAR || filter == VQ_RESAMPLE_BICUBIC) && tmp_align >= 0 && dst_align >= 0,
             "vq_debug_resample_plan: a result, n >= 1, a Pillow filter and two alignments >= 0");
    const Geometry g{{h, w, filter, out_h, out_w}, crop_top, crop_left, crop_h, crop_w};
    VQ_TRY(check_geometry("vq_debug_resample_plan", n, g));
    ResampleTables t;
    build_tables(g, t);
    ResamplePlan p = plan_resample(t, n, crop_top, crop_left, crop_h, crop_w, ResampleSwitches{force_seg != 0, lds_kb, spw});
    if (p.err) return fail(p.err, "%s", p.msg);
    plan_vertical(p, crop_h, n, tmp_align, dst_align);
    *out = vq_resample_plan{p.row_first, p.rows_needed, (int64_t)p.tmp_bytes, p.hx, p.oc, p.span, p.pitch_dw, p.tile_pitch, (int64_t)p.lds,
                            p.dword_store, p.spw, p.hgrid[0], p.hgrid[1], p.hgrid[2], t.ch.ksize, t.cv.ksize, p.row_bytes, p.vvec, p.vgrid[0],
                            p.vgrid[1], p.vgrid[2]};
    return 0;
}

int vq_debug_preproc_small_plans(int n, int64_t frame_bytes, int64_t slice_budget, int m, int tiles, int64_t scratch_budget,
                                 int post_m, int post_bands, int64_t* out) {
    VQ_CHECK(out && n >= 1 && frame_bytes >= 1 && slice_budget >= 1 && m >= 1 && tiles >= 1 && scratch_budget >= 1 && post_m >= 1 && post_bands >= 1,
             "vq_debug_preproc_small_plans: a result and positive arguments");
    const SceneBatch sb = plan_scene_batch(m, tiles, (size_t)scratch_budget);
    const PostLayout lay(post_m, post_bands);
    const int64_t v[9] = {slice_frames(n, (size_t)frame_bytes, (size_t)slice_budget), sb.batch, (int64_t)sb.hist_bytes, (int64_t)sb.ssd_bytes,
                          (int64_t)lay.partials, (int64_t)lay.res, (int64_t)lay.prefix, (int64_t)lay.keep, (int64_t)lay.total};
    memcpy(out, v, sizeof(v));
    return 0;
}

}  // extern "C"
