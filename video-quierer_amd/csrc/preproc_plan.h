// What the preprocessing handle (vq_preproc.hip) launches, as host arithmetic without HIP: the coefficient tables of a geometry,
// the A/B switches, plan_resample / plan_vertical and the small plans of the other paths (DESIGN.md "The preprocessing host layer").
// The vq_debug_* entry points return it without a GPU (tests/test_preproc_plan_cpu.py); vq_preproc.hip asserts the constants.
#pragma once
#include "../../include/vq_amd.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace vq {

constexpr int RP_PRECISION_BITS = 32 - 8 - 2;                 // Resample.c PRECISION_BITS
constexpr int RP_THREADS = 256, RP_ROWS = 64;                 // threads and source rows of a horizontal workgroup
constexpr int RP_HX_ROW_BYTES = 64 * 16, RP_HX_KW = 4;        // hx: a staged row is ONE wave-wide request; weights in four registers
constexpr int RP_HX_SLACK = 48, RP_SEG_SLACK = 24;            // staged-row slack: 15 / 3 bytes of realignment + the zero-weight over-read
// the oc search's aim (hx: measured 32 / 40 / 48 / 64 KB: 0.184 / 0.161 / 0.174 / 0.184 ms per 64 1080p frames) and the kernels' limits
constexpr size_t RP_HX_LDS = 40 << 10, RP_SEG_LDS = 48 << 10, RP_HX_LDS_MAX = 96 << 10, RP_SEG_LDS_MAX = 150 << 10;
constexpr int RP_SC_TILE = 8192, RP_SC_CHUNK_FRAMES = 8;      // scene pass: pixels / frames per workgroup
constexpr size_t RP_SLICE_BYTES = (size_t)512 << 20, RP_SCENE_SCRATCH_BYTES = (size_t)256 << 20;

// ---- Resample.c precompute_coeffs + normalize_coeffs_8bpc, in IEEE double like the C original ------------
static inline double filt_bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}
static inline double filt_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
struct Coeffs {
    int ksize = 0;
    std::vector<int> bounds;     // [out][2]: first tap, tap count          (CV_LINEAR: [out] first tap)
    std::vector<int> kk;         // [out][ksize] fixed-point weights        (CV_LINEAR: [out][2] 11-bit weights)
};
static inline void precompute_coeffs(int in_size, int out_size, int filter, Coeffs& c) {
    double (*fn)(double) = filter == VQ_RESAMPLE_BICUBIC ? filt_bicubic : filt_bilinear;
    const double fsupport = filter == VQ_RESAMPLE_BICUBIC ? 2.0 : 1.0;
    const double in0 = 0.0, in1 = (double)in_size;
    double scale = (in1 - in0) / out_size, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = fsupport * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;       // Resample.c's row length; rows here are padded to x4 with zeros
    c.ksize = (ksize + 3) & ~3;
    c.bounds.assign((size_t)out_size * 2, 0);
    c.kk.assign((size_t)out_size * c.ksize, 0);
    std::vector<double> w(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = fn((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int* k = &c.kk[(size_t)xx * c.ksize];
        for (int x = 0; x < xmax; ++x) {
            double v = w[x];
            if (ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << RP_PRECISION_BITS)) : (int)(0.5 + v * (1 << RP_PRECISION_BITS));
        }
        c.bounds[2 * xx] = xmin;
        c.bounds[2 * xx + 1] = xmax;
    }
}

// OpenCV resize.cpp INTER_LINEAR tables for one axis: first tap and the two 11-bit weights per output index.
// snap_borders = the horizontal rule (weight 1 on the edge pixel outside [0, src-1)); rows are clipped by the kernel.
static inline void cv_linear_coeffs(int src, int dst, bool snap_borders, std::vector<int>& ofs, std::vector<int>& wts) {
    const double scale = (double)src / dst;
    ofs.resize(dst); wts.resize((size_t)dst * 2);
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (snap_borders) {
            if (s < 0) { f = 0.f; s = 0; }
            if (s >= src - 1) { f = 0.f; s = src - 1; }
        }
        auto sat_short = [](float v) {                       // saturate_cast<short>(v): cvRound (half to even) + clamp
            long r = std::lrint(v);
            return (int)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
        };
        ofs[d] = s;
        wts[2 * d] = sat_short((1.f - f) * 2048.f);
        wts[2 * d + 1] = sat_short(f * 2048.f);
    }
}

// The four host tables of one geometry and the key they were built for.  ch: the horizontal axis (w -> out_w), cv: the vertical one.
struct TableKey {
    int h = 0, w = 0, filter = 0, out_h = 0, out_w = 0;      // h = 0: no tables yet
    bool operator==(const TableKey& o) const { return h == o.h && w == o.w && filter == o.filter && out_h == o.out_h && out_w == o.out_w; }
};
struct ResampleTables { TableKey key; Coeffs ch, cv; };
static inline void build_tables(const TableKey& k, ResampleTables& t) {
    if (k.filter == VQ_RESAMPLE_CV_LINEAR) {
        t.ch.ksize = t.cv.ksize = 0;
        cv_linear_coeffs(k.w, k.out_w, true, t.ch.bounds, t.ch.kk);
        cv_linear_coeffs(k.h, k.out_h, false, t.cv.bounds, t.cv.kk);
    } else {
        precompute_coeffs(k.w, k.out_w, k.filter, t.ch);
        precompute_coeffs(k.h, k.out_h, k.filter, t.cv);
    }
    t.key = k;
}
// A/B switches of the horizontal pass: $VQ_AMD_RSH=seg (never hx), $VQ_AMD_RSH_LDS_KB (the oc search's aim), $VQ_AMD_RSH_SPW; 0 = unset
struct ResampleSwitches { bool force_seg = false; int lds_kb = 0, spw = 0; };
static inline ResampleSwitches resample_switches_from_env() {
    const char *rsh = getenv("VQ_AMD_RSH"), *kb = getenv("VQ_AMD_RSH_LDS_KB"), *spw = getenv("VQ_AMD_RSH_SPW");
    return ResampleSwitches{rsh && !strcmp(rsh, "seg"), kb ? atoi(kb) : 0, spw ? atoi(spw) : 0};
}
struct ResamplePlan {
    int err = 0;                 // VQ_ERR_INVALID with `msg`: a row no LDS image holds
    char msg[160];
    int row_first = 0, rows_needed = 0;  // source rows the crop's output rows touch: what the horizontal pass produces
    size_t tmp_bytes = 0;        // the intermediate [n][rows_needed][crop_w][3]
    bool hx = false;             // resample_hx_kernel (row-block-major), else resample_h_kernel (segment-major)
    int oc = 0, span = 0;        // output columns per segment; the widest source span (pixels) of any segment
    int pitch_dw = 0;            // staged source row, dwords (odd: lanes = rows stream their rows bank-conflict free)
    int tile_pitch = 0;          // result tile row, bytes (an odd number of dwords)
    size_t lds = 0;              // [RP_ROWS][pitch_dw] dwords | [RP_ROWS][tile_pitch] bytes | [oc][ksize] weights
    bool dword_store = false;    // the tile leaves in dwords
    int spw = 1, hgrid[3] = {};  // hx: segments a workgroup walks; the horizontal grid
    int row_bytes = 0, vvec = 0, vgrid[3] = {};  // crop_w * 3; plan_vertical: bytes per access and the vertical grid
};
// widest source span (pixels) of any segment of `oc` output columns
static inline int span_max(const int* bh, int crop_left, int crop_w, int oc) {
    int m = 0;
    for (int x0 = 0; x0 < crop_w; x0 += oc) {
        const int xa = crop_left + x0, xb = crop_left + std::min(x0 + oc, crop_w) - 1;
        m = std::max(m, bh[2 * xb] + bh[2 * xb + 1] - bh[2 * xa]);
    }
    return m;
}
// The Pillow resize of n frames to the crop window.  `t` holds a BILINEAR / BICUBIC geometry.
static inline ResamplePlan plan_resample(const ResampleTables& t, int n, int crop_top, int crop_left, int crop_h, int crop_w,
                                         const ResampleSwitches& sw) {
    ResamplePlan p;
    const int *bv = t.cv.bounds.data(), *bh = t.ch.bounds.data(), ksize = t.ch.ksize;
    p.row_first = bv[2 * crop_top];
    p.rows_needed = bv[2 * (crop_top + crop_h - 1)] + bv[2 * (crop_top + crop_h - 1) + 1] - p.row_first;
    p.tmp_bytes = (size_t)n * p.rows_needed * crop_w * 3;
    p.row_bytes = crop_w * 3;
    // RP_ROWS rows x `oc` columns per workgroup; oc shrinks until the staged span fits (hx: one request per row, weights in registers)
    auto hx_fits = [&]() { return p.pitch_dw * 4 <= RP_HX_ROW_BYTES && p.oc * ksize <= RP_HX_KW * RP_THREADS; };
    p.hx = !sw.force_seg;
    for (int pass = 0; pass < 2; ++pass) {
        const size_t lds_cap = sw.lds_kb > 0 ? (size_t)sw.lds_kb * 1024 : p.hx ? RP_HX_LDS : RP_SEG_LDS;
        for (p.oc = 32;; p.oc = p.oc > 4 ? p.oc - 4 : p.oc - 1) {
            p.span = span_max(bh, crop_left, crop_w, p.oc);
            p.pitch_dw = (p.span * 3 + (p.hx ? RP_HX_SLACK : RP_SEG_SLACK) + 3) / 4 | 1;
            p.tile_pitch = (p.oc * 3 + 3) / 4 * 4;
            if (((p.tile_pitch / 4) & 1) == 0) p.tile_pitch += 4;
            p.lds = (size_t)RP_ROWS * p.pitch_dw * 4 + (size_t)RP_ROWS * p.tile_pitch + (size_t)p.oc * ksize * 4;
            if ((p.lds <= lds_cap && (!p.hx || hx_fits())) || p.oc == 1) break;
        }
        if (!p.hx || (hx_fits() && p.lds <= RP_HX_LDS_MAX)) break;
        p.hx = false;            // a single output column already spans more than a request: the segment-major kernel
    }
    if (p.lds > RP_SEG_LDS_MAX) {
        p.err = VQ_ERR_INVALID;
        snprintf(p.msg, sizeof(p.msg), "vq_resampler: a %d -> %d pixel row needs %zu bytes of LDS per workgroup", t.key.w, t.key.out_w, p.lds);
        return p;
    }
    p.dword_store = (crop_w % 4 == 0) && (p.oc % 4 == 0);
    const int nseg = (crop_w + p.oc - 1) / p.oc, yblocks = (p.rows_needed + RP_ROWS - 1) / RP_ROWS;
    if (p.hx) {                  // segments per workgroup: walk as many as leaves ~4+ rounds of workgroups on the chip
        const int64_t rounds = ((int64_t)4 * 768 + (int64_t)yblocks * n - 1) / ((int64_t)yblocks * n);
        const int xsplit = (int)std::max<int64_t>(1, std::min<int64_t>(nseg, rounds));
        p.spw = sw.spw > 0 ? std::min(sw.spw, nseg) : (nseg + xsplit - 1) / xsplit;
    }
    p.hgrid[0] = (nseg + p.spw - 1) / p.spw; p.hgrid[1] = yblocks; p.hgrid[2] = n;
    return p;
}
// The vertical pass: 16-, 4- or 1-byte accesses by the row length and the two bases (address & 15 of the intermediate and the output)
static inline void plan_vertical(ResamplePlan& p, int crop_h, int n, int tmp_align, int dst_align) {
    const int rb = p.row_bytes;
    p.vvec = (rb % 16 == 0 && dst_align % 16 == 0 && tmp_align % 16 == 0) ? 16 : (rb % 4 == 0 && dst_align % 4 == 0) ? 4 : 1;
    p.vgrid[0] = p.vvec == 16 ? (int)(((int64_t)(rb / 16) * crop_h + RP_THREADS - 1) / RP_THREADS) : (rb / p.vvec + RP_THREADS - 1) / RP_THREADS;
    p.vgrid[1] = p.vvec == 16 ? 1 : crop_h; p.vgrid[2] = n;
}

// cv2.resize's three forms (the values are preproc_kernels.h's PP_COPY / PP_HALF / PP_LINEAR); whole: the crop is the whole output
enum CvForm : int { CV_FORM_COPY = 0, CV_FORM_HALF = 1, CV_FORM_LINEAR = 2 };
static inline CvForm cv_form(int h, int w, int out_h, int out_w, bool whole = true) {
    return (out_h == h && out_w == w && whole) ? CV_FORM_COPY : (h == 2 * out_h && w == 2 * out_w) ? CV_FORM_HALF : CV_FORM_LINEAR;
}
// The fused post-processing launch: form, 16-byte source loads (copies only), store width, LDS rows of a band
struct PostFusedPlan { int mode; bool wide_src; int store_vec, lrows; };
static inline PostFusedPlan plan_post_fused(int h, int w, int out_h, int out_w, int band_rows, int src_align, int dst_align) {
    const int rb = out_w * 3, mode = cv_form(h, w, out_h, out_w);
    return PostFusedPlan{mode, mode == CV_FORM_COPY && rb % 16 == 0 && src_align % 16 == 0,
                         (rb % 16 == 0 && dst_align % 16 == 0) ? 16 : (rb % 4 == 0 && dst_align % 4 == 0) ? 4 : 1, std::min(band_rows, out_h) + 2};
}
// Byte offsets into `acc` for m frames of nb bands: partials [m][nb][3] int64 | res: kept, sums [m][3] int64 | prefix [m] int32 | keep [m]
struct PostLayout {
    size_t partials = 0, res, prefix, keep, total;
    PostLayout(int m, int nb) : res((size_t)m * nb * 3 * sizeof(long long)), prefix(res + (1 + (size_t)m * 3) * sizeof(long long)),
                                keep(prefix + ((size_t)m * 4 + 7) / 8 * 8), total(keep + ((size_t)m + 7) / 8 * 8) {}
};
// Scene pass: frames per batch (whole chunks whose (batch + 1) histogram slots fit `budget`, at least one chunk) and the partials' bytes
struct SceneBatch { int batch; size_t hist_bytes, ssd_bytes; };
static inline SceneBatch plan_scene_batch(int m, int tiles, size_t budget) {
    const size_t slot_bytes = (size_t)tiles * 256 * sizeof(uint32_t);
    const int batch = (int)std::min<size_t>((size_t)m, std::max<size_t>(RP_SC_CHUNK_FRAMES, budget / slot_bytes / RP_SC_CHUNK_FRAMES * RP_SC_CHUNK_FRAMES));
    return SceneBatch{batch, (size_t)(batch + 1) * slot_bytes, (size_t)batch * tiles * sizeof(uint32_t)};
}
// Host frames go up in slices of at most `budget` bytes, at least one frame
static inline int slice_frames(int n, size_t frame_bytes, size_t budget) {
    return (int)std::min<size_t>((size_t)n, std::max<size_t>(1, budget / frame_bytes));
}

}  // namespace vq
