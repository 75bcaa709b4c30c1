// Host-only check of csrc/preproc_plan.h under the sanitizers: the table builders, span_max and the oc search on the smallest and
// most awkward geometries.  No device, no library:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/preproc_plan_check.cpp -o preproc_plan_check
//   ./preproc_plan_check             (prints the number of plans and exits 0)
#include "../video-quierer_amd/csrc/preproc_plan.h"
#include <cstdio>

using namespace vq;

static long plans = 0, refused = 0;

static int check(int h, int w, int filter, int out_h, int out_w, int top, int left, int ch, int cw, int n, const ResampleSwitches& sw) {
    ResampleTables t;
    build_tables(TableKey{h, w, filter, out_h, out_w}, t);
    // every tap of every table stays inside the source axis
    for (int x = 0; x < out_w; ++x)
        if (t.ch.bounds[2 * x] < 0 || t.ch.bounds[2 * x + 1] < 1 || t.ch.bounds[2 * x] + t.ch.bounds[2 * x + 1] > w || t.ch.bounds[2 * x + 1] > t.ch.ksize) return 1;
    for (int y = 0; y < out_h; ++y)
        if (t.cv.bounds[2 * y] < 0 || t.cv.bounds[2 * y + 1] < 1 || t.cv.bounds[2 * y] + t.cv.bounds[2 * y + 1] > h || t.cv.bounds[2 * y + 1] > t.cv.ksize) return 2;
    ResamplePlan p = plan_resample(t, n, top, left, ch, cw, sw);
    ++plans;
    if (p.err) { ++refused; return p.lds > RP_SEG_LDS_MAX ? 0 : 3; }
    for (int oc = 1; oc <= 32; ++oc)
        if (span_max(t.ch.bounds.data(), left, cw, oc) > w) return 4;
    if (!(p.pitch_dw & 1) || !((p.tile_pitch / 4) & 1)) return 5;
    for (int x0 = 0; x0 < cw; x0 += p.oc)       // every segment's taps, straight from the table, fit the staged row with its slack
        for (int x = left + x0; x < left + std::min(x0 + p.oc, cw); ++x)
            if ((t.ch.bounds[2 * x] + t.ch.bounds[2 * x + 1] - t.ch.bounds[2 * (left + x0)]) * 3 + (p.hx ? RP_HX_SLACK : RP_SEG_SLACK) > p.pitch_dw * 4) return 5;
    if (p.hx && (p.pitch_dw * 4 > RP_HX_ROW_BYTES || p.oc * t.ch.ksize > RP_HX_KW * RP_THREADS || p.lds > RP_HX_LDS_MAX)) return 6;
    if (p.row_first < 0 || p.row_first + p.rows_needed > h || (int64_t)p.hgrid[0] * p.spw * p.oc < cw || p.hgrid[1] * RP_ROWS < p.rows_needed) return 7;
    for (int ta : {0, 4, 1})
        for (int da : {0, 4, 1}) {
            plan_vertical(p, ch, n, ta, da);
            if (p.row_bytes % p.vvec || (p.vvec == 16 ? (int64_t)p.vgrid[0] * RP_THREADS * 16 < (int64_t)p.row_bytes * ch : p.vgrid[0] * RP_THREADS * p.vvec < p.row_bytes)) return 8;
        }
    return 0;
}

int main() {
    // (h, w, out_h, out_w): 1 x 1, 1 x N and N x 1, out_w = 1, a column too wide for a request, upscales
    const int geo[][4] = {{1, 1, 1, 1}, {1, 1, 4, 4}, {1, 9, 1, 1}, {1, 9, 3, 224}, {9, 1, 224, 3}, {2, 3, 5, 7}, {5, 5461, 9, 31}, {5, 5461, 9, 1},
                          {3, 6000, 2, 1}, {37, 53, 24, 40}, {37, 53, 224, 224}, {90, 160, 224, 224}, {1080, 1920, 224, 224}, {1080, 1920, 224, 398},
                          {1, 4096, 1, 1024}, {7, 33, 700, 1024}, {2, 16, 2, 1024}};
    const ResampleSwitches sws[] = {{false, 0, 0}, {true, 0, 0}, {false, 1, 0}, {false, 32, 0}, {false, 200, 0}, {false, 0, 1}, {false, 0, 1000}};
    for (const auto& g : geo)
        for (int filter : {VQ_RESAMPLE_BILINEAR, VQ_RESAMPLE_BICUBIC})
            for (const ResampleSwitches& sw : sws)
                for (int n : {1, 3, 65535}) {
                    const int oh = g[2], ow = g[3];
                    // whole; one column at the right edge; a window off the left edge whose width is no multiple of 4
                    const int crops[][4] = {{0, 0, oh, ow}, {oh - 1, ow - 1, 1, 1}, {oh / 3, ow > 2 ? 1 : 0, oh - oh / 3, ow > 2 ? ow - 2 : ow}};
                    for (const auto& c : crops)
                        if (const int rc = check(g[0], g[1], filter, oh, ow, c[0], c[1], c[2], c[3], n, sw)) {
                            printf("FAILED (%d): %dx%d -> %dx%d filter %d crop %d,%d,%d,%d n %d\n", rc, g[0], g[1], oh, ow, filter, c[0], c[1], c[2], c[3], n);
                            return 1;
                        }
                }
    // OpenCV's tables: taps inside the source after the kernel's clipping rule for rows
    for (const auto& g : geo) {
        ResampleTables t;
        build_tables(TableKey{g[0], g[1], VQ_RESAMPLE_CV_LINEAR, g[2], g[3]}, t);
        for (int x = 0; x < g[3]; ++x)
            if (t.ch.bounds[x] < 0 || t.ch.bounds[x] > g[1] - 1 || t.ch.kk[2 * x] + t.ch.kk[2 * x + 1] != 2048) return 1;
        if ((int)t.cv.bounds.size() != g[2] || (int)t.cv.kk.size() != 2 * g[2]) return 1;
    }
    // the small plans at their edges
    if (slice_frames(1, (size_t)1 << 31, 1) != 1 || slice_frames(65535, 3, RP_SLICE_BYTES) != 65535) return 1;
    if (plan_scene_batch(1, 1, 1).batch != 1 || plan_scene_batch(65535, 2048, RP_SCENE_SCRATCH_BYTES).batch != 128) return 1;
    if (PostLayout(1, 1).total != 72 || plan_post_fused(4, 4, 4, 4, 32, 0, 0).mode != CV_FORM_COPY || cv_form(4, 4, 2, 2) != CV_FORM_HALF) return 1;
    printf("preproc_plan_check: %ld plans (%ld refused), clean\n", plans, refused);
    return 0;
}
