// ssd_rois_check.cpp — the detection-row arithmetic of evam_pp_ssd_rois (csrc/evam_geom.h: ssd_row_rect) compiled
// for the host alone under AddressSanitizer / UBSan (tests/test_native_asan_ssd.py). Rows, transforms and label lists
// live in exactly-sized heap allocations, so a read past a row, a transform or the label list fails the run; the
// values include what a detector never sends but memory may hold: NaN, infinities, +-3e38, denormals, zero and
// negative scales, huge paddings, labels outside int32 — no float-to-int conversion may be undefined. Every accepted
// rect is checked against the rules the host path applies (postproc.roi_rect, pipeline_server.roi_inside).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../edge-video-analytics-microservice_amd/csrc/evam_geom.h"

static int g_fail = 0;
#define CHECK(c, ...)                      \
    do {                                   \
        if (!(c)) {                        \
            if (g_fail++ < 20) {           \
                printf("FAIL %s: ", #c);   \
                printf(__VA_ARGS__);       \
                printf("\n");              \
            }                              \
        }                                  \
    } while (0)

static float odd_value(std::mt19937& rng) {
    static const float v[] = {0.f, -0.f, 1.f, -1.f, 0.5f, 1e-45f, -1e-45f, 3e38f, -3e38f, 2147483648.f, -2147483904.f,
                              std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                              std::numeric_limits<float>::quiet_NaN(), 1.0000001f, 0.99999994f, 4294967296.f};
    return v[rng() % (sizeof(v) / sizeof(v[0]))];
}

int main() {
    std::mt19937 rng(1234);
    std::uniform_real_distribution<float> box(-0.3f, 1.3f), conf(0.f, 1.f);
    long accepted = 0, rows = 0;
    for (int it = 0; it < 20000; it++) {
        const int W = 2 * (1 + (int)(rng() % 1000)), H = 2 * (1 + (int)(rng() % 600));
        const int TW = 1 + (int)(rng() % 640), TH = 1 + (int)(rng() % 640);
        const int k = 1 + (int)(rng() % 6);
        float* det = new float[(size_t)k * 7];  // exactly sized: a read of element 7 of the last row is caught
        for (int r = 0; r < k; r++) {
            float* row = det + r * 7;
            row[0] = 0.f;
            row[1] = (float)(int)(rng() % 5);
            row[2] = conf(rng);
            const float x0 = box(rng), y0 = box(rng);
            row[3] = x0; row[4] = y0; row[5] = x0 + conf(rng) * 0.6f; row[6] = y0 + conf(rng) * 0.6f;
            if (rng() % 4 == 0) row[1 + rng() % 6] = odd_value(rng);
        }
        evam_transform* xf = nullptr;
        if (rng() % 3) {
            xf = new evam_transform[1];
            const int kind = rng() % 4;
            xf->scale_x = kind == 3 ? odd_value(rng) : (float)TW / W;
            xf->scale_y = kind == 3 ? odd_value(rng) : (float)TH / H;
            xf->crop_x = kind == 2 ? (int)(rng() % 50) : 0;
            xf->crop_y = 0;
            xf->crop_w = kind == 0 ? W : W - xf->crop_x;
            xf->crop_h = H;
            xf->pad_x = kind == 1 ? (int)(rng() % 40) - 20 : (kind == 3 ? INT32_MAX : 0);
            xf->pad_y = kind == 3 ? INT32_MIN : 0;
            xf->resized_w = TW;
            xf->resized_h = kind == 1 ? TH / 2 + 1 : TH;
        }
        const int n_labels = (int)(rng() % 4);
        int32_t* labels = (rng() % 2) ? new int32_t[(size_t)n_labels + 1] : nullptr;  // [n_labels] is never read
        if (labels) {
            for (int j = 0; j < n_labels; j++) labels[j] = (int32_t)(rng() % 5);
            labels[n_labels] = 3;
        }
        int32_t* lab = nullptr;
        if (labels) {  // the list the function sees: exactly n_labels entries (at least a one-entry allocation)
            lab = new int32_t[(size_t)(n_labels ? n_labels : 1)];
            memcpy(lab, labels, sizeof(int32_t) * (size_t)n_labels);
        }
        const float thr = rng() % 5 ? 0.5f : odd_value(rng);
        for (int r = 0; r < k; r++) {
            const float* row = det + r * 7;
            int x = -77, y = -77, w = -77, h = -77;
            const bool ok = evam::ssd_row_rect(row, xf, W, H, TW, TH, thr, lab, n_labels, x, y, w, h);
            const bool again = evam::ssd_row_rect(row, xf, W, H, TW, TH, thr, lab, n_labels, x, y, w, h);
            CHECK(ok == again, "not deterministic");
            rows++;
            if (!ok) continue;
            accepted++;
            CHECK(row[2] >= thr, "accepted below the threshold");
            for (int j = 3; j < 7; j++) CHECK(std::isfinite(row[j]), "accepted a non-finite box");
            CHECK(w > 0 && h > 0, "w %d h %d", w, h);
            CHECK(x >= 0 && y >= 0 && x <= W && y <= H && w <= W && h <= H, "rect (%d,%d,%d,%d) in %dx%d", x, y, w, h, W, H);
            CHECK(std::min(x + w, W) - std::max(x, 0) > 0 && std::min(y + h, H) - std::max(y, 0) > 0, "rect outside");
            if (lab) {
                bool hit = false;
                for (int j = 0; j < n_labels; j++) hit |= lab[j] == (int32_t)row[1];
                CHECK(hit, "label %g not in the list", row[1]);
            }
            if (!xf) {  // identity: postproc.roi_rect on the clipped float32 box, in double
                auto cl = [](double v) { return v < 0 ? 0. : (v > 1 ? 1. : v); };
                const double a = cl(row[3]), b = cl(row[5]);
                CHECK(x == (int)std::floor(a * W + 0.5) && w == (int)std::floor((b - a) * W + 0.5), "x %d w %d", x, w);
            }
        }
        delete[] det;
        delete[] xf;
        delete[] labels;
        delete[] lab;
    }
    printf("ssd rows: %ld evaluated, %ld accepted, %d failures\n", rows, accepted, g_fail);
    CHECK(accepted > 5000, "too few accepted rows: %ld", accepted);
    if (g_fail) return 1;
    printf("all checks passed\n");
    return 0;
}
