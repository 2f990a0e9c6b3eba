// evam_detout.h — SSD DetectionOutput as a rule of this project: raw detector heads (box deltas, class probabilities,
// priors) to the [N, K, 7] blob evam_pp_ssd_rois and postproc.parse_ssd_batch read. HIP-free; the kernels
// (evam_detout_kernels.h), the host helper (evam_pp_detection_output_host) and tests/native/detout_check.cpp all call
// the functions below, so they agree bit for bit. tests/detout_ref.py restates the rule from its text.
//
// EVAM_HD marks what the kernels call too (evam_pp.hip defines it as __host__ __device__ first): evam_expf, the
// decode, jaccard and the order key. detout_image is the rule driven sequentially on the host.
//
// The rule (include/evam_pp.h; OpenVINO DetectionOutput-1 semantics for code_type CENTER_SIZE,
// share_location, normalized priors, variances in the prior tensor, no clipping), per image, all in float32 with no
// contraction (the build passes -ffp-contract=off):
//   1. class c != background, prior p: s = conf[p][c] is a candidate when s is finite and s > confidence_threshold;
//   2. within a class: score descending, ties to the lower p; the first top_k take part;
//   3. a participating candidate is decoded (detout_decode); one whose box has a non-finite value is dropped;
//   4. greedy NMS in that order: kept when jaccard(it, k) <= nms_threshold for every kept k before it;
//   5. of all kept candidates of the image the keep_top_k with the highest score survive (ties: lower class, lower p);
//   6. rows (n, c, s, xmin, ymin, xmax, ymax) ordered by class, then score descending, then p; every row from the
//      survivor count on is (-1, 0, 0, 0, 0, 0, 0).
#ifndef EVAM_DETOUT_H
#define EVAM_DETOUT_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../include/evam_pp.h"

#ifndef EVAM_HD
#define EVAM_HD
#endif

namespace evam {

constexpr int kDetoutMaxTopK = EVAM_DETOUT_MAX_TOP_K;  // top_k and keep_top_k: 1..1024
constexpr int kDetoutMaxClasses = EVAM_DETOUT_MAX_CLASSES;

EVAM_HD inline uint32_t detout_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
EVAM_HD inline float detout_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
EVAM_HD inline bool detout_finite(float f) { return (detout_bits(f) & 0x7F800000u) != 0x7F800000u; }

// exp(x) from +, *, one round-to-nearest (the add and subtract of 1.5 * 2^23) and an exponent insert, so that the host
// and the device produce the same bits; neither side's expf is called. Cody-Waite reduction x = k ln2 + r with ln2 split
// in two (k * 0.693359375 is exact for |k| <= 2^15), then exp(r) = 1 + r + r^2 q(r) with q the degree-5 polynomial of
// Cephes' expf. 2^k is applied as two normal powers of two, so a result in the subnormal range is rounded once.
// evam_expf(0) == 1; NaN -> NaN; x > 89 -> +inf (and earlier, where the product overflows); x < -104 -> 0.
// Measured over every float32 in [-20, 20] against float64 exp rounded to float32: DESIGN.md §3.
EVAM_HD inline float evam_expf(float x) {
    if (x != x) return x + x;
    if (x > 89.0f) return detout_float(0x7F800000u);
    if (x < -104.0f) return 0.0f;
    const float t = x * 1.44269504088896341f + 12582912.0f;
    const float k = t + -12582912.0f;  // round(x / ln2), ties to even
    float r = x + k * -0.693359375f;
    r = r + k * 2.12194440e-4f;
    float q = 1.9875691500e-4f;
    q = q * r + 1.3981999507e-3f;
    q = q * r + 8.3334519073e-3f;
    q = q * r + 4.1665795894e-2f;
    q = q * r + 1.6666665459e-1f;
    q = q * r + 5.0000001201e-1f;
    const float y = (q * (r * r) + r) + 1.0f;
    const int ki = (int)k;  // -150 .. 129
    const int k1 = ki >> 1, k2 = ki - k1;
    const float s1 = detout_float((uint32_t)(k1 + 127) << 23), s2 = detout_float((uint32_t)(k2 + 127) << 23);
    return (y * s1) * s2;
}

struct DetBox {
    float x0, y0, x1, y1;
};

// Step 3: prior (xmin, ymin, xmax, ymax), its four variances, the four deltas. false: a non-finite box value.
EVAM_HD inline bool detout_decode(const float* prior, const float* var, const float* l, DetBox& b) {
    const float pw = prior[2] - prior[0], ph = prior[3] - prior[1];
    const float pcx = (prior[0] + prior[2]) * 0.5f, pcy = (prior[1] + prior[3]) * 0.5f;
    const float cx = ((var[0] * l[0]) * pw) + pcx;
    const float cy = ((var[1] * l[1]) * ph) + pcy;
    const float w = evam_expf(var[2] * l[2]) * pw;
    const float h = evam_expf(var[3] * l[3]) * ph;
    const float hw = w * 0.5f, hh = h * 0.5f;
    b.x0 = cx - hw;
    b.y0 = cy - hh;
    b.x1 = cx + hw;
    b.y1 = cy + hh;
    return detout_finite(b.x0) && detout_finite(b.y0) && detout_finite(b.x1) && detout_finite(b.y1);
}

EVAM_HD inline float detout_area(const DetBox& b) {
    if (b.x1 < b.x0 || b.y1 < b.y0) return 0.0f;
    return (b.x1 - b.x0) * (b.y1 - b.y0);
}

// Step 4's overlap of finite boxes. The division is one IEEE float division.
EVAM_HD inline float detout_jaccard(const DetBox& a, const DetBox& b) {
    if (b.x0 > a.x1 || b.x1 < a.x0 || b.y0 > a.y1 || b.y1 < a.y0) return 0.0f;
    const float ix0 = a.x0 > b.x0 ? a.x0 : b.x0, iy0 = a.y0 > b.y0 ? a.y0 : b.y0;
    const float ix1 = a.x1 < b.x1 ? a.x1 : b.x1, iy1 = a.y1 < b.y1 ? a.y1 : b.y1;
    const float iw = ix1 - ix0, ih = iy1 - iy0;
    if (iw <= 0.0f || ih <= 0.0f) return 0.0f;
    const float inter = iw * ih;
    return inter / ((detout_area(a) + detout_area(b)) - inter);
}
// `it` is dropped when its overlap with a kept box is not <= the threshold (a NaN overlap, inf - inf, suppresses).
EVAM_HD inline bool detout_suppresses(const DetBox& it, const DetBox& kept, float nms_threshold) {
    return !(detout_jaccard(it, kept) <= nms_threshold);
}

// Step 1. The scores of candidates are positive floats: their bit patterns order as unsigned integers.
EVAM_HD inline bool detout_candidate(float s, float confidence_threshold) {
    return detout_finite(s) && s > confidence_threshold;
}
// The order key of a class's candidates: larger key first = score descending, then p ascending. p < 2^31.
EVAM_HD inline uint64_t detout_key(float s, uint32_t p) { return ((uint64_t)detout_bits(s) << 32) | (uint32_t)~p; }
EVAM_HD inline uint32_t detout_key_p(uint64_t key) { return ~(uint32_t)key; }
EVAM_HD inline float detout_key_score(uint64_t key) { return detout_float((uint32_t)(key >> 32)); }

// One output row.
EVAM_HD inline void detout_row(float* row, int n, int c, uint64_t key, const DetBox& b) {
    row[0] = (float)n;
    row[1] = (float)c;
    row[2] = detout_key_score(key);
    row[3] = b.x0;
    row[4] = b.y0;
    row[5] = b.x1;
    row[6] = b.y1;
}
EVAM_HD inline void detout_fill_row(float* row) {
    row[0] = -1.0f;
    row[1] = 0.0f; row[2] = 0.0f; row[3] = 0.0f; row[4] = 0.0f; row[5] = 0.0f; row[6] = 0.0f;
}

// The limits of include/evam_pp.h. 0, or EVAM_PP_ERR_INVALID_ARG with the argument named in msg.
inline int detout_validate(int n, int p, const evam_detout_cfg* cfg, char* msg, size_t cap) {
    if (!cfg) return snprintf(msg, cap, "NULL cfg"), EVAM_PP_ERR_INVALID_ARG;
    if (n < 1 || n > 65535) return snprintf(msg, cap, "n %d outside 1..65535", n), EVAM_PP_ERR_INVALID_ARG;
    if (cfg->num_classes < 2 || cfg->num_classes > kDetoutMaxClasses)
        return snprintf(msg, cap, "num_classes %d outside 2..%d", cfg->num_classes, kDetoutMaxClasses), EVAM_PP_ERR_INVALID_ARG;
    if (p < 1 || (int64_t)p * cfg->num_classes >= ((int64_t)1 << 31))
        return snprintf(msg, cap, "p %d: needs p >= 1 and p * num_classes < 2^31", p), EVAM_PP_ERR_INVALID_ARG;
    if (cfg->background_label < -1 || cfg->background_label >= cfg->num_classes)
        return snprintf(msg, cap, "background_label %d outside -1..%d", cfg->background_label, cfg->num_classes - 1),
               EVAM_PP_ERR_INVALID_ARG;
    if (cfg->top_k < 1 || cfg->top_k > kDetoutMaxTopK)
        return snprintf(msg, cap, "top_k %d outside 1..%d (-1, \"all\", is not served)", cfg->top_k, kDetoutMaxTopK),
               EVAM_PP_ERR_INVALID_ARG;
    if (cfg->keep_top_k < 1 || cfg->keep_top_k > kDetoutMaxTopK)
        return snprintf(msg, cap, "keep_top_k %d outside 1..%d (-1, \"all\", is not served)", cfg->keep_top_k, kDetoutMaxTopK),
               EVAM_PP_ERR_INVALID_ARG;
    if (!detout_finite(cfg->confidence_threshold) || !(cfg->confidence_threshold >= 0.0f))
        return snprintf(msg, cap, "confidence_threshold %g must be finite and >= 0", (double)cfg->confidence_threshold),
               EVAM_PP_ERR_INVALID_ARG;
    if (!detout_finite(cfg->nms_threshold))
        return snprintf(msg, cap, "nms_threshold %g must be finite", (double)cfg->nms_threshold), EVAM_PP_ERR_INVALID_ARG;
    return 0;
}

// The rule for image n, sequentially: loc [P][4], conf [P][C] of that image, priors [2][P][4]; out [K][7].
// Returns the survivor count.
inline uint32_t detout_image(int n, const float* loc, const float* conf, const float* priors, int P,
                             const evam_detout_cfg& cfg, float* out) {
    struct Kept {
        uint64_t key;
        int c;
        DetBox box;
    };
    const int C = cfg.num_classes, K = cfg.keep_top_k;
    const float* var = priors + (size_t)P * 4;
    std::vector<Kept> kept;
    std::vector<uint64_t> keys;
    std::vector<DetBox> boxes;  // the kept boxes of the class at hand
    for (int c = 0; c < C; c++) {
        if (c == cfg.background_label) continue;
        keys.clear();
        for (int p = 0; p < P; p++) {
            const float s = conf[(size_t)p * C + c];
            if (detout_candidate(s, cfg.confidence_threshold)) keys.push_back(detout_key(s, (uint32_t)p));
        }
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        if (keys.size() > (size_t)cfg.top_k) keys.resize((size_t)cfg.top_k);
        boxes.clear();
        for (const uint64_t key : keys) {
            const size_t p = detout_key_p(key);
            DetBox b;
            if (!detout_decode(priors + p * 4, var + p * 4, loc + p * 4, b)) continue;
            bool drop = false;
            for (size_t k = 0; k < boxes.size() && !drop; k++) drop = detout_suppresses(b, boxes[k], cfg.nms_threshold);
            if (drop) continue;
            boxes.push_back(b);
            kept.push_back(Kept{key, c, b});
        }
    }
    if (kept.size() > (size_t)K) {
        // score descending, then class ascending, then p ascending: the key's low word is ~p, so within a score a
        // larger key is a lower p
        std::stable_sort(kept.begin(), kept.end(), [](const Kept& a, const Kept& b) {
            const uint32_t sa = (uint32_t)(a.key >> 32), sb = (uint32_t)(b.key >> 32);
            if (sa != sb) return sa > sb;
            if (a.c != b.c) return a.c < b.c;
            return a.key > b.key;
        });
        kept.resize((size_t)K);
        std::stable_sort(kept.begin(), kept.end(), [](const Kept& a, const Kept& b) {
            if (a.c != b.c) return a.c < b.c;
            return a.key > b.key;
        });
    }
    for (size_t r = 0; r < (size_t)K; r++) {
        float* row = out + r * 7;
        if (r < kept.size()) detout_row(row, n, kept[r].c, kept[r].key, kept[r].box);
        else detout_fill_row(row);
    }
    return (uint32_t)kept.size();
}

}  // namespace evam

#endif  // EVAM_DETOUT_H
