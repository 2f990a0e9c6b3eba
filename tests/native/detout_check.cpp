// The SSD DetectionOutput rule of csrc/evam_detout.h (detout_validate + detout_image: what
// evam_pp_detection_output_host runs) as a stand-alone program for AddressSanitizer / UBSan
// (tests/test_native_detout.py). It reads the cases the test wrote (tests/detout_cases.py), runs the rule with every
// array in an exactly-sized heap allocation, and writes each case's blob and counts for the test to compare with the
// float32 reference of tests/detout_ref.py. Last it writes evam_expf of a few values.
//
// Input (binary, native endian): int32 n_cases, then per case int32 N, P, C, background_label, top_k, keep_top_k,
// float32 confidence_threshold, nms_threshold, then loc [N*P*4], conf [N*P*C], priors [2*P*4] float32.
// Output (binary): per case out [N*K*7] float32 and counts [N] uint32; then int32 m and m pairs (x, evam_expf(x)).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../edge-video-analytics-microservice_amd/csrc/evam_detout.h"

using namespace evam;

template <class T>
static bool rd(FILE* f, T* p, size_t n) {
    return fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: detout_check IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n_cases = 0;
    if (!rd(in, &n_cases, 1)) return 2;
    long images = 0, rows = 0;
    for (int i = 0; i < n_cases; i++) {
        int32_t hd[6];
        float thr[2];
        if (!rd(in, hd, 6) || !rd(in, thr, 2)) return 2;
        const int N = hd[0], P = hd[1];
        evam_detout_cfg cfg{hd[2], hd[3], hd[4], hd[5], thr[0], thr[1]};
        char msg[256];
        if (detout_validate(N, P, &cfg, msg, sizeof(msg))) {
            fprintf(stderr, "case %d refused: %s\n", i, msg);
            return 1;
        }
        const size_t C = (size_t)cfg.num_classes, K = (size_t)cfg.keep_top_k;
        // exactly as many elements as the rule may touch: a read or write past them is a heap overflow
        std::unique_ptr<float[]> loc(new float[(size_t)N * P * 4]), conf(new float[(size_t)N * P * C]);
        std::unique_ptr<float[]> priors(new float[(size_t)2 * P * 4]), blob(new float[(size_t)N * K * 7]);
        std::unique_ptr<uint32_t[]> counts(new uint32_t[N]);
        if (!rd(in, loc.get(), (size_t)N * P * 4) || !rd(in, conf.get(), (size_t)N * P * C) ||
            !rd(in, priors.get(), (size_t)2 * P * 4))
            return 2;
        for (int n = 0; n < N; n++) {
            // each image's rows in an allocation of their own, copied out: a write past K rows is caught per image
            std::unique_ptr<float[]> one(new float[K * 7]);
            counts[n] = detout_image(n, loc.get() + (size_t)n * P * 4, conf.get() + (size_t)n * P * C, priors.get(), P, cfg,
                                     one.get());
            if (counts[n] > K) {
                fprintf(stderr, "case %d image %d: %u survivors for keep_top_k %zu\n", i, n, counts[n], K);
                return 1;
            }
            memcpy(blob.get() + (size_t)n * K * 7, one.get(), sizeof(float) * K * 7);
            rows += counts[n];
        }
        images += N;
        fwrite(blob.get(), sizeof(float), (size_t)N * K * 7, out);
        fwrite(counts.get(), sizeof(uint32_t), (size_t)N, out);
    }
    const float xs[] = {0.0f, -0.0f, 1.0f, -1.0f, 20.0f, -20.0f, 0.34657359f, -0.34657359f, 88.7f, 89.5f, -87.5f, -103.0f,
                        -104.5f, 1e30f, -1e30f};
    const int32_t m = (int32_t)(sizeof(xs) / sizeof(xs[0]));
    fwrite(&m, sizeof(m), 1, out);
    for (float x : xs) {
        const float y = evam_expf(x);
        fwrite(&x, sizeof(x), 1, out);
        fwrite(&y, sizeof(y), 1, out);
    }
    if (evam_expf(0.0f) != 1.0f) {
        fprintf(stderr, "evam_expf(0) != 1\n");
        return 1;
    }
    fclose(in);
    fclose(out);
    printf("detout_check: %d cases, %ld images, %ld survivor rows: all checks passed\n", n_cases, images, rows);
    return 0;
}
