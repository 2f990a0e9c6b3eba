// Stand-alone check of the raw-plane output of csrc/evam_jpeg_dec.h (jdec_planes_host, jdec_planes_row and
// jdec_store_clipped, which the kernel evam_jdec_idct_planes shares), built with -fsanitize=address,undefined
// (tests/test_native_asan_jpeg_planes.py). Every even-sized 4:2:0 file named on the command line is decoded to NV12
// and to I420 planes that are exactly-sized heap blocks: a plane of `rows` rows is (rows - 1) * pitch + row bytes
// long, so a store below the last row, or behind the last row's pixels, is a heap overflow; the padding of the rows
// above holds a sentinel that must survive. The planes must equal the component planes of the pixel path (jdec_dc_and_idct_host) cropped, and NV12 must be
// I420 interleaved. Then 5,000 seeded random damaged scans of the good files are decoded the same way: any status,
// no store outside the pixel bytes.
//   usage: jpeg_planes_check file... [--damaged file...]
//   Files in front of the flag must decode with status 0 and seed the random scans; files the planes path does not
//   serve (or the parse refuses) are counted and skipped.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../edge-video-analytics-microservice_amd/csrc/evam_jpeg_dec.h"

namespace {

int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

constexpr uint8_t kSentinel = 0xA5;

struct Plane {
    uint8_t* p = nullptr;
    int pitch = 0, rows = 0, row = 0;
    size_t bytes() const { return (size_t)(rows - 1) * pitch + row; }
    void alloc(int rows_, int row_, int extra) {
        rows = rows_; row = row_; pitch = (row + 15) / 16 * 16 + extra;
        if (posix_memalign((void**)&p, 16, bytes())) exit(2);
        memset(p, kSentinel, bytes());
    }
    // the padding of every row but the last (which has none) still holds the sentinel
    bool padding_intact() const {
        for (int y = 0; y + 1 < rows; y++)
            for (int x = row; x < pitch; x++)
                if (p[(size_t)y * pitch + x] != kSentinel) return false;
        return true;
    }
};

// 0: skipped (refused, or no even-sized 4:2:0 file); 1: decoded
int check_file(const std::vector<uint8_t>& file, const char* what, bool good, int* status_out) {
    evam_jpeg_info info{};
    JdecFile* f = new JdecFile;
    struct Free { JdecFile* p; ~Free() { delete p; } } free_f{f};
    char msg[320];
    JdecGeom g;
    if (jdec_parse(file.data(), file.size(), &info, f, msg, sizeof(msg)) || !jdec_planes_ok(info) || !jdec_geom(info, g))
        return 0;
    int err = 0;
    uint8_t* stream = (uint8_t*)malloc((size_t)f->scan_len + kJdecStreamPad);
    uint32_t* first = (uint32_t*)malloc(((size_t)g.n_int + 1) * sizeof(uint32_t));
    err |= jdec_unstuff_host(file.data() + (file.size() - f->scan_len), f->scan_len, g.n_int, stream, first) != 0;
    std::vector<int16_t> raw((size_t)g.n_blk * 64, 0);
    JdecScan sc{stream, f, g.nluma, g.bpm};
    for (int k = 0; k < g.n_int; k++) {
        const uint32_t m0 = g.ri > 0 ? (uint32_t)k * g.ri : 0u;
        uint32_t m1 = g.ri > 0 ? m0 + g.ri : (uint32_t)g.n_mcu;
        if (m1 > (uint32_t)g.n_mcu) m1 = g.n_mcu;
        uint32_t p = first[k] * 8, bz = 0;
        const uint32_t end = first[k + 1] * 8, blk0 = m0 * g.bpm, limit = m1 * g.bpm;
        const uint32_t done = jdec_run(sc, p, bz, end, end, raw.data(), blk0, limit, err);
        if (blk0 + done < limit) err = 1;
    }
    free(first); free(stream);

    // the pixel path's component planes: the reference for the cropped ones
    std::vector<int16_t> coef = raw;
    uint8_t* comp = (uint8_t*)malloc(g.plane_bytes);
    int err_ref = err;
    jdec_dc_and_idct_host(g, *f, coef.data(), comp, err_ref);

    Plane nv[2], iy[3];
    const int extra = (g.W / 2) % 3 * 16;  // pitches of 0, 16 or 32 bytes beyond the rounded row
    nv[0].alloc(g.H, g.W, extra); nv[1].alloc(g.H / 2, g.W, extra + 16);
    iy[0].alloc(g.H, g.W, extra); iy[1].alloc(g.H / 2, g.W / 2, extra + 16); iy[2].alloc(g.H / 2, g.W / 2, extra);
    JdecPlanesOut on{}, oi{};
    for (int p = 0; p < 2; p++) { on.p[p] = nv[p].p; on.pitch[p] = nv[p].pitch; }
    for (int p = 0; p < 3; p++) { oi.p[p] = iy[p].p; oi.pitch[p] = iy[p].pitch; }
    int err_n = err, err_i = err;
    coef = raw;
    jdec_planes_host<true>(g, *f, coef.data(), on, err_n);
    coef = raw;
    jdec_planes_host<false>(g, *f, coef.data(), oi, err_i);
    CHECK(err_n == err_ref && err_i == err_ref, "%s: status %d on the pixel path, %d NV12, %d I420", what, err_ref, err_n,
          err_i);
    for (int p = 0; p < 2; p++) CHECK(nv[p].padding_intact(), "%s: NV12 plane %d: padding written", what, p);
    for (int p = 0; p < 3; p++) CHECK(iy[p].padding_intact(), "%s: I420 plane %d: padding written", what, p);
    int bad = 0;
    for (int y = 0; y < g.H; y++)
        for (int x = 0; x < g.W; x++) {
            const uint8_t want = comp[(size_t)y * g.yp + x];
            bad += nv[0].p[(size_t)y * nv[0].pitch + x] != want || iy[0].p[(size_t)y * iy[0].pitch + x] != want;
        }
    for (int c = 1; c <= 2; c++)
        for (int y = 0; y < g.H / 2; y++)
            for (int x = 0; x < g.W / 2; x++) {
                const uint8_t want = comp[jdec_plane_off(g, c) + (size_t)y * g.cp + x];
                bad += nv[1].p[(size_t)y * nv[1].pitch + 2 * x + c - 1] != want ||
                       iy[c].p[(size_t)y * iy[c].pitch + x] != want;
            }
    CHECK(bad == 0, "%s: %d samples differ from the pixel path's component planes", what, bad);
    if (good) CHECK(err_ref == 0, "%s: a good file ended with status %d", what, err_ref);
    for (Plane& p : nv) free(p.p);
    for (Plane& p : iy) free(p.p);
    free(comp);
    if (status_out) *status_out = err_ref ? EVAM_PP_ERR_INVALID_ARG : 0;
    return 1;
}

std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> v;
    FILE* fp = fopen(path, "rb");
    if (!fp) { printf("cannot open %s\n", path); exit(2); }
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), fp)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(fp);
    return v;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

}  // namespace

int main(int argc, char** argv) {
    bool damaged = false;
    std::vector<std::vector<uint8_t>> good;
    int n_files = 0, n_skipped = 0;
    bool sizes[3] = {false, false, false};  // 2x2, 10x10, 24x8 among the good files
    for (int i = 1; i < argc; i++) {
        if (std::string(argv[i]) == "--damaged") { damaged = true; continue; }
        const std::vector<uint8_t> file = read_file(argv[i]);
        int status = 0;
        n_files++;
        if (!check_file(file, argv[i], !damaged, &status)) { n_skipped++; continue; }
        printf("%s: status %d\n", argv[i], status);
        if (!damaged) {
            good.push_back(file);
            evam_jpeg_info info{};
            char msg[320];
            jdec_parse(file.data(), file.size(), &info, nullptr, msg, sizeof(msg));
            sizes[0] |= info.width == 2 && info.height == 2;
            sizes[1] |= info.width == 10 && info.height == 10;
            sizes[2] |= info.width == 24 && info.height == 8;
        }
    }
    CHECK(sizes[0] && sizes[1] && sizes[2], "the good files must include the sizes 2x2, 10x10 and 24x8");
    int n_random = 0, n_random_bad = 0;
    if (!good.empty()) {
        for (int it = 0; it < 5000; it++) {
            std::vector<uint8_t> f = good[rnd() % good.size()];
            evam_jpeg_info info{};
            char msg[320];
            if (jdec_parse(f.data(), f.size(), &info, nullptr, msg, sizeof(msg))) continue;
            const size_t s0 = info.scan_offset, n = f.size() - s0;
            if (n == 0) continue;
            const int kind = (int)(rnd() % 6);
            const int times = 1 + (int)(rnd() % 8);
            for (int t = 0; t < times; t++) {
                const size_t at = s0 + rnd() % n;
                if (kind == 0) f[at] ^= (uint8_t)(1u << (rnd() % 8));
                else if (kind == 1) f[at] = (uint8_t)rnd();
                else if (kind == 2) f[at] = 0xFF;
                else if (kind == 3) f[at] = 0x00;
                else if (kind == 4 && at + 1 < f.size()) { f[at] = 0xFF; f[at + 1] = (uint8_t)(0xD0 + rnd() % 8); }
            }
            if (kind == 5) f.resize(s0 + rnd() % n);
            int status = 0;
            if (!check_file(f, "random damaged scan", false, &status)) continue;
            n_random++;
            n_random_bad += status != 0;
        }
    }
    printf("%d files (%d skipped), %d random damaged scans (%d with a non-zero status)\n", n_files, n_skipped, n_random,
           n_random_bad);
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("all checks passed\n");
    return 0;
}
