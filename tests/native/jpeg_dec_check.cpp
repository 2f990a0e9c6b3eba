// Stand-alone check of csrc/evam_jpeg_dec.h, the arithmetic the JPEG decoder's kernels and its host twin share, built
// with -fsanitize=address,undefined (tests/test_native_asan_jpeg_dec.py). Every file named on the command line is
// parsed and decoded twice: sequentially, as evam_pp_decode_jpeg_host drives jdec_run, and by sub-sequences, driven
// exactly as the kernels drive it: kJdecChunk sub-sequences of kJdecSubBits bits at a time, rounds until no exit
// state changes, a carry between chunks, records in a slot table, then the write pass from the final entry states.
// Both must end with the same status and the same coefficients, inside exactly-sized heap buffers, within the round
// bound. The same is asked with 64-bit sub-sequences in chunks of 4 (so that small files cross chunk borders) and of
// 20,000 seeded random damaged scans derived from the good files.
//   usage: jpeg_dec_check file... [--good-only file...] [--damaged file...] [--expect-bad file...]
//   Files in front of the flags must decode with status 0 (or be refused by the parse) and seed the random scans;
//   after --good-only they must decode with status 0 and seed nothing (files too long to damage 20,000 times);
//   after --damaged any status is accepted, after --expect-bad only a non-zero one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../edge-video-analytics-microservice_amd/csrc/evam_jpeg_dec.h"

namespace {

int g_fail = 0;
int g_max_rounds = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

struct Result {
    int rc = 0;      // header parse
    int status = 0;  // scan
    std::vector<int16_t> coef;
    std::vector<uint8_t> pixels;
};

void interval_blocks(const JdecGeom& g, uint32_t k, uint32_t& blk0, uint32_t& limit) {
    const uint32_t m0 = g.ri > 0 ? k * (uint32_t)g.ri : 0u;
    uint32_t m1 = g.ri > 0 ? m0 + (uint32_t)g.ri : (uint32_t)g.n_mcu;
    if (m1 > (uint32_t)g.n_mcu) m1 = (uint32_t)g.n_mcu;
    blk0 = m0 * g.bpm; limit = m1 * g.bpm;
}

// sub_bits == 0: sequential. Otherwise sub-sequences of sub_bits bits in chunks of `chunk`.
Result decode(const std::vector<uint8_t>& file, uint32_t sub_bits, uint32_t chunk, int bpp) {
    Result R;
    evam_jpeg_info info{};
    JdecFile* f = new JdecFile;
    char msg[320];
    R.rc = jdec_parse(file.data(), file.size(), &info, f, msg, sizeof(msg));
    JdecGeom g;
    if (R.rc || !jdec_geom(info, g)) { delete f; return R; }
    int err = 0;
    uint8_t* stream = (uint8_t*)malloc((size_t)f->scan_len + kJdecStreamPad);
    uint32_t* first = (uint32_t*)malloc(((size_t)g.n_int + 1) * sizeof(uint32_t));
    err |= jdec_unstuff_host(file.data() + (file.size() - f->scan_len), f->scan_len, g.n_int, stream, first) != 0;
    R.coef.assign((size_t)g.n_blk * 64, 0);
    JdecScan sc{stream, f, g.nluma, g.bpm};
    if (sub_bits == 0) {
        for (uint32_t k = 0; k < (uint32_t)g.n_int; k++) {
            uint32_t blk0, limit, p = first[k] * 8, bz = 0;
            interval_blocks(g, k, blk0, limit);
            const uint32_t end = first[k + 1] * 8;
            const uint32_t done = jdec_run(sc, p, bz, end, end, R.coef.data(), blk0, limit, err);
            if (blk0 + done < limit) err = 1;
        }
    } else {
        const uint32_t sub_bytes = sub_bits / 8;
        const size_t n_slots = (size_t)f->scan_len / sub_bytes + (size_t)g.n_int + 1;
        struct Slot { uint32_t p, bz, blk, iv; };
        Slot* slots = (Slot*)calloc(n_slots, sizeof(Slot));
        std::vector<uint32_t> ep(chunk), ebz(chunk), xp(chunk), xbz(chunk), cnt(chunk), sp(chunk), sbz(chunk);
        // kernel 2
        for (uint32_t k = 0; k < (uint32_t)g.n_int; k++) {
            const uint32_t fb = first[k], fe = first[k + 1] >= fb ? first[k + 1] : fb;
            const uint32_t P0 = fb * 8, end = fe * 8, nsub = (fe - fb + sub_bytes - 1) / sub_bytes;
            const uint32_t slot0 = fb / sub_bytes + k;
            uint32_t blk0, limit;
            interval_blocks(g, k, blk0, limit);
            uint32_t carry_p = P0, carry_bz = 0, carry_blk = blk0;
            int unused = 0;
            for (uint32_t c0 = 0; c0 < nsub; c0 += chunk) {
                const uint32_t act = nsub - c0 < chunk ? nsub - c0 : chunk;
                for (uint32_t t = 0; t < act; t++) {
                    const uint32_t start = P0 + (c0 + t) * sub_bits;
                    ep[t] = t == 0 ? carry_p : start; ebz[t] = t == 0 ? carry_bz : 0;
                    xp[t] = ep[t]; xbz[t] = ebz[t];
                    cnt[t] = jdec_run(sc, xp[t], xbz[t], start + sub_bits, end, nullptr, 0, 0, unused);
                }
                int rounds = 1;
                for (uint32_t r = 1; r < chunk; r++) {
                    sp = xp; sbz = xbz;  // what the threads read before any of them writes
                    bool changed = false;
                    for (uint32_t t = 1; t < act; t++) {
                        if (sp[t - 1] == ep[t] && sbz[t - 1] == ebz[t]) continue;
                        ep[t] = sp[t - 1]; ebz[t] = sbz[t - 1];
                        uint32_t np = ep[t], nbz = ebz[t];
                        cnt[t] = jdec_run(sc, np, nbz, P0 + (c0 + t + 1) * sub_bits, end, nullptr, 0, 0, unused);
                        if (np != xp[t] || nbz != xbz[t]) { xp[t] = np; xbz[t] = nbz; changed = true; }
                    }
                    rounds++;
                    if (!changed) break;
                }
                if (rounds > g_max_rounds) g_max_rounds = rounds;
                for (uint32_t t = 1; t < act; t++)  // converged: every entry is its predecessor's exit
                    CHECK(ep[t] == xp[t - 1] && ebz[t] == xbz[t - 1], "chunk not converged within %u rounds", chunk);
                for (uint32_t t = 0; t < act; t++) {
                    const size_t slot = (size_t)slot0 + c0 + t;
                    CHECK(slot < n_slots, "slot %zu of %zu", slot, n_slots);
                    if (slot < n_slots) slots[slot] = Slot{ep[t], ebz[t], carry_blk, k + 1};
                    carry_blk += cnt[t];
                }
                carry_p = xp[act - 1]; carry_bz = xbz[act - 1];
            }
            if (carry_blk < limit) err = 1;
        }
        // kernel 3
        for (size_t slot = 0; slot < n_slots; slot++) {
            const Slot s = slots[slot];
            if (s.iv == 0) continue;
            const uint32_t k = s.iv - 1, fb = first[k], fe = first[k + 1] >= fb ? first[k + 1] : fb;
            const uint32_t i = (uint32_t)slot - (fb / sub_bytes + k);
            uint32_t blk0, limit, p = s.p, bz = s.bz;
            interval_blocks(g, k, blk0, limit);
            jdec_run(sc, p, bz, fb * 8 + (i + 1) * sub_bits, fe * 8, R.coef.data(), s.blk, limit, err);
        }
        free(slots);
    }
    std::vector<int16_t> coef = R.coef;  // the DC pass works in place: keep the raw differences for the comparison
    uint8_t* planes = (uint8_t*)malloc(g.plane_bytes);
    jdec_dc_and_idct_host(g, *f, coef.data(), planes, err);
    R.pixels.assign((size_t)g.W * g.H * bpp, 0);
    jdec_colour_host(g, planes, R.pixels.data(), g.W * bpp, bpp);
    R.status = err ? EVAM_PP_ERR_INVALID_ARG : 0;
    free(planes); free(first); free(stream);
    delete f;
    return R;
}

// 0: refused by the parse; 1: decoded. All drivings must agree.
int check_file(const std::vector<uint8_t>& file, const char* what, int* status_out) {
    const Result a = decode(file, 0, 0, 3);
    if (a.rc) { if (status_out) *status_out = a.rc; return 0; }
    const Result b = decode(file, kJdecSubBits, kJdecChunk, 4);
    const Result c = decode(file, 64, 4, 3);
    CHECK(a.status == b.status && a.status == c.status, "%s: status %d sequential, %d in sub-sequences, %d in small ones",
          what, a.status, b.status, c.status);
    CHECK(a.coef == b.coef && a.coef == c.coef, "%s: coefficients differ between the drivings", what);
    CHECK(a.pixels == c.pixels, "%s: pixels differ between the drivings", what);
    if (status_out) *status_out = a.status;
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
    int mode = 0;  // 0 good, 1 damaged, 2 expected bad
    std::vector<std::vector<uint8_t>> good;
    int n_files = 0, n_refused = 0;
    for (int i = 1; i < argc; i++) {
        if (std::string(argv[i]) == "--damaged") { mode = 1; continue; }
        if (std::string(argv[i]) == "--expect-bad") { mode = 2; continue; }
        if (std::string(argv[i]) == "--good-only") { mode = 3; continue; }
        const std::vector<uint8_t> file = read_file(argv[i]);
        int status = 0;
        n_files++;
        if (!check_file(file, argv[i], &status)) { n_refused++; printf("%s: refused (%d)\n", argv[i], status); continue; }
        printf("%s: status %d\n", argv[i], status);
        if (mode == 2) CHECK(status != 0, "%s: a damaged scan ended with status 0", argv[i]);
        else if (mode == 0 || mode == 3) {
            CHECK(status == 0, "%s: a good file ended with status %d", argv[i], status);
            if (mode == 0) good.push_back(file);
        }
    }
    int n_random = 0, n_random_bad = 0;
    if (!good.empty()) {
        for (int it = 0; it < 20000; it++) {
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
            check_file(f, "random damaged scan", &status);
            n_random++;
            n_random_bad += status != 0;
        }
    }
    printf("%d files (%d refused), %d random damaged scans (%d with a non-zero status), at most %d rounds per chunk\n",
           n_files, n_refused, n_random, n_random_bad, g_max_rounds);
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("all checks passed\n");
    return 0;
}
