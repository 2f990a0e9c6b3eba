// Baseline JPEG encoder of the published BGR frame (evam_pp_encode_jpeg): tables and kernels.
// Included by evam_pp.hip inside its anonymous namespace, before struct evam_pp. The arithmetic is libjpeg's
// (baseline, 4:2:0, JDCT_ISLOW, Annex K tables, no restart interval): include/evam_pp.h states the contract,
// DESIGN.md §4.5 the decomposition.
//
// Stages, all on the handle's stream, per call:
//   jpeg_coef    one wave per MCU: BGR -> YCbCr, 2x2 chroma down-sample, 8x8 DCT, quantisation; writes zig-zag
//                int16 coefficients and per block (AC bit count << 16 | DC)
//   jpeg_scan1   per group of kJpegGroup blocks: block bit counts (DC difference + AC), exclusive scan in the group
//   jpeg_scan2   one workgroup per frame: exclusive scan of the group totals; zeroes the words groups share
//   jpeg_pack    per group: every thread Huffman-codes its block into LDS at its bit offset; whole words leave with
//                plain stores, the (at most two) words a group shares with a neighbour with one atomicOr each
//   jpeg_finish  one workgroup per frame: header, byte stuffing, 1-padding, EOI, sizes[i]
#pragma once

constexpr int kJpegHeaderLen = 623;
constexpr int kJpegGroup = 128;          // blocks per scan / pack workgroup (one block per thread)
constexpr int kJpegBlockBits = 1660;     // DC 11 + 11, AC 63 x (16 + 10)
constexpr int kJpegPackWords = kJpegGroup * kJpegBlockBits / 32 + 2;  // a group's worst case, plus a shared word each side
constexpr int kJpegFinishThreads = 512;

struct JpegTables {           // device copy, rebuilt when (width, height, quality) change
    uint8_t header[640];      // kJpegHeaderLen bytes used
    uint16_t qv[2][64];       // 8 * Q in zig-zag order: luminance, chrominance
    uint32_t dc[2][16];       // category -> code | length << 16
    uint32_t ac[2][256];      // run << 4 | size -> code | length << 16
};

// ---- Annex K ----
const uint8_t kJpegZigzag[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63};
__constant__ uint8_t kJpegZigzagDev[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63};
const uint8_t kJpegQLuma[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
    51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
    101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kJpegQChroma[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kJpegDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
     0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
     0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
     0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
     0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
     0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
     0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
     0xF9, 0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
     0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
     0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
     0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
     0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
     0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
     0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
     0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
     0xF9, 0xFA}};

inline int jpeg_quality_scale(int quality) {  // jpeg_quality_scaling
    const int q = quality <= 0 ? 1 : (quality > 100 ? 100 : quality);
    return q < 50 ? 5000 / q : 200 - 2 * q;
}

inline void jpeg_quant_table(const uint8_t* base, int quality, uint8_t* out /* natural order */) {
    const int scale = jpeg_quality_scale(quality);
    for (int i = 0; i < 64; i++) {
        const int v = (base[i] * scale + 50) / 100;
        out[i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

// code | length << 16 per symbol of a table given as counts and symbols
inline void jpeg_huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = code++ | (uint32_t)len << 16;
        code <<= 1;
    }
}

// The header every frame of one (width, height, quality) starts with, and the device tables that go with it.
inline void jpeg_build_tables(int width, int height, int quality, JpegTables& t) {
    memset(&t, 0, sizeof(t));
    uint8_t q[2][64];
    jpeg_quant_table(kJpegQLuma, quality, q[0]);
    jpeg_quant_table(kJpegQChroma, quality, q[1]);
    uint8_t* p = t.header;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00});
    for (int i = 0; i < 2; i++) {
        put({0xFF, 0xDB, 0x00, 0x43, i});
        for (int k = 0; k < 64; k++) {
            *p++ = q[i][kJpegZigzag[k]];
            t.qv[i][k] = (uint16_t)(8 * q[i][kJpegZigzag[k]]);
        }
    }
    put({0xFF, 0xC0, 0x00, 0x11, 0x08, height >> 8, height & 255, width >> 8, width & 255, 0x03, 0x01, 0x22, 0x00,
         0x02, 0x11, 0x01, 0x03, 0x11, 0x01});
    for (int i = 0; i < 4; i++) {  // DC0, AC0, DC1, AC1
        const int tbl = i >> 1, ac = i & 1;
        const uint8_t* bits = ac ? kJpegAcBits[tbl] : kJpegDcBits[tbl];
        const uint8_t* vals = ac ? kJpegAcVals[tbl] : kJpegDcVals;
        const int nv = ac ? 162 : 12, len = 2 + 1 + 16 + nv;
        put({0xFF, 0xC4, len >> 8, len & 255, ac << 4 | tbl});
        for (int k = 0; k < 16; k++) *p++ = bits[k];
        for (int k = 0; k < nv; k++) *p++ = vals[k];
        jpeg_huff_codes(bits, vals, ac ? t.ac[tbl] : t.dc[tbl]);
    }
    put({0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00});
}

struct JpegGeom {
    int W, H;          // frame
    int mx, my;        // MCUs across / down
    int n_mcu, n_blk;  // per frame
    int n_grp;         // scan / pack groups per frame
    int yb_x, yb_y;    // real Y blocks across / down: ceil(W/8), ceil(H/8)
    int cq_y;          // real chroma rows: ceil(H/2)
};

struct JpegParams {
    JpegGeom g;
    const uint8_t* bgr;       // [n][H][W][3]
    const JpegTables* tab;
    int16_t* coef;            // [n][n_blk][64] zig-zag
    uint32_t* meta;           // [n][n_blk]  AC bits << 16 | (uint16)DC
    uint32_t* off;            // [n][n_blk]  block's bit offset inside its group
    uint32_t* gsum;           // [n][n_grp]  group totals, then (jpeg_scan2) the groups' exclusive bit offsets
    uint32_t* total;          // [n]         bits of the frame's scan
    uint32_t* stream;         // [n][stream_words] unstuffed scan, bit 31 of a word first
    uint32_t stream_words;    // per frame, a multiple of 4
    uint8_t* dst;
    size_t dst_stride;
    uint32_t* sizes;
};

__device__ __forceinline__ int jpeg_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Exclusive scan of one value per thread over a workgroup of NT threads (a multiple of 64). sh: NT / 64 + 1 words.
template <int NT>
__device__ __forceinline__ uint32_t jpeg_block_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();  // sh may still be read from the previous use
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const uint32_t s = sh[w];
        if (w < wave) base += s;
        sum += s;
    }
    total = sum;
    return base + inc - v;
}

// One pass of jfdctint.c over eight values. FIRST: rows (results scaled up by PASS1_BITS); else columns.
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int* d) {
    constexpr int CB = 13, P1 = 2;
    constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                  F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    constexpr int N = FIRST ? CB - P1 : CB + P1;
    auto desc = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * (1 << P1);
        d[4] = (t10 - t11) * (1 << P1);
    } else {
        d[0] = desc(t10 + t11, P1);
        d[4] = desc(t10 - t11, P1);
    }
    int z1 = (t12 + t13) * F0541;
    d[2] = desc(z1 + t13 * F0765, N);
    d[6] = desc(z1 - t12 * F1847, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1175;
    t4 *= F0298; t5 *= F2053; t6 *= F3072; t7 *= F1501;
    z1 *= -F0899; z2 *= -F2562;
    z3 = z3 * -F1961 + z5;
    z4 = z4 * -F0390 + z5;
    d[7] = desc(t4 + z1 + z3, N);
    d[5] = desc(t5 + z2 + z4, N);
    d[3] = desc(t6 + z2 + z3, N);
    d[1] = desc(t7 + z1 + z4, N);
}

// grid (ceil(n_mcu / 4), frames), 256 threads: wave w of a workgroup owns MCU blockIdx.x * 4 + w.
__global__ __launch_bounds__(256) void evam_jpeg_coef(const JpegParams P) {
    __shared__ int s_all[4][6][64];
    const JpegGeom& g = P.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mcu = blockIdx.x * 4 + wave, frame = blockIdx.y;
    const bool live = mcu < g.n_mcu;  // a dead wave keeps the barriers and touches no memory
    int (*s)[64] = s_all[wave];
    const int my = live ? mcu / g.mx : 0, mxi = live ? mcu - my * g.mx : 0;
    if (live) {
        // colour conversion of this lane's 2x2 quad; edges replicate as libjpeg pads them (evam_pp.h)
        const uint8_t* img = P.bgr + (size_t)frame * g.H * g.W * 3;
        const int qx = lane & 7, qy = lane >> 3;
        const int x0 = mxi * 16 + qx * 2, y0 = my * 16 + qy * 2;
        const int xa = min(x0, g.W - 1), xb = min(x0 + 1, g.W - 1);
        const int ya = min(y0, g.H - 1), yb = min(y0 + 1, g.H - 1);
        // chroma rows: the last real down-sampled row repeats, not the last source row
        const int cy = min(my * 8 + qy, g.cq_y - 1);
        const int ca = cy * 2, cb_ = min(cy * 2 + 1, g.H - 1);
        int cbs = 0, crs = 0;
        auto px = [&](int y, int x, int& Y, int& Cb, int& Cr) {
            const uint8_t* p = img + ((size_t)y * g.W + x) * 3;
            const int B = p[0], G = p[1], R = p[2];
            Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        };
        const int ys[2] = {ya, yb}, xs[2] = {xa, xb}, cs[2] = {ca, cb_};
        const bool same_rows = ca == ya && cb_ == yb;
        const int blk = (qy >> 2) * 2 + (qx >> 2);
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                int Y, Cb, Cr;
                px(ys[dy], xs[dx], Y, Cb, Cr);
                s[blk][((qy & 3) * 2 + dy) * 8 + (qx & 3) * 2 + dx] = Y - 128;
                if (!same_rows) { int Y2; px(cs[dy], xs[dx], Y2, Cb, Cr); }
                cbs += Cb;
                crs += Cr;
            }
        const int bias = 1 + (qx & 1);
        s[4][qy * 8 + qx] = ((cbs + bias) >> 2) - 128;
        s[5][qy * 8 + qx] = ((crs + bias) >> 2) - 128;
    }
    __syncthreads();
    if (live && lane < 48) {  // rows
        int* r = &s[lane >> 3][(lane & 7) * 8];
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = r[i];
        jpeg_fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; i++) r[i] = d[i];
    }
    __syncthreads();
    if (live && lane < 48) {  // columns
        int* c = &s[lane >> 3][lane & 7];
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; i++) d[i] = c[i * 8];
        jpeg_fdct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; i++) c[i * 8] = d[i];
    }
    __syncthreads();
    if (!live) return;
    // lane k quantises zig-zag coefficient k of all six blocks
    int q[6];
    const int nat = kJpegZigzagDev[lane];
#pragma unroll
    for (int b = 0; b < 6; b++) {
        const int c = s[b][nat];
        const int qv = P.tab->qv[b >> 2][lane];
        const int a = (abs(c) + (qv >> 1)) / qv;
        q[b] = c < 0 ? -a : a;
    }
    // dummy Y blocks (beyond the real block columns / rows): AC zero, DC of the block before in the MCU
    bool dummy[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        dummy[b] = mxi * 2 + (b & 1) >= g.yb_x || my * 2 + (b >> 1) >= g.yb_y;
        if (dummy[b]) q[b] = lane == 0 ? q[b - (b > 0)] : 0;  // lane 0 holds every DC; b = 0 is never a dummy
    }
    const size_t blk0 = ((size_t)frame * g.n_mcu + mcu) * 6;
#pragma unroll
    for (int b = 0; b < 6; b++) {
        P.coef[(blk0 + b) * 64 + lane] = (int16_t)q[b];
        // AC bits: every non-zero lane prices its own run/size code, the wave adds them up
        const uint32_t* ac = P.tab->ac[b >> 2];
        const bool nz = lane > 0 && q[b] != 0;
        const unsigned long long mask = __ballot(nz);
        int bits = 0;
        if (nz) {
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            const int prev = below ? 63 - __clzll(below) : 0;
            const int run = lane - prev - 1;
            const int size = 32 - __clz(abs(q[b]));
            bits = (run >> 4) * (int)(ac[0xF0] >> 16) + (int)(ac[(run & 15) << 4 | size] >> 16) + size;
        }
        bits = jpeg_wave_sum(bits);
        if (!(mask >> 63)) bits += (int)(ac[0] >> 16);  // EOB
        if (lane == 0) P.meta[blk0 + b] = (uint32_t)bits << 16 | (uint32_t)(uint16_t)(int16_t)q[b];
    }
}

// The DC a block's difference is taken from: the block of the same component before it in the scan.
__device__ __forceinline__ int jpeg_pred_dc(const uint32_t* meta /* frame */, int i) {
    const int j = i % 6;
    int p;
    if (j >= 1 && j <= 3) p = i - 1;
    else if (i < 6) return 0;
    else p = j == 0 ? i - 3 : i - 6;
    return (int16_t)(meta[p] & 0xFFFF);
}

// grid (n_grp, frames), kJpegGroup threads: one block per thread.
__global__ __launch_bounds__(kJpegGroup) void evam_jpeg_scan1(const JpegParams P) {
    __shared__ uint32_t sh[kJpegGroup / 64 + 1];
    const JpegGeom& g = P.g;
    const int frame = blockIdx.y, i = blockIdx.x * kJpegGroup + threadIdx.x;
    const uint32_t* meta = P.meta + (size_t)frame * g.n_blk;
    uint32_t bits = 0;
    if (i < g.n_blk) {
        const uint32_t m = meta[i];
        const int diff = (int16_t)(m & 0xFFFF) - jpeg_pred_dc(meta, i);
        const int cat = 32 - __clz(abs(diff));
        bits = (m >> 16) + (P.tab->dc[(i % 6) >= 4][cat] >> 16) + cat;
    }
    uint32_t total;
    const uint32_t ex = jpeg_block_scan<kJpegGroup>(bits, sh, total);
    if (i < g.n_blk) P.off[(size_t)frame * g.n_blk + i] = ex;
    if (threadIdx.x == 0) P.gsum[(size_t)frame * g.n_grp + blockIdx.x] = total;
}

// grid (frames), 256 threads: group totals -> exclusive offsets; the stream words two groups share start at zero.
__global__ __launch_bounds__(256) void evam_jpeg_scan2(const JpegParams P) {
    __shared__ uint32_t sh[256 / 64 + 1];
    const JpegGeom& g = P.g;
    const int frame = blockIdx.x;
    uint32_t* gs = P.gsum + (size_t)frame * g.n_grp;
    uint32_t* stream = P.stream + (size_t)frame * P.stream_words;
    uint32_t carry = 0;
    for (int base = 0; base < g.n_grp; base += 256) {
        const int k = base + threadIdx.x;
        const uint32_t v = k < g.n_grp ? gs[k] : 0;
        uint32_t total;
        const uint32_t ex = carry + jpeg_block_scan<256>(v, sh, total);
        if (k < g.n_grp) {
            gs[k] = ex;
            stream[ex >> 5] = 0;
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        P.total[frame] = carry;
        stream[carry >> 5] = 0;  // the last group's last word; stream_words covers it
    }
}

// grid (n_grp, frames), kJpegGroup threads: one block per thread, packed in LDS from the group's first word on.
__global__ __launch_bounds__(kJpegGroup) void evam_jpeg_pack(const JpegParams P) {
    __shared__ uint32_t win[kJpegPackWords];
    __shared__ uint32_t s_ac[2][256];
    __shared__ uint32_t s_dc[2][16];
    const JpegGeom& g = P.g;
    const int frame = blockIdx.y, grp = blockIdx.x, tid = threadIdx.x;
    const int i = grp * kJpegGroup + tid;
    const uint32_t g0 = P.gsum[(size_t)frame * g.n_grp + grp];
    const uint32_t g1 = grp + 1 < g.n_grp ? P.gsum[(size_t)frame * g.n_grp + grp + 1] : P.total[frame];
    const uint32_t w0 = g0 >> 5;
    const uint32_t n_words = g1 > g0 ? ((g1 - 1) >> 5) - w0 + 1 : 0;  // <= kJpegPackWords by the per-block bound
    for (uint32_t w = tid; w < n_words; w += kJpegGroup) win[w] = 0;
    for (int k = tid; k < 512; k += kJpegGroup) (&s_ac[0][0])[k] = (&P.tab->ac[0][0])[k];
    if (tid < 32) (&s_dc[0][0])[tid] = (&P.tab->dc[0][0])[tid];
    __syncthreads();
    if (i < g.n_blk) {
        const uint32_t* meta = P.meta + (size_t)frame * g.n_blk;
        const uint32_t pos = g0 - (w0 << 5) + P.off[(size_t)frame * g.n_blk + i];  // bit offset inside win
        uint32_t widx = pos >> 5;
        int nacc = (int)(pos & 31);  // bits held in acc, the first nacc of them another block's (zero here)
        unsigned long long acc = 0;
        auto emit = [&](uint32_t code, int len) {  // len <= 27
            acc = acc << len | code;
            nacc += len;
            if (nacc >= 32) {
                nacc -= 32;
                atomicOr(&win[widx++], (uint32_t)(acc >> nacc));
            }
        };
        const int tbl = (i % 6) >= 4;
        const uint4* cp = reinterpret_cast<const uint4*>(P.coef + ((size_t)frame * g.n_blk + i) * 64);
        const uint32_t* ac = s_ac[tbl];
        const uint32_t zrl = ac[0xF0];
        int run = 0;
        for (int v4 = 0; v4 < 8; v4++) {
            const uint4 u = cp[v4];
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 8; e++) {
                int c = (int16_t)(w[e >> 1] >> ((e & 1) * 16));
                if (v4 == 0 && e == 0) {
                    c -= jpeg_pred_dc(meta, i);
                    const int cat = 32 - __clz(abs(c));
                    const uint32_t h = s_dc[tbl][cat];
                    const uint32_t vb = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << cat) - 1u);
                    emit((h & 0xFFFF) << cat | vb, (int)(h >> 16) + cat);
                    continue;
                }
                if (c == 0) { run++; continue; }
                while (run > 15) { emit(zrl & 0xFFFF, (int)(zrl >> 16)); run -= 16; }
                const int size = 32 - __clz(abs(c));
                const uint32_t h = ac[run << 4 | size];
                const uint32_t vb = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1u);
                emit((h & 0xFFFF) << size | vb, (int)(h >> 16) + size);
                run = 0;
            }
        }
        if (run) emit(ac[0] & 0xFFFF, (int)(ac[0] >> 16));
        if (nacc) atomicOr(&win[widx], (uint32_t)(acc << (32 - nacc)));
    }
    __syncthreads();
    // a word wholly inside [g0, g1) is this group's alone; the first and the last may be shared with a neighbour
    uint32_t* stream = P.stream + (size_t)frame * P.stream_words;
    for (uint32_t w = tid; w < n_words; w += kJpegGroup) {
        const uint64_t b0 = (uint64_t)(w0 + w) << 5;
        if (b0 >= g0 && b0 + 32 <= g1) stream[w0 + w] = win[w];
        else atomicOr(&stream[w0 + w], win[w]);
    }
}

// grid (frames), kJpegFinishThreads threads: header, stuffed scan, EOI, sizes[frame]. Nothing is written at or
// beyond dst_stride.
__global__ __launch_bounds__(kJpegFinishThreads) void evam_jpeg_finish(const JpegParams P) {
    __shared__ uint32_t sh[kJpegFinishThreads / 64 + 1];
    const int frame = blockIdx.x, tid = threadIdx.x;
    uint8_t* out = P.dst + (size_t)frame * P.dst_stride;
    const size_t cap = P.dst_stride;
    for (int k = tid; k < kJpegHeaderLen; k += kJpegFinishThreads)
        if ((size_t)k < cap) out[k] = P.tab->header[k];
    const uint32_t total = P.total[frame];
    const uint32_t n_bytes = (total + 7) >> 3;
    const uint32_t pad = (8 - (total & 7)) & 7;  // 1-bits that fill the last byte
    const uint4* stream = reinterpret_cast<const uint4*>(P.stream + (size_t)frame * P.stream_words);
    size_t pos = kJpegHeaderLen;  // the same in every thread
    for (uint32_t base = 0; base < n_bytes; base += kJpegFinishThreads * 16) {
        const uint32_t b0 = base + tid * 16;
        uint32_t w[4] = {0, 0, 0, 0};
        uint32_t n = 0, nff = 0;
        if (b0 < n_bytes) {
            const uint4 u = stream[b0 >> 4];
            w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
            n = min(16u, n_bytes - b0);
            if (pad && b0 + n == n_bytes) w[(n - 1) >> 2] |= ((1u << pad) - 1u) << (24 - 8 * ((n - 1) & 3));
            for (uint32_t k = 0; k < n; k++) nff += ((w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFF) == 0xFF;
        }
        uint32_t chunk;
        size_t o = pos + jpeg_block_scan<kJpegFinishThreads>(n + nff, sh, chunk);
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t b = (w[k >> 2] >> (24 - 8 * (k & 3))) & 0xFF;
            if (o < cap) out[o] = (uint8_t)b;
            o++;
            if (b == 0xFF) {
                if (o < cap) out[o] = 0;
                o++;
            }
        }
        pos += chunk;
    }
    if (tid == 0) {
        if (pos < cap) out[pos] = 0xFF;
        if (pos + 1 < cap) out[pos + 1] = 0xD9;
        P.sizes[frame] = (uint32_t)(pos + 2);
    }
}

// Handle-owned device scratch of the encoder: grows on demand, reused across calls.
struct JpegScratch {
    void* buf[8] = {};
    size_t cap[8] = {};
    int key[3] = {0, 0, -1};  // (width, height, quality) the device tables were built for
};
enum { kJsBgr, kJsTab, kJsCoef, kJsMeta, kJsOff, kJsGsum, kJsTotal, kJsStream };
