// evam_jpeg_dec.h - the arithmetic of the baseline JPEG decoder, shared by the kernels (evam_jpeg_dec_kernels.h), by
// evam_pp_decode_jpeg_host and by tests/native/jpeg_dec_check.cpp. Everything here is plain C++: EVAM_HD marks what
// the kernels call too (evam_pp.hip defines it as __host__ __device__ before including this file).
//
// The pixels are those of libjpeg's default decode (JDCT_ISLOW, fancy up-sampling, integer YCbCr -> RGB); the stored
// Pillow decodes under tests/golden/jpeg_dec/ are the arbiter. Every loop below that depends on file data carries a
// trip bound derived from a length the header parse validated, and every index is masked or checked against its
// buffer: any byte sequence whatsoever ends with a status.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/evam_pp.h"

#ifndef EVAM_HD
#define EVAM_HD
#endif

constexpr int kJdecLook = 9;                       // bits of the Huffman look-ahead table; longer codes walk maxcode
constexpr int kJdecSubBits = 1024;                 // S: bits of one sub-sequence (one thread)
constexpr int kJdecSubBytes = kJdecSubBits / 8;
constexpr int kJdecChunk = 1024;                   // T: sub-sequences a workgroup synchronises at a time
constexpr int kJdecMaxSymBits = 16 + 15;           // a code plus its extra bits: what one step can consume at most
constexpr uint32_t kJdecMaxLen = 1u << 28;         // file length limit (bit positions stay below 2^31)
constexpr int kJdecStreamPad = 16;                 // zero bytes behind a file's compacted scan (the 64-bit peek)

// One Huffman table: codes of up to kJdecLook bits resolve through look (length << 8 | symbol, 0 = longer or none),
// the rest through the Annex F walk: the first length l with code <= maxcode[l] gives vals[valoff[l] + code].
struct JdecHuff {
    uint16_t look[1 << kJdecLook];
    int32_t maxcode[17];  // [1..16]; -1 where a length has no code
    int32_t valoff[17];   // index of the length's first symbol minus its first code
    uint8_t vals[256];
};

// What the scan of one file needs: its tables, resolved per component. huff[0..1] are DC, huff[2..3] AC.
struct JdecFile {
    JdecHuff huff[4];
    uint8_t q[3][64];     // per component, in zig-zag order as the file stores it
    uint8_t dc_tab[3];    // per component: index into huff (0..1)
    uint8_t ac_tab[3];    // per component: index into huff (2..3)
    uint8_t pad[2];
    uint32_t scan_len;    // bytes from the first entropy-coded byte to the end of the file
    uint32_t raw_off;     // where those bytes start inside the call's raw buffer
};

// The geometry the files of one call share.
struct JdecGeom {
    int32_t W, H, ncomp, hs, vs, ri;
    int32_t mx, my, n_mcu;   // MCU columns, rows, count
    int32_t nluma, bpm;      // luma blocks per MCU, blocks per MCU
    int32_t n_blk, n_int;    // blocks of the scan, restart intervals
    int32_t cw, ch;          // real chroma size: ceil(W / hs), ceil(H / vs)
    int32_t yp, yrows;       // luma plane: pitch and rows, whole MCUs
    int32_t cp, crows;       // chroma planes
    uint32_t plane_bytes;    // all planes of one file
};

EVAM_HD inline bool jdec_geom(const evam_jpeg_info& in, JdecGeom& g) {
    if (in.width <= 0 || in.height <= 0 || in.width > 32768 || in.height > 32768) return false;
    g.W = in.width; g.H = in.height; g.ncomp = in.components; g.hs = in.h_samp; g.vs = in.v_samp;
    g.ri = in.restart_interval;
    g.mx = (g.W + 8 * g.hs - 1) / (8 * g.hs);
    g.my = (g.H + 8 * g.vs - 1) / (8 * g.vs);
    g.n_mcu = g.mx * g.my;
    g.nluma = g.hs * g.vs;
    g.bpm = g.ncomp == 1 ? 1 : g.nluma + 2;
    g.n_blk = g.n_mcu * g.bpm;
    g.n_int = g.ri > 0 ? (g.n_mcu + g.ri - 1) / g.ri : 1;
    g.cw = (g.W + g.hs - 1) / g.hs; g.ch = (g.H + g.vs - 1) / g.vs;
    g.yp = g.mx * 8 * g.hs; g.yrows = g.my * 8 * g.vs;
    g.cp = g.mx * 8; g.crows = g.my * 8;
    g.plane_bytes = (uint32_t)g.yp * g.yrows + (g.ncomp == 3 ? 2u * g.cp * g.crows : 0u);
    return true;
}

// natural (row * 8 + column) index -> zig-zag index
EVAM_HD inline int jdec_nat_to_zig(int k) {
    constexpr uint8_t t[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                               41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                               46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return t[k & 63];
}

// ---------------------------------------------------------------------------------------------------------------
// Header parse (host only): the markers up to and including SOS.
// ---------------------------------------------------------------------------------------------------------------

// Build one table from a DHT segment's 16 counts and its symbols. false: the counts over-subscribe the code space.
inline bool jdec_build_huff(const uint8_t* counts, const uint8_t* syms, int nsyms, JdecHuff& h) {
    memset(&h, 0, sizeof(h));
    for (int i = 0; i < nsyms; i++) h.vals[i] = syms[i];
    int code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) return false;
        h.valoff[l] = k - code;
        h.maxcode[l] = n ? code + n - 1 : -1;
        if (l <= kJdecLook)
            for (int i = 0; i < n; i++) {
                const int first = (code + i) << (kJdecLook - l);
                for (int j = 0; j < (1 << (kJdecLook - l)); j++) h.look[first + j] = (uint16_t)(l << 8 | syms[k + i]);
            }
        code = (code + n) << 1;
        k += n;
    }
    return true;
}

#define JDEC_FAIL(code, ...) do { if (msg && cap) snprintf(msg, cap, __VA_ARGS__); return (code); } while (0)

// Returns EVAM_PP_OK / EVAM_PP_ERR_INVALID_ARG / EVAM_PP_ERR_UNSUPPORTED; on failure msg names the reason.
// file_out may be NULL (evam_pp_jpeg_info); raw_off is left 0.
inline int jdec_parse(const uint8_t* f, size_t len, evam_jpeg_info* info, JdecFile* file_out, char* msg, size_t cap) {
    if (!f || !info) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "NULL argument");
    if (len >= kJdecMaxLen) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "file of %zu bytes: the limit is 2^28 - 1", len);
    if (len < 4 || f[0] != 0xFF || f[1] != 0xD8) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "no SOI marker: not a JPEG file");
    uint8_t qt[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
    JdecHuff* huff = new JdecHuff[4];
    struct Free { JdecHuff* p; ~Free() { delete[] p; } } free_huff{huff};
    int nc = 0, cid[3] = {0, 0, 0}, chs[3] = {1, 1, 1}, cvs[3] = {1, 1, 1}, ctq[3] = {0, 0, 0};
    int W = 0, H = 0, ri = 0, adobe = -1;
    bool jfif = false, sof = false;
    size_t pos = 2;
    // every pass consumes at least two bytes: at most len / 2 passes
    for (size_t pass = 0; pass < len; pass++) {
        if (pos + 2 > len) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "the file ends before a scan (SOS) starts");
        if (f[pos] != 0xFF) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "byte %zu: 0x%02X where a marker should start", pos, f[pos]);
        const int m = f[pos + 1];
        if (m == 0xFF) { pos++; continue; }  // a fill byte
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // stand-alone markers
        if (m == 0xD8 || m == 0xD9 || m == 0x00)
            JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "marker 0xFF%02X before the scan", m);
        if (pos + 2 > len) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "segment 0xFF%02X runs past the end of the file", m);
        const size_t L = (size_t)f[pos] << 8 | f[pos + 1];
        if (L < 2 || pos + L > len)
            JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "segment 0xFF%02X of length %zu runs past the end of the file", m, L);
        const uint8_t* d = f + pos + 2;
        const size_t n = L - 2;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC0) {
            static const char* const kinds[16] = {
                "", "extended sequential", "progressive", "lossless", "", "differential sequential",
                "differential progressive", "differential lossless", "reserved (JPG)", "arithmetic-coded sequential",
                "arithmetic-coded progressive", "arithmetic-coded lossless", "arithmetic conditioning (DAC)",
                "arithmetic-coded differential", "arithmetic-coded differential", "arithmetic-coded differential"};
            JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "%s JPEG (marker 0xFF%02X): only baseline sequential (SOF0) files are "
                      "decoded", kinds[m - 0xC0], m);
        }
        if (m == 0xC0) {
            if (sof) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "a second frame header (SOF0)");
            if (n < 6) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "SOF0 segment of %zu bytes is too short", n);
            if (d[0] != 8) JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "%d-bit samples: only 8-bit files are decoded", d[0]);
            H = d[1] << 8 | d[2]; W = d[3] << 8 | d[4]; nc = d[5];
            if (W == 0 || H == 0) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "zero size %dx%d", W, H);
            if (W > 32768 || H > 32768) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "size %dx%d: the limit is 32768", W, H);
            if (nc != 1 && nc != 3)
                JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "%d components: only 1 (grey) and 3 (YCbCr) are decoded", nc);
            if (n < (size_t)6 + 3 * nc) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "SOF0 segment of %zu bytes is too short", n);
            for (int c = 0; c < nc; c++) {
                cid[c] = d[6 + 3 * c];
                chs[c] = d[7 + 3 * c] >> 4; cvs[c] = d[7 + 3 * c] & 15;
                ctq[c] = d[8 + 3 * c];
                if (ctq[c] > 3) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "component %d names quantisation table %d", c, ctq[c]);
            }
            sof = true;
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < n) {  // each table consumes 65 bytes
                const int pq = d[o] >> 4, tq = d[o] & 15;
                if (pq != 0) JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "16-bit quantisation table: only 8-bit tables are decoded");
                if (tq > 3) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "quantisation table id %d", tq);
                if (o + 65 > n) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "DQT segment is too short for its table");
                memcpy(qt[tq], d + o + 1, 64);
                have_q[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < n) {  // each table consumes at least 17 bytes
                const int tc = d[o] >> 4, th = d[o] & 15;
                if (tc > 1 || th > 3) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "Huffman table class %d id %d", tc, th);
                if (th > 1) JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "Huffman table id %d: a baseline file has ids 0 and 1", th);
                if (o + 17 > n) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "DHT segment is too short for its counts");
                int total = 0;
                for (int i = 0; i < 16; i++) total += d[o + 1 + i];
                if (total > 256 || o + 17 + total > n)
                    JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "DHT segment is too short for its %d symbols", total);
                if (!jdec_build_huff(d + o + 1, d + o + 17, total, huff[tc * 2 + th]))
                    JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "Huffman table %d/%d has more codes than its lengths allow", tc, th);
                have_h[tc * 2 + th] = true;
                o += 17 + total;
            }
        } else if (m == 0xDD) {
            if (n < 2) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "DRI segment is too short");
            ri = d[0] << 8 | d[1];
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(d, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(d, "Adobe", 5) == 0) adobe = d[11];
        } else if (m == 0xDA) {
            if (!sof) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "a scan (SOS) before the frame header (SOF0)");
            if (n < 1) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "SOS segment is too short");
            const int ns = d[0];
            if (ns < 1 || ns > 4 || n != (size_t)4 + 2 * ns) JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "SOS segment of %zu bytes "
                                                                       "for %d components", n, ns);
            if (ns != nc) JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "a scan of %d of the %d components: only one interleaved "
                                    "scan over all components is decoded", ns, nc);
            if (d[1 + 2 * ns] != 0 || d[2 + 2 * ns] != 63 || d[3 + 2 * ns] != 0)
                JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "scan with spectral selection %d..%d, approximation 0x%02X: only a "
                          "full baseline scan is decoded", d[1 + 2 * ns], d[2 + 2 * ns], d[3 + 2 * ns]);
            int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
            for (int c = 0; c < ns; c++) {
                if (d[1 + 2 * c] != cid[c])
                    JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "scan lists component id %d where the frame has %d", d[1 + 2 * c], cid[c]);
                td[c] = d[2 + 2 * c] >> 4; ta[c] = d[2 + 2 * c] & 15;
                if (td[c] > 1 || ta[c] > 1 || !have_h[td[c]] || !have_h[2 + ta[c]])
                    JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "scan names Huffman tables DC %d / AC %d, which the file never "
                              "defined", td[c], ta[c]);
                if (!have_q[ctq[c]])
                    JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "component %d names quantisation table %d, which the file never "
                              "defined", c, ctq[c]);
            }
            int hs = 1, vs = 1;
            if (nc == 3) {
                hs = chs[0]; vs = cvs[0];
                const bool ok = chs[1] == 1 && cvs[1] == 1 && chs[2] == 1 && cvs[2] == 1 &&
                                ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
                if (!ok) JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "sampling %dx%d,%dx%d,%dx%d: only 4:4:4, 4:2:2 and 4:2:0 are "
                                   "decoded", chs[0], cvs[0], chs[1], cvs[1], chs[2], cvs[2]);
                if (adobe >= 0 && adobe != 1)
                    JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "Adobe transform %d: only YCbCr (1) files are decoded", adobe);
                if (adobe < 0 && !jfif && cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')
                    JDEC_FAIL(EVAM_PP_ERR_UNSUPPORTED, "RGB components: only YCbCr files are decoded");
            }
            info->width = W; info->height = H; info->components = nc;
            info->h_samp = hs; info->v_samp = vs;
            info->restart_interval = ri;
            info->scan_offset = (uint32_t)(pos + L);
            if (file_out) {
                memset(file_out, 0, sizeof(*file_out));
                for (int i = 0; i < 4; i++)
                    if (have_h[i]) file_out->huff[i] = huff[i];
                for (int c = 0; c < nc; c++) {
                    memcpy(file_out->q[c], qt[ctq[c]], 64);
                    file_out->dc_tab[c] = (uint8_t)td[c];
                    file_out->ac_tab[c] = (uint8_t)(2 + ta[c]);
                }
                file_out->scan_len = (uint32_t)(len - (pos + L));
            }
            return EVAM_PP_OK;
        }
        pos += L;  // APPn, COM and everything else: skipped
    }
    JDEC_FAIL(EVAM_PP_ERR_INVALID_ARG, "the file ends before a scan (SOS) starts");
}

// ---------------------------------------------------------------------------------------------------------------
// Un-stuffing: what byte j of the entropy-coded data d[0, n) is, from its neighbours alone.
// ---------------------------------------------------------------------------------------------------------------
enum { kJdecKeep = 0, kJdecDrop = 1, kJdecRst = 2, kJdecEnd = 3 };

EVAM_HD inline int jdec_byte_kind(const uint8_t* d, uint32_t n, uint32_t j) {
    const int b = d[j];
    const int prev = j > 0 ? d[j - 1] : 0;
    if (prev == 0xFF && b != 0xFF) {
        if (b == 0) return kJdecDrop;                  // the stuffed zero behind a data FF
        return (b >= 0xD0 && b <= 0xD7) ? kJdecRst : kJdecEnd;  // a marker's code: RSTn, or one that ends the scan
    }
    if (b == 0xFF) {
        if (j + 1 >= n) return kJdecEnd;               // an FF with nothing behind it
        return d[j + 1] == 0 ? kJdecKeep : kJdecDrop;  // data, or a fill byte / a marker's first byte
    }
    return kJdecKeep;
}

// The sequential form (host twin, sanitizer program). out holds n + kJdecStreamPad bytes; first holds n_int + 1
// entries: first[k] is interval k's first byte in out, first[n_int] the end of the last one. Returns 0, or
// EVAM_PP_ERR_INVALID_ARG when the restart markers are not exactly RST0, RST1, .. in n_int - 1 places.
inline int jdec_unstuff_host(const uint8_t* d, uint32_t n, int n_int, uint8_t* out, uint32_t* first) {
    uint32_t kept = 0, rst = 0;
    int err = 0;
    first[0] = 0;
    for (uint32_t j = 0; j < n; j++) {
        const int kind = jdec_byte_kind(d, n, j);
        if (kind == kJdecEnd) break;
        if (kind == kJdecKeep) out[kept++] = d[j];
        else if (kind == kJdecRst) {
            if ((d[j] & 7) != (int)(rst & 7)) err = EVAM_PP_ERR_INVALID_ARG;
            if (rst + 1 <= (uint32_t)n_int) first[rst + 1] = kept;
            rst++;
        }
    }
    if (rst != (uint32_t)n_int - 1) err = EVAM_PP_ERR_INVALID_ARG;
    for (uint32_t k = rst + 1; k <= (uint32_t)n_int; k++) first[k] = kept;
    for (int i = 0; i < kJdecStreamPad; i++) out[kept + i] = 0;
    return err;
}

// ---------------------------------------------------------------------------------------------------------------
// Entropy decoding (ITU-T T.81 Annex F) from a decoder state.
// ---------------------------------------------------------------------------------------------------------------

// A decoder state: bit position p in the file's compacted scan, and bz = block index inside the MCU << 8 | zig-zag
// index of the next coefficient.
struct JdecScan {
    const uint8_t* stream;   // the compacted scan, 4-byte aligned; readable up to the interval's last byte + 8
    const JdecFile* file;
    int32_t nluma, bpm;
};

// 32 bits from bit position p, most significant first: two aligned words of the scan.
EVAM_HD inline uint32_t jdec_peek(const JdecScan& sc, uint32_t p) {
    uint32_t w[2];
    memcpy(w, sc.stream + (size_t)(p >> 5) * 4, 8);
    const uint64_t v = (uint64_t)__builtin_bswap32(w[0]) << 32 | __builtin_bswap32(w[1]);
    return (uint32_t)((v << (p & 31)) >> 32);
}

// symbol of the code at the top of w, its length in len; -1 when the bits are no code of the table
EVAM_HD inline int jdec_huff(const JdecHuff& h, uint32_t w, int& len) {
    const uint32_t e = h.look[w >> (32 - kJdecLook)];
    if (e) { len = (int)(e >> 8); return (int)(e & 255); }
    for (int l = kJdecLook + 1; l <= 16; l++) {
        const int code = (int)(w >> (32 - l));
        if (code <= h.maxcode[l]) { len = l; return h.vals[(h.valoff[l] + code) & 255]; }
    }
    return -1;
}

// s extra bits -> the signed value (T.81 F.2.2.1 EXTEND)
EVAM_HD inline int jdec_extend(uint32_t bits, int s) {
    return s == 0 ? 0 : ((bits >> (s - 1)) ? (int)bits : (int)bits - (1 << s) + 1);
}

// Decode from (p, bz) until p reaches stop (a sub-sequence's end; symbols that start before it are finished) or the
// interval's end. Returns the number of blocks completed; p and bz become the exit state.
// coef != NULL: the write pass. blk is the scan index of the block the entry state lies in; symbols of blocks below
// blk_limit store their value at coef[block * 64 + zig-zag index] (DC differences raw) and raise err for what no
// baseline scan holds; decoding stops at blk_limit. coef == NULL: the synchronising pass, which stores and flags
// nothing.
// A pattern that is no code consumes one bit, so every step consumes at least one: the loop's bound is the number of
// bits in front of stop. Nothing is read behind the byte of end + 8.
EVAM_HD inline uint32_t jdec_run(const JdecScan& sc, uint32_t& p, uint32_t& bz, uint32_t stop, uint32_t end,
                                 int16_t* coef, uint32_t blk, uint32_t blk_limit, int& err) {
    uint32_t done = 0;
    uint32_t b = bz >> 8, z = bz & 255;
    if (stop > end) stop = end;
    const uint32_t max_steps = p < stop ? stop - p : 0;
    for (uint32_t step = 0; step < max_steps && p < stop; step++) {
        if (coef && blk >= blk_limit) break;
        const uint32_t w = jdec_peek(sc, p);
        const int comp = (int)b < sc.nluma ? 0 : (int)b - sc.nluma + 1;
        const bool dc = z == 0;
        const JdecHuff& h = sc.file->huff[(dc ? sc.file->dc_tab[comp] : sc.file->ac_tab[comp]) & 3];
        int len = 0;
        const int sym = jdec_huff(h, w, len);
        if (sym < 0) {  // no code: give up one bit and go on
            if (coef) err = 1;
            p += 1;
            continue;
        }
        const int s = sym & 15, r = dc ? 0 : sym >> 4;
        const uint32_t used = (uint32_t)(len + s);  // <= kJdecMaxSymBits
        if (p + used > end) {  // the data ends inside this symbol
            if (coef) err = 1;
            p = end;
            break;
        }
        const uint32_t bits = s ? (w << len) >> (32 - s) : 0u;
        const int v = jdec_extend(bits, s);
        p += used;
        if (dc) {
            if (coef) {
                if (sym > 11) err = 1;
                coef[(size_t)blk * 64] = (int16_t)v;
            }
            z = 1;
        } else if (s == 0) {
            if (r == 15) {
                z += 16;
                if (z > 64) { if (coef) err = 1; z = 64; }
            } else {
                if (r != 0 && coef) err = 1;  // EOBn belongs to progressive scans
                z = 64;
            }
        } else {
            z += (uint32_t)r;
            if (z > 63) {
                if (coef) err = 1;  // a run past coefficient 63
                z = 64;
            } else {
                if (coef) {
                    if (s > 10) err = 1;
                    coef[(size_t)blk * 64 + z] = (int16_t)v;
                }
                z++;
            }
        }
        if (z >= 64) {
            z = 0;
            b = b + 1 >= (uint32_t)sc.bpm ? 0 : b + 1;
            blk++;
            done++;
        }
    }
    bz = b << 8 | z;
    return done;
}

// ---------------------------------------------------------------------------------------------------------------
// Dequantise + jidctint.c's jpeg_idct_islow, one column / one row at a time (JLONG arithmetic: 64-bit).
// ---------------------------------------------------------------------------------------------------------------
EVAM_HD inline int jdec_range_limit(int64_t x) {
    const int v = (int)(x & 1023);
    return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

// in[8] -> out[8]; shift: 11 for the column pass, 18 for the row pass
EVAM_HD inline void jdec_idct_1d(const int64_t* in, int64_t* out, int shift) {
    constexpr int64_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633,
                      F1_501 = 12299, F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    int64_t z2 = in[2], z3 = in[6];
    int64_t z1 = (z2 + z3) * F0_541;
    int64_t tmp2 = z1 - z3 * F1_847;
    int64_t tmp3 = z1 + z2 * F0_765;
    z2 = in[0]; z3 = in[4];
    int64_t tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;
    const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    const int64_t z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298; tmp1 *= F2_053; tmp2 *= F3_072; tmp3 *= F1_501;
    z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    const int64_t rnd = (int64_t)1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + rnd) >> shift; out[7] = (tmp10 - tmp3 + rnd) >> shift;
    out[1] = (tmp11 + tmp2 + rnd) >> shift; out[6] = (tmp11 - tmp2 + rnd) >> shift;
    out[2] = (tmp12 + tmp1 + rnd) >> shift; out[5] = (tmp12 - tmp1 + rnd) >> shift;
    out[3] = (tmp13 + tmp0 + rnd) >> shift; out[4] = (tmp13 - tmp0 + rnd) >> shift;
}

// column c of a block: coef in zig-zag order (DC already summed), q in zig-zag order -> ws[r * 8 + c], r = 0..7
EVAM_HD inline void jdec_idct_column(const int16_t* coef, const uint8_t* q, int c, int32_t* ws) {
    int64_t in[8], out[8];
    for (int r = 0; r < 8; r++) {
        const int zz = jdec_nat_to_zig(r * 8 + c);
        in[r] = (int64_t)coef[zz] * q[zz];
    }
    jdec_idct_1d(in, out, 11);
    for (int r = 0; r < 8; r++) ws[r * 8 + c] = (int32_t)out[r];
}

// row r of a block from the column pass's workspace -> 8 samples
EVAM_HD inline void jdec_idct_row(const int32_t* ws, int r, uint8_t* px) {
    int64_t in[8], out[8];
    for (int c = 0; c < 8; c++) in[c] = ws[r * 8 + c];
    jdec_idct_1d(in, out, 18);
    for (int c = 0; c < 8; c++) px[c] = (uint8_t)jdec_range_limit(out[c]);
}

// Where block `blk` of the scan lies: its component and the top-left sample inside that component's plane.
EVAM_HD inline void jdec_block_pos(const JdecGeom& g, uint32_t blk, int& comp, int& x0, int& y0) {
    const int mcu = (int)(blk / (uint32_t)g.bpm), k = (int)(blk % (uint32_t)g.bpm);
    const int mxi = mcu % g.mx, myi = mcu / g.mx;
    if (k < g.nluma) {
        comp = 0;
        x0 = (mxi * g.hs + k % g.hs) * 8;
        y0 = (myi * g.vs + k / g.hs) * 8;
    } else {
        comp = k - g.nluma + 1;
        x0 = mxi * 8; y0 = myi * 8;
    }
}

EVAM_HD inline uint32_t jdec_plane_off(const JdecGeom& g, int comp) {
    return comp == 0 ? 0u : (uint32_t)g.yp * g.yrows + (uint32_t)(comp - 1) * g.cp * g.crows;
}

// ---------------------------------------------------------------------------------------------------------------
// Up-sampling (jdsample.c, fancy) and colour (jdcolor.c).
// ---------------------------------------------------------------------------------------------------------------

// The chroma sample of output pixel (x, y) from plane c (pitch g.cp, real size g.cw x g.ch).
EVAM_HD inline int jdec_chroma(const JdecGeom& g, const uint8_t* c, int x, int y) {
    if (g.hs == 1) return c[(size_t)y * g.cp + x];
    const int i = x >> 1, n = g.cw;
    if (g.vs == 1) {  // h2v1
        const uint8_t* r = c + (size_t)y * g.cp;
        if (n <= 2) return r[i];
        if (!(x & 1)) return i == 0 ? r[0] : (3 * r[i] + r[i - 1] + 1) >> 2;
        return i == n - 1 ? r[n - 1] : (3 * r[i] + r[i + 1] + 2) >> 2;
    }
    const int yn = y >> 1;  // h2v2
    if (n <= 2) return c[(size_t)yn * g.cp + i];
    int yf = (y & 1) ? yn + 1 : yn - 1;
    yf = yf < 0 ? 0 : yf > g.ch - 1 ? g.ch - 1 : yf;
    const uint8_t* rn = c + (size_t)yn * g.cp;
    const uint8_t* rf = c + (size_t)yf * g.cp;
    const int s = 3 * rn[i] + rf[i];
    if (!(x & 1)) return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * rn[i - 1] + rf[i - 1] + 8) >> 4;
    return i == n - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * rn[i + 1] + rf[i + 1] + 7) >> 4;
}

EVAM_HD inline int jdec_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// b | g << 8 | r << 16 | 255 << 24 of pixel (x, y) from one file's planes
EVAM_HD inline uint32_t jdec_pixel(const JdecGeom& g, const uint8_t* planes, int x, int y) {
    const int Y = planes[(size_t)y * g.yp + x];
    if (g.ncomp == 1) return (uint32_t)Y * 0x010101u | 0xFF000000u;
    const int cb = jdec_chroma(g, planes + jdec_plane_off(g, 1), x, y) - 128;
    const int cr = jdec_chroma(g, planes + jdec_plane_off(g, 2), x, y) - 128;
    const int R = jdec_clamp8(Y + ((91881 * cr + 32768) >> 16));
    const int B = jdec_clamp8(Y + ((116130 * cb + 32768) >> 16));
    const int G = jdec_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    return (uint32_t)B | (uint32_t)G << 8 | (uint32_t)R << 16 | 0xFF000000u;
}

// ---------------------------------------------------------------------------------------------------------------
// The whole decode of one file on the host, driven sequentially (evam_pp_decode_jpeg_host). The file was parsed.
// work: g.n_blk * 64 int16 + plane_bytes + scan_len + kJdecStreamPad bytes + (n_int + 1) uint32, carved by the caller.
// ---------------------------------------------------------------------------------------------------------------

// DC differences -> DC values, per component and restart interval, in place.
inline void jdec_dc_host(const JdecGeom& g, int16_t* coef, int& err) {
    for (int k = 0; k < g.n_int; k++) {
        int64_t dc[3] = {0, 0, 0};  // 64 bits: a damaged file's sum leaves int32 as well, and only err records it
        const int m0 = g.ri > 0 ? k * g.ri : 0, m1 = g.ri > 0 ? (m0 + g.ri < g.n_mcu ? m0 + g.ri : g.n_mcu) : g.n_mcu;
        for (uint32_t blk = (uint32_t)m0 * g.bpm; blk < (uint32_t)m1 * g.bpm; blk++) {
            const int kk = (int)(blk % (uint32_t)g.bpm), comp = kk < g.nluma ? 0 : kk - g.nluma + 1;
            dc[comp] += coef[(size_t)blk * 64];
            if (dc[comp] < -32768 || dc[comp] > 32767) err = 1;
            coef[(size_t)blk * 64] = (int16_t)dc[comp];
        }
    }
}

inline void jdec_dc_and_idct_host(const JdecGeom& g, const JdecFile& file, int16_t* coef, uint8_t* planes, int& err) {
    jdec_dc_host(g, coef, err);
    for (uint32_t blk = 0; blk < (uint32_t)g.n_blk; blk++) {
        int comp, x0, y0;
        jdec_block_pos(g, blk, comp, x0, y0);
        const int pitch = comp == 0 ? g.yp : g.cp;
        int32_t ws[64];
        for (int c = 0; c < 8; c++) jdec_idct_column(coef + (size_t)blk * 64, file.q[comp], c, ws);
        for (int r = 0; r < 8; r++)
            jdec_idct_row(ws, r, planes + jdec_plane_off(g, comp) + (size_t)(y0 + r) * pitch + x0);
    }
}

inline void jdec_colour_host(const JdecGeom& g, const uint8_t* planes, uint8_t* out, int pitch, int bpp) {
    for (int y = 0; y < g.H; y++)
        for (int x = 0; x < g.W; x++) {
            const uint32_t px = jdec_pixel(g, planes, x, y);
            uint8_t* o = out + (size_t)y * pitch + (size_t)x * bpp;
            o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
            if (bpp == 4) o[3] = 255;
        }
}

// ---------------------------------------------------------------------------------------------------------------
// Raw 4:2:0 planes (evam_pp_decode_jpeg_planes): every component's IDCT output, cropped, straight into the caller's
// NV12 / I420 planes. No up-sampling and no colour conversion: what libjpeg's jpeg_read_raw_data returns.
// ---------------------------------------------------------------------------------------------------------------

// One file's output planes (NV12: p[0..1], I420: p[0..2]); bases and pitches are multiples of 16.
struct JdecPlanesOut {
    uint8_t* p[3];
    int32_t pitch[3];
    int32_t pad[3];
};

// Geometry the planes path serves: 4:2:0 of even width and height.
EVAM_HD inline bool jdec_planes_ok(const evam_jpeg_info& in) {
    return in.components == 3 && in.h_samp == 2 && in.v_samp == 2 && !(in.width & 1) && !(in.height & 1);
}

// The one store of the planes path: N (8 or 16) bytes px of row y, from byte xb of the row, clipped to a plane of
// row_bytes x rows pixel bytes. xb is a multiple of N and the plane's base and pitch are multiples of 16, so a
// segment wholly inside the row is one aligned N-byte store; a segment that straddles the row's end is stored byte by
// byte up to it; a segment behind it, or a row at or past rows, stores nothing.
template <int N>
EVAM_HD inline void jdec_store_clipped(uint8_t* plane, int pitch, int xb, int y, int row_bytes, int rows,
                                       const uint8_t* px) {
    static_assert(N == 8 || N == 16, "an 8- or 16-byte segment");
    typedef uint32_t Seg __attribute__((vector_size(N), may_alias));  // one store instruction, aligned to N
    if (y >= rows || xb >= row_bytes) return;
    uint8_t* o = plane + (size_t)y * pitch + xb;
    if (xb + N <= row_bytes) {
        Seg v;
        memcpy(&v, px, N);
        *reinterpret_cast<Seg*>(o) = v;
    } else {
        for (int i = 0; xb + i < row_bytes; i++) o[i] = px[i];
    }
}

constexpr int kJdecPlaneRows = 24;  // row tasks of one 4:2:0 MCU: 16 luma rows, 8 chroma rows

// Row task t of MCU `mcu` from the column pass's six workspaces ws[6][64] (Y00 Y01 Y10 Y11 Cb Cr, the scan's order).
// t < 16: luma row t of the MCU, the rows of its two horizontally adjacent blocks as one 16-byte segment.
// t >= 16: row t - 16 of the Cb and the Cr block: 16 interleaved bytes (NV12) or 8 bytes into each plane (I420).
template <bool NV12>
EVAM_HD inline void jdec_planes_row(const JdecGeom& g, const JdecPlanesOut& o, int mcu, int t, const int32_t* ws) {
    const int mxi = mcu % g.mx, myi = mcu / g.mx;
    alignas(16) uint8_t px[16];
    if (t < 16) {
        const int32_t* w = ws + (t >> 3) * 128;
        jdec_idct_row(w, t & 7, px);
        jdec_idct_row(w + 64, t & 7, px + 8);
        jdec_store_clipped<16>(o.p[0], o.pitch[0], mxi * 16, myi * 16 + t, g.W, g.H, px);
        return;
    }
    const int r = t - 16, y = myi * 8 + r;
    if (NV12) {
        uint8_t cb[8], cr[8];
        jdec_idct_row(ws + 4 * 64, r, cb);
        jdec_idct_row(ws + 5 * 64, r, cr);
        for (int i = 0; i < 8; i++) { px[2 * i] = cb[i]; px[2 * i + 1] = cr[i]; }
        jdec_store_clipped<16>(o.p[1], o.pitch[1], mxi * 16, y, g.W, g.H / 2, px);
    } else {
        jdec_idct_row(ws + 4 * 64, r, px);
        jdec_idct_row(ws + 5 * 64, r, px + 8);
        jdec_store_clipped<8>(o.p[1], o.pitch[1], mxi * 8, y, g.W / 2, g.H / 2, px);
        jdec_store_clipped<8>(o.p[2], o.pitch[2], mxi * 8, y, g.W / 2, g.H / 2, px + 8);
    }
}

// The host twin of evam_jdec_idct_planes: the same row tasks, MCU by MCU. coef holds the scan's raw DC differences.
template <bool NV12>
inline void jdec_planes_host(const JdecGeom& g, const JdecFile& file, int16_t* coef, const JdecPlanesOut& o, int& err) {
    jdec_dc_host(g, coef, err);
    int32_t ws[6 * 64];
    for (int mcu = 0; mcu < g.n_mcu; mcu++) {
        for (int k = 0; k < 6; k++)
            for (int c = 0; c < 8; c++)
                jdec_idct_column(coef + ((size_t)mcu * 6 + k) * 64, file.q[k < 4 ? 0 : k - 3], c, ws + k * 64);
        for (int t = 0; t < kJdecPlaneRows; t++) jdec_planes_row<NV12>(g, o, mcu, t, ws);
    }
}
