// evam_jpeg_dec_kernels.h - the six kernels of evam_pp_decode_jpeg (gfx950). Included by evam_pp.hip inside its
// anonymous namespace; the arithmetic is evam_jpeg_dec.h's, shared with the host twin.
//
//   1 evam_jdec_unstuff  one workgroup per file: drops stuffed zeros, finds RSTn / the scan's end, compacts the scan
//                        and writes the interval table (first byte of every restart interval)
//   2 evam_jdec_sync     one workgroup per (interval, file): self-synchronising sub-sequence decoding, kJdecChunk
//                        sub-sequences of kJdecSubBits bits at a time, in order, with a carry
//   3 evam_jdec_write    one thread per sub-sequence: decodes from its final entry state and stores coefficients
//   4 evam_jdec_dc       one workgroup per (interval, file): DC differences -> DC values, per component
//   5 evam_jdec_idct     eight threads per block: dequantise, both IDCT passes, range limit -> component planes
//   6 evam_jdec_colour   one thread per VEC pixels: fancy up-sampling + YCbCr -> BGR / BGRX rows
// evam_pp_decode_jpeg_planes runs kernels 1 to 4 and then evam_jdec_idct_planes in place of 5 and 6: five launches.
//
// No kernel talks to another workgroup: every hand-off is a kernel boundary on the handle's stream. Every loop over
// file data is bounded by a length the host validated (scan_len, n_int, n_slots, n_mcu) and every store is checked
// against its buffer, so a damaged scan ends with a status and nothing else.
#pragma once

struct JdecOut {
    uint8_t* p;
    int32_t pitch;
    int32_t pad;
};

struct JdecParams {
    JdecGeom g;
    const JdecFile* files;   // [n]
    const JdecOut* outs;     // [n] (BGR / BGRX output)
    const JdecPlanesOut* pouts;  // [n] (NV12 / I420 output)
    const uint8_t* raw;      // the files' entropy-coded bytes, file i at files[i].raw_off
    uint8_t* stream;         // [n][stream_stride] compacted scans
    uint32_t stream_stride;
    uint32_t* first;         // [n][n_int + 1] interval table
    uint4* slots;            // [n][n_slots] sub-sequence records: entry p, entry bz, first block, interval + 1
    uint32_t n_slots;
    int16_t* coef;           // [n][n_blk][64], zig-zag order
    uint8_t* planes;         // [n][plane_bytes] (BGR / BGRX output only)
    int32_t* status;         // [n]
};

constexpr int kJdecUnstuffBytes = 16;  // bytes per thread and pass of kernel 1

// inclusive scan of s[0, N) by N threads; the caller synchronised after writing s
template <int N>
__device__ inline void jdec_scan(uint32_t* s, int tid) {
    for (int d = 1; d < N; d <<= 1) {
        const uint32_t v = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void evam_jdec_unstuff(const JdecParams P) {
    __shared__ uint32_t s_cnt[256];  // kept bytes | RSTn markers << 16 of a thread's 16 bytes
    __shared__ uint32_t s_end;
    const int tid = threadIdx.x, fi = blockIdx.x;
    const JdecFile& f = P.files[fi];
    const uint8_t* d = P.raw + f.raw_off;
    const uint32_t n = f.scan_len;
    const uint32_t n_int = (uint32_t)P.g.n_int;
    uint8_t* out = P.stream + (size_t)fi * P.stream_stride;
    uint32_t* first = P.first + (size_t)fi * (n_int + 1);
    uint32_t kept = 0, rst = 0;  // uniform carries
    bool err = false;
    if (tid == 0) first[0] = 0;
    for (uint32_t base = 0; base < n; base += 256 * kJdecUnstuffBytes) {
        if (tid == 0) s_end = 0xFFFFFFFFu;
        __syncthreads();
        const uint32_t j0 = base + (uint32_t)tid * kJdecUnstuffBytes;
        // this thread's 16 bytes in one load (the raw buffer is 16-byte aligned and padded) and a neighbour each side
        union { uint4 v; uint8_t b[kJdecUnstuffBytes + 2]; } win;
        uint8_t* wb = win.b + 1;
        uint32_t kinds = 0;
        if (j0 < n) {
            union { uint4 v; uint8_t b[16]; } ld;
            ld.v = *reinterpret_cast<const uint4*>(d + j0);
            for (int i = 0; i < kJdecUnstuffBytes; i++) wb[i] = ld.b[i];
            wb[-1] = j0 > 0 ? d[j0 - 1] : 0;
            wb[kJdecUnstuffBytes] = j0 + kJdecUnstuffBytes < n ? d[j0 + kJdecUnstuffBytes] : 0;
        }
        for (int i = 0; i < kJdecUnstuffBytes; i++) {
            const uint32_t j = j0 + i;
            // jdec_byte_kind on the window: index i + 1 of n' = bytes of the window that lie inside the scan
            const uint32_t nw = j0 < n ? (n - j0 + 1 < kJdecUnstuffBytes + 2u ? n - j0 + 1 : kJdecUnstuffBytes + 2u) : 0u;
            const int kind = j < n ? jdec_byte_kind(win.b, nw, (uint32_t)i + 1) : kJdecDrop;
            kinds |= (uint32_t)kind << (2 * i);
            if (kind == kJdecEnd) atomicMin(&s_end, j);
        }
        __syncthreads();
        const uint32_t E = s_end;
        uint32_t nk = 0, nr = 0;
        for (int i = 0; i < kJdecUnstuffBytes; i++) {
            const int kind = (kinds >> (2 * i)) & 3;
            if (j0 + i < E) { nk += kind == kJdecKeep; nr += kind == kJdecRst; }
        }
        s_cnt[tid] = nk | nr << 16;  // at most 4,096 bytes and 2,048 markers per pass
        __syncthreads();
        jdec_scan<256>(s_cnt, tid);
        uint32_t ok = kept + (s_cnt[tid] & 0xFFFFu) - nk, orst = rst + (s_cnt[tid] >> 16) - nr;
        for (int i = 0; i < kJdecUnstuffBytes; i++) {
            const uint32_t j = j0 + i;
            const int kind = (kinds >> (2 * i)) & 3;
            if (j >= E || j >= n) break;
            if (kind == kJdecKeep) out[ok++] = wb[i];  // ok < kept bytes <= scan_len <= stream_stride - pad
            else if (kind == kJdecRst) {
                if ((uint32_t)(wb[i] & 7) != (orst & 7)) err = true;
                if (orst + 1 <= n_int) first[orst + 1] = ok;
                orst++;
            }
        }
        kept += s_cnt[255] & 0xFFFFu; rst += s_cnt[255] >> 16;
        __syncthreads();
        if (E != 0xFFFFFFFFu) break;
    }
    if (rst != n_int - 1) err = true;
    for (uint32_t k = rst + 1 + tid; k <= n_int; k += 256) first[k] = kept;
    if (tid < kJdecStreamPad) out[kept + tid] = 0;
    if (err) P.status[fi] = EVAM_PP_ERR_INVALID_ARG;
}

__device__ inline void jdec_load_file(JdecFile* s_file, const JdecFile* src, int tid, int nthreads) {
    const uint32_t* a = reinterpret_cast<const uint32_t*>(src);
    uint32_t* b = reinterpret_cast<uint32_t*>(s_file);
    for (int i = tid; i < (int)(sizeof(JdecFile) / 4); i += nthreads) b[i] = a[i];
}

// interval k of the file: its first and last MCU -> blocks [blk0, limit)
__device__ inline void jdec_interval_blocks(const JdecGeom& g, uint32_t k, uint32_t& blk0, uint32_t& limit) {
    const uint32_t m0 = g.ri > 0 ? k * (uint32_t)g.ri : 0u;
    uint32_t m1 = g.ri > 0 ? m0 + (uint32_t)g.ri : (uint32_t)g.n_mcu;
    if (m1 > (uint32_t)g.n_mcu) m1 = (uint32_t)g.n_mcu;
    blk0 = m0 * (uint32_t)g.bpm; limit = m1 * (uint32_t)g.bpm;
}

__global__ __launch_bounds__(kJdecChunk) void evam_jdec_sync(const JdecParams P) {
    static_assert(kJdecChunk <= 1024 && kJdecChunk % 64 == 0, "one workgroup of whole waves");
    __shared__ JdecFile s_file;
    __shared__ uint32_t s_p[kJdecChunk], s_bz[kJdecChunk], s_cnt[kJdecChunk];
    const int tid = threadIdx.x, fi = blockIdx.y;
    const uint32_t k = blockIdx.x;
    jdec_load_file(&s_file, P.files + fi, tid, kJdecChunk);
    __syncthreads();
    const uint32_t* first = P.first + (size_t)fi * (P.g.n_int + 1);
    const uint32_t fb = first[k], fe = first[k + 1] >= fb ? first[k + 1] : fb;
    const uint32_t P0 = fb * 8, end = fe * 8;
    const uint32_t nsub = (fe - fb + kJdecSubBytes - 1) / kJdecSubBytes;
    const uint32_t slot0 = fb / kJdecSubBytes + k;
    uint32_t blk0, limit;
    jdec_interval_blocks(P.g, k, blk0, limit);
    JdecScan sc;
    sc.stream = P.stream + (size_t)fi * P.stream_stride;
    sc.file = &s_file;
    sc.nluma = P.g.nluma; sc.bpm = P.g.bpm;
    uint32_t carry_p = P0, carry_bz = 0, carry_blk = blk0;  // uniform
    int unused = 0;
    for (uint32_t c0 = 0; c0 < nsub; c0 += kJdecChunk) {
        const uint32_t i = c0 + tid;
        const bool active = i < nsub;
        const uint32_t start = P0 + i * kJdecSubBits;
        const uint32_t stop = start + kJdecSubBits < end ? start + kJdecSubBits : end;
        uint32_t ep = tid == 0 ? carry_p : start, ebz = tid == 0 ? carry_bz : 0u;  // entry state: true, or guessed
        uint32_t xp = ep, xbz = ebz, cnt = 0;
        if (active) cnt = jdec_run(sc, xp, xbz, stop, end, nullptr, 0, 0, unused);
        s_p[tid] = xp; s_bz[tid] = xbz;
        __syncthreads();
        // after round r the chunk's first r + 1 exits are final: at most kJdecChunk rounds in all
        for (int r = 1; r < kJdecChunk; r++) {
            bool redo = false;
            if (active && tid > 0 && (s_p[tid - 1] != ep || s_bz[tid - 1] != ebz)) {
                ep = s_p[tid - 1]; ebz = s_bz[tid - 1];
                redo = true;
            }
            __syncthreads();
            int changed = 0;
            if (redo) {
                uint32_t np = ep, nbz = ebz;
                cnt = jdec_run(sc, np, nbz, stop, end, nullptr, 0, 0, unused);
                if (np != xp || nbz != xbz) {
                    xp = np; xbz = nbz;
                    s_p[tid] = np; s_bz[tid] = nbz;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        s_cnt[tid] = active ? cnt : 0u;
        __syncthreads();
        jdec_scan<kJdecChunk>(s_cnt, tid);
        const uint32_t slot = slot0 + i;
        if (active && slot < P.n_slots)
            P.slots[(size_t)fi * P.n_slots + slot] = make_uint4(ep, ebz, carry_blk + s_cnt[tid] - cnt, k + 1);
        const uint32_t last = nsub - c0 < (uint32_t)kJdecChunk ? nsub - c0 - 1 : kJdecChunk - 1;
        carry_p = s_p[last]; carry_bz = s_bz[last]; carry_blk += s_cnt[kJdecChunk - 1];
        __syncthreads();
    }
    if (tid == 0 && carry_blk < limit) P.status[fi] = EVAM_PP_ERR_INVALID_ARG;  // the data ends before the last MCU
}

__global__ __launch_bounds__(256) void evam_jdec_write(const JdecParams P) {
    __shared__ JdecFile s_file;
    const int tid = threadIdx.x, fi = blockIdx.y;
    jdec_load_file(&s_file, P.files + fi, tid, 256);
    __syncthreads();
    const uint32_t slot = blockIdx.x * 256u + tid;
    if (slot >= P.n_slots) return;
    const uint4 rec = P.slots[(size_t)fi * P.n_slots + slot];
    if (rec.w == 0 || rec.w > (uint32_t)P.g.n_int) return;
    const uint32_t k = rec.w - 1;
    const uint32_t* first = P.first + (size_t)fi * (P.g.n_int + 1);
    const uint32_t fb = first[k], fe = first[k + 1] >= fb ? first[k + 1] : fb;
    const uint32_t i = slot - (fb / kJdecSubBytes + k);
    const uint32_t end = fe * 8;
    uint32_t stop = fb * 8 + (i + 1) * kJdecSubBits;
    if (stop > end) stop = end;
    uint32_t blk0, limit;
    jdec_interval_blocks(P.g, k, blk0, limit);
    JdecScan sc;
    sc.stream = P.stream + (size_t)fi * P.stream_stride;
    sc.file = &s_file;
    sc.nluma = P.g.nluma; sc.bpm = P.g.bpm;
    uint32_t p = rec.x, bz = rec.y;
    int err = 0;
    if (p < fb * 8 || rec.z < blk0) return;  // not a record kernel 2 wrote
    jdec_run(sc, p, bz, stop, end, P.coef + (size_t)fi * P.g.n_blk * 64, rec.z, limit, err);
    if (err) P.status[fi] = EVAM_PP_ERR_INVALID_ARG;
}

constexpr int kJdecDcThreads = 256;

__global__ __launch_bounds__(kJdecDcThreads) void evam_jdec_dc(const JdecParams P) {
    __shared__ int64_t s_sum[3][kJdecDcThreads];  // 64 bits: a damaged file's sums leave int32 as well
    const int lane = threadIdx.x, fi = blockIdx.y;
    const JdecGeom& g = P.g;
    uint32_t blk0, limit;
    jdec_interval_blocks(g, blockIdx.x, blk0, limit);
    const uint32_t m0 = blk0 / (uint32_t)g.bpm, m = (limit - blk0) / (uint32_t)g.bpm;
    const uint32_t per = (m + kJdecDcThreads - 1) / kJdecDcThreads;
    uint32_t a = m0 + lane * per, b = a + per;
    if (a > m0 + m) a = m0 + m;
    if (b > m0 + m) b = m0 + m;
    int16_t* coef = P.coef + (size_t)fi * g.n_blk * 64;
    int64_t sum[3] = {0, 0, 0};
    for (uint32_t mcu = a; mcu < b; mcu++)
        for (int kk = 0; kk < g.bpm; kk++)
            sum[kk < g.nluma ? 0 : kk - g.nluma + 1] += coef[((size_t)mcu * g.bpm + kk) * 64];
    for (int c = 0; c < 3; c++) s_sum[c][lane] = sum[c];
    __syncthreads();
    int64_t dc[3] = {0, 0, 0};
    for (int l = 0; l < lane; l++)
        for (int c = 0; c < 3; c++) dc[c] += s_sum[c][l];
    bool err = false;
    for (uint32_t mcu = a; mcu < b; mcu++)
        for (int kk = 0; kk < g.bpm; kk++) {
            const int c = kk < g.nluma ? 0 : kk - g.nluma + 1;
            int16_t* q = coef + ((size_t)mcu * g.bpm + kk) * 64;
            dc[c] += *q;
            if (dc[c] < -32768 || dc[c] > 32767) err = true;
            *q = (int16_t)dc[c];
        }
    if (err) P.status[fi] = EVAM_PP_ERR_INVALID_ARG;
}

__global__ __launch_bounds__(256) void evam_jdec_idct(const JdecParams P) {
    __shared__ int32_t s_ws[32][64];
    const int tid = threadIdx.x, fi = blockIdx.y;
    const int lb = tid >> 3, c = tid & 7;
    const uint32_t blk = blockIdx.x * 32u + lb;
    const bool valid = blk < (uint32_t)P.g.n_blk;
    int comp = 0, x0 = 0, y0 = 0;
    if (valid) {
        jdec_block_pos(P.g, blk, comp, x0, y0);
        jdec_idct_column(P.coef + ((size_t)fi * P.g.n_blk + blk) * 64, P.files[fi].q[comp], c, s_ws[lb]);
    }
    __syncthreads();
    if (!valid) return;
    union { uint8_t b[8]; uint2 v; } px;
    jdec_idct_row(s_ws[lb], c, px.b);
    const int pitch = comp == 0 ? P.g.yp : P.g.cp;
    uint8_t* o = P.planes + (size_t)fi * P.g.plane_bytes + jdec_plane_off(P.g, comp) + (size_t)(y0 + c) * pitch + x0;
    *reinterpret_cast<uint2*>(o) = px.v;  // 8-byte aligned: x0, the pitches and the plane offsets are multiples of 8
}

// The planes path's kernel 5 (evam_pp_decode_jpeg_planes, 4:2:0 only): coefficients -> the caller's NV12 / I420 planes,
// with no component planes in scratch and no second pass. A workgroup takes kJdecPlaneMcus MCUs: eight threads per
// block run the column pass into LDS, then kJdecPlaneRows threads per MCU each finish two block rows and store them
// as one 16-byte segment (I420 chroma: two 8-byte segments), clipped by jdec_store_clipped.
constexpr int kJdecPlaneMcus = 5;  // 30 blocks: 240 of 256 threads in the column pass, 120 in the row pass

template <bool NV12>
__global__ __launch_bounds__(256) void evam_jdec_idct_planes(const JdecParams P) {
    __shared__ int32_t s_ws[kJdecPlaneMcus * 6][64];
    const int tid = threadIdx.x, fi = blockIdx.y;
    const uint32_t mcu0 = blockIdx.x * (uint32_t)kJdecPlaneMcus;
    const int lb = tid >> 3, c = tid & 7;
    const uint32_t blk = mcu0 * 6u + lb;
    if (lb < kJdecPlaneMcus * 6 && blk < (uint32_t)P.g.n_blk) {
        const int k = lb % 6;
        jdec_idct_column(P.coef + ((size_t)fi * P.g.n_blk + blk) * 64, P.files[fi].q[k < 4 ? 0 : k - 3], c, s_ws[lb]);
    }
    __syncthreads();
    const int lm = tid / kJdecPlaneRows, t = tid % kJdecPlaneRows;
    if (lm >= kJdecPlaneMcus || mcu0 + lm >= (uint32_t)P.g.n_mcu) return;
    jdec_planes_row<NV12>(P.g, P.pouts[fi], (int)(mcu0 + lm), t, s_ws[lm * 6]);
}

// VEC pixels per thread; VEC * BPP bytes are stored as 32-bit words (one 16-byte store for 4 BGRX pixels), the row's
// last pixels byte by byte, so nothing behind width * BPP is written.
template <int BPP, int VEC>
__global__ __launch_bounds__(256) void evam_jdec_colour(const JdecParams P) {
    static_assert((VEC * BPP) % 4 == 0, "whole words");
    const int fi = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (x0 >= P.g.W || y >= P.g.H) return;
    const uint8_t* planes = P.planes + (size_t)fi * P.g.plane_bytes;
    const JdecOut out = P.outs[fi];
    uint8_t* o = out.p + (size_t)y * out.pitch + (size_t)x0 * BPP;
    if (x0 + VEC <= P.g.W) {
        uint32_t px[VEC];
        for (int i = 0; i < VEC; i++) px[i] = jdec_pixel(P.g, planes, x0 + i, y);
        if (BPP == 4) {
            if (VEC == 4) *reinterpret_cast<uint4*>(o) = make_uint4(px[0], px[1], px[2], px[3]);
            else for (int i = 0; i < VEC; i++) reinterpret_cast<uint32_t*>(o)[i] = px[i];
        } else {
            uint32_t w[VEC * 3 / 4];
            for (int q = 0; q < VEC / 4; q++) {  // four pixels -> three words
                const uint32_t a = px[4 * q] & 0xFFFFFFu, b = px[4 * q + 1] & 0xFFFFFFu, c = px[4 * q + 2] & 0xFFFFFFu,
                               d = px[4 * q + 3] & 0xFFFFFFu;
                w[3 * q] = a | b << 24; w[3 * q + 1] = b >> 8 | c << 16; w[3 * q + 2] = c >> 16 | d << 8;
            }
            for (int i = 0; i < VEC * 3 / 4; i++) reinterpret_cast<uint32_t*>(o)[i] = w[i];
        }
    } else {
        for (int i = 0; x0 + i < P.g.W; i++) {
            const uint32_t px = jdec_pixel(P.g, planes, x0 + i, y);
            o[i * BPP] = (uint8_t)px; o[i * BPP + 1] = (uint8_t)(px >> 8); o[i * BPP + 2] = (uint8_t)(px >> 16);
            if (BPP == 4) o[i * BPP + 3] = 255;
        }
    }
}
