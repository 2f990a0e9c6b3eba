// evam_pp_band, the band kernel (uniform 4:2:0 vertical upscales), and the helpers only it uses: vfinal_masked, kVMask,
// pack4_u8_sums, vmcnt_le. Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

namespace {

// vfinal for horizontal results already masked with kVMask (a kernel that reuses a source row's results).
constexpr uint32_t kVMask = 0xFFFF00u;
template <int OUT>
__device__ __forceinline__ uint32_t vfinal_masked(uint32_t D0m, uint32_t D1m, uint32_t b0s, uint32_t b1s) {
    const uint32_t x = mulhi_u24(b0s, D0m) + mulhi_u24(b1s, D1m) + 2u;
    return OUT != 0 ? (x & ~3u) : (x >> 2);
}

// u8 bytes (x >> 2) of four vertical-pass sums x = mulhi + mulhi + 2 < 2^16 (each result <= 255), packed little-endian: two u16 pairs, one packed
// shift each, one byte permute (5 VALU for 4 pixels instead of 4 shifts and 4 shift / or steps)
__device__ __forceinline__ uint32_t pack4_u8_sums(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const evam_u16x2 p01 = __builtin_bit_cast(evam_u16x2, x0 | (x1 << 16)) >> (evam_u16x2){2, 2};
    const evam_u16x2 p23 = __builtin_bit_cast(evam_u16x2, x2 | (x3 << 16)) >> (evam_u16x2){2, 2};
    return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, p23), __builtin_bit_cast(uint32_t, p01), 0x06040200u);
}

// Wait until at most n (>= 0, wave-uniform) vector-memory operations of this wave are outstanding, rounded down to
// 0-4, 6, 8, 12, 16 or 32: waiting for a few more operations than needed is always safe. A binary tree of scalar
// compares and branches in one asm block: 4-5 compares, one wait and one branch on every path. (The same tree in C was
// structurised by the compiler into flag registers carried through every level, ~25 scalar instructions per wait;
// same box, one launch at a time: C1 equal, C1 / I420 +2.2 %, profiles/r06n_vmcnt_asm_ab.txt. The tree itself costs a
// third of the scalar instructions of an exact 64-case jump, C1 +2 % against it: profiles/r04k2_vmcnt_coarse_ab.txt.)
__device__ __forceinline__ void vmcnt_le(int n) {
    n = __builtin_amdgcn_readfirstlane(n);
    asm volatile(
        "s_cmp_lt_i32 %0, 8\n\t"
        "s_cbranch_scc1 5f\n\t"
        "s_cmp_lt_i32 %0, 16\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_cmp_lt_i32 %0, 32\n\t"
        "s_cbranch_scc1 1f\n\t"
        "s_waitcnt vmcnt(32)\n\t"
        "s_branch 9f\n"
        "1:\n\t"
        "s_waitcnt vmcnt(16)\n\t"
        "s_branch 9f\n"
        "2:\n\t"
        "s_cmp_lt_i32 %0, 12\n\t"
        "s_cbranch_scc1 3f\n\t"
        "s_waitcnt vmcnt(12)\n\t"
        "s_branch 9f\n"
        "3:\n\t"
        "s_waitcnt vmcnt(8)\n\t"
        "s_branch 9f\n"
        "5:\n\t"
        "s_cmp_lt_i32 %0, 4\n\t"
        "s_cbranch_scc1 7f\n\t"
        "s_cmp_lt_i32 %0, 6\n\t"
        "s_cbranch_scc1 6f\n\t"
        "s_waitcnt vmcnt(6)\n\t"
        "s_branch 9f\n"
        "6:\n\t"
        "s_waitcnt vmcnt(4)\n\t"
        "s_branch 9f\n"
        "7:\n\t"
        "s_cmp_lt_i32 %0, 2\n\t"
        "s_cbranch_scc1 8f\n\t"
        "s_cmp_lt_i32 %0, 3\n\t"
        "s_cbranch_scc1 4f\n\t"
        "s_waitcnt vmcnt(3)\n\t"
        "s_branch 9f\n"
        "4:\n\t"
        "s_waitcnt vmcnt(2)\n\t"
        "s_branch 9f\n"
        "8:\n\t"
        "s_cmp_lt_i32 %0, 1\n\t"
        "s_cbranch_scc1 10f\n\t"
        "s_waitcnt vmcnt(1)\n\t"
        "s_branch 9f\n"
        "10:\n\t"
        "s_waitcnt vmcnt(0)\n"
        "9:"
        ::"s"(n)
        : "scc", "memory");
}

// Band kernel for uniform 4:2:0 batches whose consecutive output rows share source rows (vertical
// upscales: C1). One wave owns one band of TH output rows of one 64·PX-column strip (lane l: the PX
// adjacent columns X0 + PX l ..), with no workgroup barrier after the prologue:
//  * every source row the band reads (luma rows r0(first) .. r1(last), and their chroma rows) is staged
//    once, in need order, by one LDS-DMA instruction per row segment at the start; output row i then
//    waits with one counted vmcnt for the rows it needs, so its arithmetic overlaps the later rows' DMA;
//  * horizontal results stay in registers per source row (HA: row pa, HB: row pb) and the BT.601 chroma
//    terms per chroma row, so a source row is converted and filtered once however many output rows read
//    it (~0.84 source rows per output row at 432 -> 512);
//  * coefficients of the strip's columns (per lane) and of the band's rows (one per lane, v_readlane)
//    come from the kernels' shared linear_coef: no table loads (the host's column table loaded at entry instead
//    was 1.5 % slower on C1: the per-pixel setup then waits for the load, profiles/r05t_c1_band_table_dd_ab.txt);
//  * DD (six-column lanes, band_six_columns): a lane's 4 pixels read 6 source columns and 3 chroma columns, so a
//    source row costs 6 luma and 18 saturating sums instead of 8 and 24, a chroma row 3 conversions instead of 8;
//  * each channel of a row leaves as one PX-wide store per lane.
// Workgroups of up to four waves: the strips of one band of one item.
// NHWC (interleaved u8 output, PX = 4): a lane's four pixels are 12 adjacent bytes of the slot, packed from the
// same sums into three dwords and stored as one 12-byte store per row (the host admits it where that store is
// dword-aligned: DW % 4 == 0 and a 4-byte-aligned tensor base).
template <int FMT, int OUT, int PX, int DD, bool NHWC = false>
__global__ __launch_bounds__(256) void evam_pp_band(const TParams P) {
    static_assert(!NHWC || (OUT == 0 && PX == 4), "the interleaved band store is u8 at four pixels per lane");
    constexpr int NS = NHWC ? 1 : 3;  // stores per output row
    __shared__ __attribute__((aligned(16))) float lut_s[OUT == 1 ? 768 : 4];
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (kAblate & 128) return;  // diagnostics: launch cost only
    static_assert(FMT == kNV12 || FMT == kI420, "4:2:0 sources");
    static_assert(PX == 1 || PX == 2 || PX == 4, "pixels per lane");
    static_assert(!DD || PX == 4, "six-column lanes hold 4 pixels");
    constexpr int NPC = FMT == kI420 ? 2 : 1;  // chroma planes
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    EVAM_WSTAMP(0);
    // grid (strip group, band, item): every kernel-argument load of the prologue has an address known at entry,
    // so they all go out in one batch (one round trip before the first DMA)
    const int item = blockIdx.z, band = blockIdx.y;
    const ItemArg& it = P.items[item];
    const ColSpan sf = P.sfoot[min((int)blockIdx.x * 8 + wave, kSfoot - 1)];
    const int p_nw = P.nw, p_TH = P.TH, p_DH = P.DH, p_DW = P.DW;
    int p_ns = P.nstrips, k_wb = P.wave_bytes;
    const uint8_t* p0 = it.plane[0];
    const uint8_t* p1 = it.plane[1];
    const uint8_t* p2 = it.plane[2];
    const int pitch0 = it.pitch[0], pitch1 = it.pitch[1], pitch2 = it.pitch[2];
    const int x0 = it.x0, y0 = it.y0;
    // The row table's and the LUT DMA's parameters join the batch as opaque values the compiler cannot reload
    // (loaded where first used, they were two more dependent kernel-argument round trips before the first DMA);
    // one statement, so every load goes out before the one wait (30 operands at most: the output's
    // parameters, first needed at the first store, are left out).
    double k_scale_y = P.scale_y;
    int k_ch = P.ch, k_rgb = P.color_rgb;
    const float* k_lut = P.lut;
    asm volatile("" : "+s"(k_scale_y), "+s"(k_ch), "+s"(k_lut), "+s"(k_rgb), "+s"(p_ns), "+s"(k_wb)
                 : "s"(p_nw), "s"(p_TH), "s"(p_DH), "s"(p_DW), "s"(P.ox), "s"(P.rw), "s"(P.oy), "s"(P.rh),
                   "s"(P.segY), "s"(P.segC), "s"(P.nrY), "s"(p0), "s"(p1), "s"(p2), "s"(pitch0),
                   "s"(pitch1), "s"(pitch2), "s"(x0), "s"(y0), "s"(it.index), "s"(sf.x), "s"(sf.y));
    const int strip = (int)blockIdx.x * p_nw + wave;
    const bool live = strip < p_ns;
    const int Y0 = band * p_TH, Y1 = min(Y0 + p_TH, p_DH);
    const int X0 = strip * 64 * PX;
    const bool cols = live && sf.x >= 0;
    int fsY = 0, nY = 0, fsC = 0, nC = 0;
    if (cols) footprint_chunks(FMT, 1, x0 + sf.x, x0 + sf.y, fsY, nY, fsC, nC);
    const int vr0 = max(Y0, P.oy), vr1 = min(Y1, P.oy + P.rh);
    const int n = cols && vr1 > vr0 ? vr1 - vr0 : 0;  // visible rows of the band (<= 64)

    // row table, one visible row per lane: source rows relative to the crop, weights << 8
    int lr0 = 0, lr1 = 0, lb0 = 0, lb1 = 0;
    if (lane < n) {
        int sy, b0, b1;
        linear_coef(vr0 + lane - P.oy, k_scale_y, k_ch, false, sy, b0, b1);
        lr0 = min(max(sy, 0), k_ch - 1);
        lr1 = min(max(sy + 1, 0), k_ch - 1);
        lb0 = b0 << 8;
        lb1 = b1 << 8;
    }
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsU = __builtin_amdgcn_make_buffer_rsrc((void*)p1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(NPC == 2 ? p2 : p1), (short)0, 0x7FFFFFFF, 0x00020000);
    uint8_t* const wbuf = smem + wave * k_wb;
    const int segY = P.segY, segC = P.segC;
    uint8_t* const cbuf = wbuf + P.nrY * segY;  // chroma rows; I420: V row k at + segC / 2 (segC holds U | V)
    // source rows of the band (rows are monotonic in the output row): luma [rlo, rhi], chroma [clo, chi]
    const int rlo = n ? __builtin_amdgcn_readlane(lr0, 0) : 0;
    const int rhi = n ? __builtin_amdgcn_readlane(lr1, n - 1) : -1;
    const int clo = (y0 + rlo) >> 1;
    // The wave counts every vector-memory operation it issues (pos) and remembers pos right after each luma row's
    // DMA (lane r - rlo of dpos), so every wait below is exact.
    int pos = 0, dpos = 0;
    // fp32: the LUT (3 KB, sections in source channel order) by LDS-DMA ahead of the rows, so no VGPR waits
    // on it and the rows' counted waits are unaffected (it is older)
    if constexpr (OUT == 1) {
        for (int c0 = wave * 64; c0 < 192; c0 += (int)(blockDim.x >> 6) * 64, pos++) {
            const int c = c0 + lane, sec = c >> 6;
            const int src = ((k_rgb ? 2 - sec : sec) * 64 + (c & 63)) * 16;
            const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc((void*)k_lut, (short)0, 3072, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsL, (__attribute__((address_space(3))) void*)((uint8_t*)lut_s + c0 * 16),
                                                     16, (uint32_t)src, 0, 0, 0);
        }
    }
    const int lut_pos = pos;
    // DMA in need order: luma row r, then its chroma row when r is the first row reading it. Rows go out up to
    // `ahead` source rows past the last row the current output row reads (EVAM_PP_BAND_AHEAD; 64: the whole band
    // at once), so a wave's first rows do not queue behind the rest of the band in the launch's opening burst.
    int rnext = rlo, cprev = -1;
    const int ahead = P.ahead;
    auto issue_to = [&](int rmax) {
        const uint32_t vo = (uint32_t)lane * 16u;
        for (; rnext <= rmax; rnext++) {
            const int r = rnext, ya = y0 + r, c = ya >> 1;
            if (lane < nY)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, (__attribute__((address_space(3))) void*)(wbuf + (r - rlo) * segY),
                                                         16, vo, ya * pitch0 + fsY, EVAM_PP_LOAD_AUX, 0);
            pos++;
            if (c != cprev) {
                uint8_t* cb = cbuf + (c - clo) * segC;
                if (lane < nC) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsU, (__attribute__((address_space(3))) void*)cb, 16, vo,
                                                             c * pitch1 + fsC, EVAM_PP_LOAD_AUX, 0);
                    if constexpr (NPC == 2)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (__attribute__((address_space(3))) void*)(cb + segC / 2),
                                                                 16, vo, c * pitch2 + fsC, EVAM_PP_LOAD_AUX, 0);
                }
                pos += NPC;
                cprev = c;
            }
            dpos = lane == r - rlo ? pos : dpos;
        }
    };
    if (n) issue_to(min(rhi, __builtin_amdgcn_readlane(lr1, 0) + ahead));
    EVAM_WSTAMP(1);
    EVAM_WTRACE_VAL(5, (unsigned long long)n << 48);

    if constexpr (OUT == 1) {
        vmcnt_le(pos - lut_pos);  // this wave's LUT pieces landed (issued before every row)
        lds_barrier();            // ... and every other wave's (LDS only: the rows' DMA stays in flight)
    }
    if (!live) return;

    // per-lane column state: tap offsets in the staged rows (tap 0 low, tap 1 high half), packed 11-bit
    // weights, padding columns
    const int X = X0 + lane * PX;
    const bool xin = X < p_DW;  // DW % PX == 0: a lane's pixels are all in or all out
    uint32_t lY[PX], lC[PX], wp[PX];
    bool padc[PX];
    bool anyp = false;
#pragma unroll
    for (int j = 0; j < PX; j++) {
        lY[j] = lC[j] = wp[j] = 0;
        padc[j] = true;
        const int dx = X + j - P.ox;
        if (cols && xin && dx >= 0 && dx < P.rw) {
            int s0, a0, a1;
            linear_coef(dx, P.scale_x, P.cw, true, s0, a0, a1);
            const int ca = x0 + s0, cb = x0 + min(s0 + 1, P.cw - 1);
            lY[j] = (uint32_t)(ca - fsY) | ((uint32_t)(cb - fsY) << 16);
            if constexpr (FMT == kNV12)
                lC[j] = (uint32_t)(2 * (ca >> 1) - fsC) | ((uint32_t)(2 * (cb >> 1) - fsC) << 16);
            else
                lC[j] = (uint32_t)((ca >> 1) - fsC) | ((uint32_t)((cb >> 1) - fsC) << 16);
            wp[j] = (uint32_t)a0 | ((uint32_t)a1 << 16);
            padc[j] = false;
        }
        anyp |= xin && padc[j];
    }
    const bool anypad = __builtin_amdgcn_ballot_w64(anyp) != 0;
    if (kAblate & 64) {  // diagnostics: prologue only (row / column coefficients, the first rows' DMA landed)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" ::"v"(lY[0]), "v"(lC[0]), "v"(wp[0]), "v"(lb0), "v"(lb1), "v"((int)anypad));
        return;
    }
    const size_t esz = OUT == 1 ? 4 : 1;
    const uint32_t vo = (uint32_t)(xin ? X : 0) * (uint32_t)(NHWC ? 3 * esz : esz);
    const size_t plane = (size_t)p_DW * p_DH;
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)(P.slot_offset + it.index * P.slot_stride) * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;
    // (NHWC: rsO0 is the whole slot)
    const __amdgpu_buffer_rsrc_t rsO0 = __builtin_amdgcn_make_buffer_rsrc((void*)(!NHWC && k_rgb ? d2 : d0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO1 = __builtin_amdgcn_make_buffer_rsrc((void*)d1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO2 = __builtin_amdgcn_make_buffer_rsrc((void*)(k_rgb ? d0 : d2), (short)0, 0x7FFFFFFF, 0x00020000);
    const uint32_t fq0 = P.fill & 0xFF, fq1 = (P.fill >> 8) & 0xFF, fq2 = (P.fill >> 16) & 0xFF;
    const uint32_t fsh = OUT == 1 ? 2 : 0;
    const uint32_t fill0 = (k_rgb ? fq2 : fq0) << fsh, fill1 = fq1 << fsh, fill2 = (k_rgb ? fq0 : fq2) << fsh;
    const uint8_t* lutb = reinterpret_cast<const uint8_t*>(lut_s);
    // one row of the strip: v[c][j] = LUT byte offsets (fp32) or bytes (u8) in source channel order; the
    // row offset in the VGPR offset (soffset 0: the store-data hazard of wide stores, see evam_pp_wave)
    // NHWC: the lane's 12 bytes of row Y from the sums x (byte = x >> 2), source channel order in, output order out
    auto put_nhwc = [&](int Y, const uint32_t (&x)[3][PX]) {
        if constexpr (NHWC) {
            if (!xin) return;
            uint32_t a[4], c[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                a[j] = k_rgb ? x[2][j] : x[0][j];
                c[j] = k_rgb ? x[0][j] : x[2][j];
            }
            const evam_v3i q = {(int)pack4_u8_sums(a[0], x[1][0], c[0], a[1]), (int)pack4_u8_sums(x[1][1], c[1], a[2], x[1][2]),
                                (int)pack4_u8_sums(c[2], a[3], x[1][3], c[3])};
            __builtin_amdgcn_raw_buffer_store_b96(q, rsO0, vo + (uint32_t)(Y * p_DW) * 3u, 0, EVAM_PP_STORE_AUX);
        }
    };
    auto put = [&](int Y, const uint32_t (&v)[3][PX]) {
        if (!xin) return;
        if constexpr (NHWC) {
            uint32_t x[3][PX];
#pragma unroll
            for (int j = 0; j < PX; j++)
#pragma unroll
                for (int c = 0; c < 3; c++) x[c][j] = v[c][j] << 2;
            put_nhwc(Y, x);
            return;
        }
        const uint32_t off = vo + (uint32_t)(Y * p_DW) * (uint32_t)esz;
        store_off<OUT, PX>(rsO0, off, lutb, v[0]);
        store_off<OUT, PX>(rsO1, off, lutb + 1024, v[1]);
        store_off<OUT, PX>(rsO2, off, lutb + 2048, v[2]);
    };
    auto put_fill = [&](int Y) {
        uint32_t v[3][PX];
#pragma unroll
        for (int j = 0; j < PX; j++) { v[0][j] = fill0; v[1][j] = fill1; v[2][j] = fill2; }
        put(Y, v);
    };
    for (int Y = Y0; Y < (n ? vr0 : Y1); Y++) {  // letterbox rows above
        put_fill(Y);
        pos += NS;
    }

    uint32_t kb = kKBs, kg = kKGs, kr = kKRs;
    int cvg = kCVG, cug = kCUG;
    asm volatile("" : "+v"(kb), "+v"(kg), "+v"(kr), "+s"(cvg), "+s"(cug));
    auto uvt = [&](uint32_t U, uint32_t V) {
        int gu = __mul24((int)U, cug) + (int)kg;
        asm("" : "+v"(gu));
        return UVs{__umul24(U, (uint32_t)kCUB) + kb, (uint32_t)(__mul24((int)V, cvg) + gu), __umul24(V, (uint32_t)kCVR) + kr};
    };
    // chroma terms of the chroma row cc for both taps of every pixel (kept across source rows)
    UVs tA[PX], tB[PX];
    int cc = -1;
    auto chroma_row = [&](int c) {
        const uint8_t* cb = cbuf + (c - clo) * segC;
        cc = c;
        if constexpr (DD) {  // the chroma columns of (c0, c1), (c2, c3), (c4, c5) in tA[0..2]
            const uint32_t o[3] = {lC[0] & 0xFFFF, lC[1] >> 16, lC[2] >> 16};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint8_t* a = cb + o[k];
                tA[k] = uvt(a[0], FMT == kNV12 ? a[1] : a[segC / 2]);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const uint8_t* a0 = cb + (lC[j] & 0xFFFF);
            const uint8_t* a1 = cb + (lC[j] >> 16);
            if constexpr (FMT == kNV12) {
                tA[j] = uvt(a0[0], a0[1]);
                tB[j] = uvt(a1[0], a1[1]);
            } else {
                tA[j] = uvt(a0[0], a0[segC / 2]);
                tB[j] = uvt(a1[0], a1[segC / 2]);
            }
        }
    };
    // A source row's 3 PX filtered values travel as 64-bit register pairs (value k of pixel j at flat index
    // 3 j + k), so the HA <- HB copy of a one-row step is one v_pk_mov_b32 per two values.
    constexpr int NH = (3 * PX + 1) / 2;
    struct HRow { uint64_t p[NH]; };
    auto hget = [](const HRow& h, int j, int k) -> uint32_t {
        const int f = 3 * j + k;
        return (uint32_t)(h.p[f >> 1] >> (32 * (f & 1)));
    };
    auto hpack = [](HRow& h, const uint32_t (&H)[PX][3]) {
#pragma unroll
        for (int i = 0; i < NH; i++) {
            const int f0 = 2 * i, f1 = 2 * i + 1;
            const uint32_t lo = H[f0 / 3][f0 % 3], hi = f1 < 3 * PX ? H[f1 / 3][f1 % 3] : 0u;
            h.p[i] = (uint64_t)lo | ((uint64_t)hi << 32);
        }
    };
    // horizontal pass of source row r (crop-relative) into HR
    auto hrow = [&](int r, HRow& HR) {
        uint32_t H[PX][3];
        const int c = (y0 + r) >> 1;
        if (c != cc) chroma_row(c);
        const uint8_t* yb = wbuf + (r - rlo) * segY;
        if constexpr (DD) {  // columns c0..c5: pixel 0 (c0, c1), 1 (c1, c2), 2 (c3, c4), 3 (c4, c5)
            const uint32_t yl[6] = {luma_term(yb[lY[0] & 0xFFFF]), luma_term(yb[lY[0] >> 16]), luma_term(yb[lY[1] >> 16]),
                                    luma_term(yb[lY[2] & 0xFFFF]), luma_term(yb[lY[2] >> 16]), luma_term(yb[lY[3] >> 16])};
#pragma unroll
            for (int ch3 = 0; ch3 < 3; ch3++) {
                uint32_t sm[6];
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const UVs& t = tA[k >> 1];
                    sm[k] = __builtin_elementwise_add_sat(yl[k], ch3 == 0 ? t.b : (ch3 == 1 ? t.g : t.r));
                }
                H[0][ch3] = hpass_sums(sm[0], sm[1], wp[0]) & kVMask;
                H[1][ch3] = hpass_sums(sm[1], sm[2], wp[1]) & kVMask;
                H[2][ch3] = hpass_sums(sm[3], sm[4], wp[2]) & kVMask;
                H[3][ch3] = hpass_sums(sm[4], sm[5], wp[3]) & kVMask;
            }
            hpack(HR, H);
            return;
        }
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const uint32_t yA = luma_term(yb[lY[j] & 0xFFFF]), yB = luma_term(yb[lY[j] >> 16]);
            // masked once per source row here rather than per output row in vfinal (each row serves ~2.4 output rows)
            H[j][0] = hpass_sat(yA, tA[j].b, yB, tB[j].b, wp[j]) & kVMask;
            H[j][1] = hpass_sat(yA, tA[j].g, yB, tB[j].g, wp[j]) & kVMask;
            H[j][2] = hpass_sat(yA, tA[j].r, yB, tB[j].r, wp[j]) & kVMask;
        }
        hpack(HR, H);
    };
    HRow HA, HB;
    int pa = -1, pb = -1;
    const int nst = NS;  // stores per output row (one PX-wide store per channel; NHWC: one for all three)
    // progress-based priority (EVAM_PP_PRIO), as in the strip kernel
    ProgressPrio prio(P.prio != 0, n);
    for (int i = 0; i < n; i++) {
        prio.step(i);
        const int ra = __builtin_amdgcn_readlane(lr0, i), rb = __builtin_amdgcn_readlane(lr1, i);
        issue_to(rb);  // (issued already unless `ahead` is 0)
        vmcnt_le(pos - __builtin_amdgcn_readlane(dpos, rb - rlo));  // rows up to rb landed
#ifdef EVAM_PP_TRACE
        if (i == 0) {
            EVAM_WSTAMP(2);
            EVAM_WSTAMP(3);
        }
#endif
        const uint32_t wb0 = (uint32_t)__builtin_amdgcn_readlane(lb0, i), wb1 = (uint32_t)__builtin_amdgcn_readlane(lb1, i);
        if (kAblate & 2) {  // diagnostics: no pixel math (no tap reads), stores and DMA kept
            put_fill(vr0 + i);
            pos += nst;
            asm volatile("" ::: "memory");
            if (i + 1 < n) issue_to(min(rhi, __builtin_amdgcn_readlane(lr1, i + 1) + ahead));
            asm volatile("" ::: "memory");
            continue;
        }
        // HA <- row ra, HB <- row rb, reusing what the previous output row filtered (wave-uniform branches)
        if (ra != pa) {
            if (ra == pb) {
                HA = HB;
            } else {
                hrow(ra, HA);
            }
        }
        if (rb == ra) {
            HB = HA;
        } else if (rb != pb || ra == pb) {  // HB was overwritten into HA above, or holds another row
            hrow(rb, HB);
        }
        pa = ra;
        pb = rb;
        uint32_t v[3][PX];
#pragma unroll
        for (int j = 0; j < PX; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) v[c][j] = vfinal_masked<OUT>(hget(HA, j, c), hget(HB, j, c), wb0, wb1);
        if constexpr (OUT == 0 && PX == 4) {  // u8, 4 pixels per lane: the sums packed by pack4_u8_sums
            uint32_t x[3][4];
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int c = 0; c < 3; c++) x[c][j] = mulhi_u24(wb0, hget(HA, j, c)) + mulhi_u24(wb1, hget(HB, j, c)) + 2u;
            if (anypad) {  // padding columns: the fill byte as a sum (x >> 2 == fill)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    x[0][j] = padc[j] ? fill0 << 2 : x[0][j];
                    x[1][j] = padc[j] ? fill1 << 2 : x[1][j];
                    x[2][j] = padc[j] ? fill2 << 2 : x[2][j];
                }
            }
            if constexpr (NHWC) {
                put_nhwc(vr0 + i, x);
            } else if (xin) {
                const uint32_t off = vo + (uint32_t)((vr0 + i) * p_DW);
                __builtin_amdgcn_raw_buffer_store_b32(pack4_u8_sums(x[0][0], x[0][1], x[0][2], x[0][3]), rsO0, off, 0,
                                                      EVAM_PP_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b32(pack4_u8_sums(x[1][0], x[1][1], x[1][2], x[1][3]), rsO1, off, 0,
                                                      EVAM_PP_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b32(pack4_u8_sums(x[2][0], x[2][1], x[2][2], x[2][3]), rsO2, off, 0,
                                                      EVAM_PP_STORE_AUX);
            }
            pos += nst;
            asm volatile("" ::: "memory");  // issue order is what the counted waits assume
            if (i + 1 < n) issue_to(min(rhi, __builtin_amdgcn_readlane(lr1, i + 1) + ahead));
            asm volatile("" ::: "memory");
            continue;
        }
        if (anypad) {
#pragma unroll
            for (int j = 0; j < PX; j++) {
                v[0][j] = padc[j] ? fill0 : v[0][j];
                v[1][j] = padc[j] ? fill1 : v[1][j];
                v[2][j] = padc[j] ? fill2 : v[2][j];
            }
        }
        put(vr0 + i, v);
        pos += nst;
        asm volatile("" ::: "memory");  // issue order is what the counted waits assume
        if (i + 1 < n) issue_to(min(rhi, __builtin_amdgcn_readlane(lr1, i + 1) + ahead));
        asm volatile("" ::: "memory");
    }
    for (int Y = max(n ? vr1 : Y1, Y0); Y < Y1; Y++) put_fill(Y);  // letterbox rows below
#ifdef EVAM_PP_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    EVAM_WSTAMP(4);
    {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        EVAM_WTRACE_VAL(6, (unsigned long long)xcc);
    }
#endif
}

}  // namespace
