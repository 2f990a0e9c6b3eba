// evam_pp_strip, the row-strip kernel (uniform 4:2:0 downscales), and vmcnt_exact, which only it uses.
// Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// strip kernel (uniform geometry, 4:2:0 sources, no shared source rows between output rows)
// ------------------------------------------------------------------------------------------------

// Wait until at most n (wave-uniform) vector-memory operations of this wave are outstanding, exact for n <= 24 (a jump
// over immediates; larger n waits for 24).
__device__ __forceinline__ void vmcnt_exact(int n) {
    n = __builtin_amdgcn_readfirstlane(n);
#define EVAM_VMC(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        EVAM_VMC(0) EVAM_VMC(1) EVAM_VMC(2) EVAM_VMC(3) EVAM_VMC(4) EVAM_VMC(5) EVAM_VMC(6) EVAM_VMC(7) EVAM_VMC(8)
        EVAM_VMC(9) EVAM_VMC(10) EVAM_VMC(11) EVAM_VMC(12) EVAM_VMC(13) EVAM_VMC(14) EVAM_VMC(15) EVAM_VMC(16)
        EVAM_VMC(17) EVAM_VMC(18) EVAM_VMC(19) EVAM_VMC(20) EVAM_VMC(21) EVAM_VMC(22) EVAM_VMC(23)
        default: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
    }
#undef EVAM_VMC
}

// Row-strip kernel for uniform-geometry 4:2:0 batches whose output rows do not share source rows
// (downscales: C2, C4, C5). Every wave owns one strip of 64 x PX output columns of a tile (lane l holds
// columns l, l + 64, ...) and walks the tile's rows alone, one output row per step, with no workgroup
// barrier after the prologue:
//  * a ring of D row entries per wave (two luma row segments, one or two chroma row segments: the strip's
//    16-byte-aligned footprint) fed by LDS-DMA D rows ahead; the wait for a row is one counted vmcnt,
//    so the ring's other rows and the stores of the previous rows stay in flight;
//  * the OpenCV coefficient tables of the strip's columns (per lane) and of the tile's rows (one per
//    lane, read back with v_readlane) are computed in the prologue by the kernels' shared linear_coef, so
//    the first DMA waits for no table load;
//  * per pixel: four luma taps and two chroma taps per chroma row from LDS, BT.601 as saturating two-tap
//    registers, the 11-bit horizontal pass as one v_dot2 per channel, VResizeLinear 32s->8u as mulhi_u24,
//    the LUT (fp32) and three planar stores (256 contiguous bytes per store instruction).
// Strip width: the C2 data movement alone takes 39.4 us in 64-column strips and 36.4 us in 128-column
// strips (one 480-byte DMA segment per source row instead of 240: half the DMA instructions for the same
// bytes), the copy floor of those bytes on the same box (profiles/r03c_strip_bw.txt).
// Letterbox rows are plain fill stores outside the ring; letterbox columns are a per-lane select in the
// strips that have any. D = ring depth (rows of DMA in flight).
// NHWC (interleaved fp32 output): a pixel's three values leave as one 12-byte store, so a store instruction covers
// 768 contiguous bytes of the row where the planar one covers 256 in each of three planes, and a row costs one
// store per pixel column group instead of three. (u8 would be 3-byte stores per lane: the wave kernel serves it.)
template <int FMT, int OUT, int D, int PX, int PR, bool NHWC = false>
__global__ __launch_bounds__(512) void evam_pp_strip(const TParams P) {
    static_assert(!NHWC || OUT == 1, "the interleaved strip store is fp32 only");
    constexpr int NS = NHWC ? 1 : 3;  // stores per pixel column group and row
    // the LUT at a static LDS address (folds into the reads' immediate offsets); the rings after it
    __shared__ __attribute__((aligned(16))) float lut_s[OUT != 0 ? 768 : 4];
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    static_assert(FMT == kNV12 || FMT == kI420 || FMT == kBGRX, "4:2:0 or BGRx sources");
    static_assert(D >= 1 && D <= 4, "ring depth");
    static_assert(PX == 1 || PX == 2, "pixels per lane");
    constexpr int SLOT = strip_slot(FMT, PX);
    constexpr bool PK = FMT == kBGRX;                 // packed BGRx: one plane, 4 bytes a pixel, no conversion
    constexpr int NPC = FMT == kI420 ? 2 : (PK ? 0 : 1);  // chroma planes
    // PR (paired taps): both source rows of a plane go out in ONE LDS-DMA instruction, lanes 0-31 the first
    // row's chunks and lanes 32-63 the second's (I420: U tap0 / U tap1 / V tap0 / V tap1 in lane quarters), so
    // every row costs exactly NI instructions. Without PR a row costs 2 + NPC (chroma row shared) or 2 + 2 NPC.
    static_assert(PR == 0 || PR == 1, "paired taps");
    constexpr int NMIN = PR ? (PK ? 1 : 2) : 2 + NPC;  // fewest DMA instructions of one row (PR: exact)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (kAblate & 128) return;  // diagnostics: launch cost only
    EVAM_WSTAMP(0);
    const uint8_t *p0, *p1, *p2;
    int pitch0, pitch1, pitch2, x0, y0, index, p_nw, p_DH, p_DW, strip, Y0, Y1;
    int g_ox, g_rw, g_oy, g_rh, g_cw, k_ch, k_rgb;
    double k_scale_x, k_scale_y;
    const float* k_lut;
    ColSpan sf;
    // grid (tile column, tile row, item): every kernel-argument load of the prologue has an address known at
    // entry, so they all go out in one batch (one round trip before the first DMA)
    const int item = blockIdx.z, ty = blockIdx.y;
    const ItemArg& it = P.items[item];
    sf = P.sfoot[min((int)blockIdx.x * 8 + wave, kSfoot - 1)];
    const int p_TH = P.TH;
    p_nw = P.nw; p_DH = P.DH; p_DW = P.DW;
    p0 = it.plane[0];
    p1 = it.plane[1];
    p2 = it.plane[2];
    pitch0 = it.pitch[0]; pitch1 = it.pitch[1]; pitch2 = it.pitch[2];
    x0 = it.x0; y0 = it.y0;
    index = it.index;
    asm volatile("" ::"s"(p_nw), "s"(p_TH), "s"(p_DH), "s"(p_DW), "s"(P.ox), "s"(P.rw), "s"(P.oy), "s"(P.rh),
                 "s"(P.wave_bytes), "s"(p0), "s"(p1), "s"(p2), "s"(pitch0), "s"(pitch1), "s"(pitch2), "s"(x0), "s"(y0),
                 "s"(index), "s"(sf.x), "s"(sf.y), "s"(P.dst), "s"(P.slot_offset), "s"(P.slot_stride));
    // the row table's and the LUT DMA's parameters in the same batch, as opaque values the compiler cannot
    // reload: loaded where first used, they were one or two more dependent kernel-argument round trips before
    // the first DMA
    k_scale_y = P.scale_y;
    k_ch = P.ch; k_rgb = P.color_rgb;
    k_lut = P.lut;
    asm volatile("" : "+s"(k_scale_y), "+s"(k_ch), "+s"(k_lut), "+s"(k_rgb));
    strip = (int)blockIdx.x * p_nw + wave;
    Y0 = ty * p_TH; Y1 = min(Y0 + p_TH, p_DH);
    g_ox = P.ox; g_rw = P.rw; g_oy = P.oy; g_rh = P.rh; g_cw = P.cw;
    k_scale_x = P.scale_x;
    const int X0 = strip * 64 * PX;
    const bool live = X0 < p_DW;  // a wave past the last strip only joins the LUT barrier
    const bool cols = live && sf.x >= 0;
    int fsY = 0, nY = 0, fsC = 0, nC = 0;
    if (cols) footprint_chunks(FMT, PK ? 4 : 1, x0 + sf.x, x0 + sf.y, fsY, nY, fsC, nC);
    // visible output rows of the tile (the rest are letterbox fill)
    const int vr0 = max(Y0, g_oy), vr1 = min(Y1, g_oy + g_rh);
    const int n = cols && vr1 > vr0 ? vr1 - vr0 : 0;

    // row table, one visible row per lane: source rows relative to the crop, weights << 8
    int lr0 = 0, lr1 = 0, lb0 = 0, lb1 = 0;
    if (lane < n) {
        int sy, b0, b1;
        linear_coef(vr0 + lane - g_oy, k_scale_y, k_ch, false, sy, b0, b1);
        lr0 = min(max(sy, 0), k_ch - 1);
        lr1 = min(max(sy + 1, 0), k_ch - 1);
        lb0 = b0 << 8;
        lb1 = b1 << 8;
    }
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsU = __builtin_amdgcn_make_buffer_rsrc((void*)p1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(NPC == 2 ? p2 : p1), (short)0, 0x7FFFFFFF, 0x00020000);
    uint8_t* const wbuf = smem + wave * P.wave_bytes;
    // Ring entry layout. Without PR: [Y tap0][Y tap1][C tap0][C tap1] (+ [V tap0][V tap1] for I420), SLOT bytes
    // each; BGRx: [row tap0][row tap1]. With PR: [Y tap0 | Y tap1] (512 B halves) then, for 4:2:0,
    // [C tap0 | C tap1] (NV12, 512 B halves) or [U tap0 | U tap1 | V tap0 | V tap1] (I420, 256 B quarters).
    //   SY: Y tap1 - Y tap0; CB: chroma region; SC: C tap1 - C tap0; SV: I420 V tap0 - U tap0.
    constexpr int SY = PR ? 512 : SLOT;
    constexpr int CB = PR ? 1024 : 2 * SLOT;
    constexpr int SC = PR ? (NPC == 2 ? 256 : 512) : SLOT;
    constexpr int SV = PR ? 512 : 2 * SLOT;
    constexpr int GRP = PR ? (PK ? 1024 : 2048) : 2 * SLOT + 2 * NPC * SLOT;
    constexpr int segY = SY;
    // I420 with PR: one buffer resource over both chroma planes, based at the lower one. Every byte read lies below
    // (offset of the upper plane) + (its extent), which must stay under num_records 0x7FFFFFFF: the host admits the
    // pairing only when that holds for every item of the launch, else the group runs unpaired
    const uint8_t* const pcl = NPC == 2 && PR ? (p1 < p2 ? p1 : p2) : p1;
    const uint32_t dU = (uint32_t)(p1 - pcl), dV = (uint32_t)(p2 - pcl);
    const __amdgpu_buffer_rsrc_t rsC2 = __builtin_amdgcn_make_buffer_rsrc((void*)pcl, (short)0, 0x7FFFFFFF, 0x00020000);
    auto issue = [&](int i, int k) {
        if (kAblate & 16) return;  // diagnostics: no DMA
        const int ya = y0 + __builtin_amdgcn_readlane(lr0, i), yb = y0 + __builtin_amdgcn_readlane(lr1, i);
        uint8_t* e = wbuf + k * GRP;
        if constexpr (PR) {
            const int hi = lane >> 5, c = lane & 31;
            if (c < nY)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, (__attribute__((address_space(3))) void*)e, 16,
                                                         (uint32_t)((hi ? yb : ya) * pitch0 + fsY + c * 16), 0,
                                                         EVAM_PP_LOAD_AUX, 0);
            if constexpr (NPC == 1) {
                const int ca = ya >> 1, cb = yb >> 1;
                if (c < nC && (!hi || ca != cb))
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsU, (__attribute__((address_space(3))) void*)(e + CB), 16,
                                                             (uint32_t)((hi ? cb : ca) * pitch1 + fsC + c * 16), 0,
                                                             EVAM_PP_LOAD_AUX, 0);
            } else if constexpr (NPC == 2) {
                const int ca = ya >> 1, cb = yb >> 1, q = lane >> 4, c4 = lane & 15, r = (q & 1) ? cb : ca;
                const uint32_t off = (q & 2) ? dV + (uint32_t)(r * pitch2) : dU + (uint32_t)(r * pitch1);
                if (c4 < nC && (!(q & 1) || ca != cb))
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsC2, (__attribute__((address_space(3))) void*)(e + CB), 16,
                                                             off + (uint32_t)(fsC + c4 * 16), 0, EVAM_PP_LOAD_AUX, 0);
            }
            return;
        }
        const uint32_t vo = (uint32_t)lane * 16u;
        if (lane < nY) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, (__attribute__((address_space(3))) void*)e, 16, vo,
                                                     ya * pitch0 + fsY, EVAM_PP_LOAD_AUX, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, (__attribute__((address_space(3))) void*)(e + segY), 16, vo,
                                                     yb * pitch0 + fsY, EVAM_PP_LOAD_AUX, 0);
        }
        if constexpr (NPC == 0) return;
        const int ca = ya >> 1, cb = yb >> 1;
        if (lane < nC) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsU, (__attribute__((address_space(3))) void*)(e + CB), 16, vo,
                                                     ca * pitch1 + fsC, EVAM_PP_LOAD_AUX, 0);
            if constexpr (NPC == 2)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (__attribute__((address_space(3))) void*)(e + CB + SV),
                                                         16, vo, ca * pitch2 + fsC, EVAM_PP_LOAD_AUX, 0);
        }
        if (ca != cb && lane < nC) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsU, (__attribute__((address_space(3))) void*)(e + CB + SC), 16,
                                                     vo, cb * pitch1 + fsC, EVAM_PP_LOAD_AUX, 0);
            if constexpr (NPC == 2)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (__attribute__((address_space(3))) void*)(e + CB + SV + SC),
                                                         16, vo, cb * pitch2 + fsC, EVAM_PP_LOAD_AUX, 0);
        }
    };

    // The LUT first (oldest VMEM: the first row's wait covers it), then the ring's first D rows. With four or
    // more waves, waves 0-2 each bring one 1 KB section by LDS-DMA (source section swapped for RGB): no ds_write
    // follows the ring's DMA, so nothing makes the compiler drain the ring before the LUT barrier.
    const int nthr = p_nw * 64;
    const bool lut_early = nthr >= 256;
    if constexpr (OUT != 0) {
        if (lut_early && wave < 3) {
            const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc((void*)k_lut, (short)0, 3072, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsL, (__attribute__((address_space(3))) void*)(lut_s + wave * 256), 16,
                                                     (uint32_t)lane * 16u, (k_rgb ? 2 - wave : wave) * 1024, 0, 0);
        }
    }
    const int npro = min(n, D);
    for (int i = 0; i < npro; i++) issue(i, i);
    EVAM_WSTAMP(1);
    EVAM_WTRACE_VAL(5, (unsigned long long)blockIdx.z | ((unsigned long long)strip << 16) |
                           ((unsigned long long)blockIdx.y << 32) | ((unsigned long long)n << 48));

    // per-lane column state of the lane's PX pixels: tap offsets inside the staged segments, packed
    // 11-bit weights, store offsets
    bool xin[PX], padc[PX];
    uint32_t lY[PX], lC0[PX], lC1[PX], wp[PX], vo[PX];
    bool anyp = false;
    const size_t esz = out_esz(OUT);
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const int X = X0 + lane + 64 * j;
        xin[j] = live && X < p_DW;
        vo[j] = (uint32_t)(xin[j] ? X : 0) * (uint32_t)(NHWC ? 3 * esz : esz);
        lY[j] = lC0[j] = lC1[j] = wp[j] = 0;
        padc[j] = true;
        const int dx = X - g_ox;
        if (cols && xin[j] && dx >= 0 && dx < g_rw) {
            int s0, a0, a1;
            linear_coef(dx, k_scale_x, g_cw, true, s0, a0, a1);
            const int ca = x0 + s0;  // tap 1 reads ca + 1: at the right edge (s0 = cw - 1) its weight a1 is 0
            lY[j] = (uint32_t)(ca * (PK ? 4 : 1) - fsY);
            if constexpr (FMT == kNV12) {
                lC0[j] = (uint32_t)(2 * (ca >> 1) - fsC);
                lC1[j] = (uint32_t)(2 * ((ca + 1) >> 1) - fsC);
            } else if constexpr (FMT == kI420) {
                lC0[j] = (uint32_t)((ca >> 1) - fsC);
                lC1[j] = (uint32_t)(((ca + 1) >> 1) - fsC);
            }
            // BGRx: the weights carry the 16x that the 4:2:0 path's saturating clamp leaves on its taps
            wp[j] = PK ? ((uint32_t)a0 << 4) | ((uint32_t)a1 << 20) : (uint32_t)a0 | ((uint32_t)a1 << 16);
            padc[j] = false;
        }
        anyp |= xin[j] && padc[j];
    }
    // some visible lane shows letterbox columns (wave-uniform): only then the per-pixel fill select
    const bool anypad = cols && __builtin_amdgcn_ballot_w64(anyp) != 0;
    // stores per row of this wave: 3 per pixel column group with any lane inside the output (counted waits)
    const bool full = X0 + 64 * (PX - 1) < p_DW;

    const size_t plane = (size_t)p_DW * p_DH;
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)(P.slot_offset + index * P.slot_stride) * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;
    // output planes in source channel order (B, G, R): planes 0 and 2 exchanged for RGB; NHWC: rsO0 is the whole slot
    const __amdgpu_buffer_rsrc_t rsO0 = __builtin_amdgcn_make_buffer_rsrc((void*)(!NHWC && k_rgb ? d2 : d0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO1 = __builtin_amdgcn_make_buffer_rsrc((void*)d1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO2 = __builtin_amdgcn_make_buffer_rsrc((void*)(k_rgb ? d0 : d2), (short)0, 0x7FFFFFFF, 0x00020000);
    // fill in source channel order (P.fill is in output plane order)
    const uint32_t fq0 = P.fill & 0xFF, fq1 = (P.fill >> 8) & 0xFF, fq2 = (P.fill >> 16) & 0xFF;
    const uint32_t fsh = OUT != 0 ? 2 : 0;
    const uint32_t fill0 = (k_rgb ? fq2 : fq0) << fsh, fill1 = fq1 << fsh, fill2 = (k_rgb ? fq0 : fq2) << fsh;

    if constexpr (OUT != 0) {
        if (lut_early) {
            // this wave's LUT section landed once at most the ring's DMA instructions are outstanding; the
            // barrier then needs no vmcnt(0): each wave waits for its own ring rows in the loop
            if (npro == D) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NMIN * D) : "memory");
            else vmcnt_exact(NMIN * npro);
            lds_barrier();
        } else {  // workgroups of 1-3 waves (outputs narrower than 64 x PX x 3 + 1 columns)
            for (int idx = threadIdx.x; idx < 768; idx += nthr)
                lut_s[idx] = k_lut[k_rgb ? 512 - (idx & ~255) + (idx & 255) : idx];
            __syncthreads();
        }
    }
    EVAM_WSTAMP(2);
    if (!live) return;
    if (kAblate & 64) {  // diagnostics: prologue only (tables, LUT, the ring's first DMA)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" ::"v"(lY[0]), "v"(lC0[0]), "v"(lC1[0]), "v"(wp[0]), "v"(vo[0]), "v"(lb0), "v"(lb1));
        return;
    }
    const uint8_t* lutb = reinterpret_cast<const uint8_t*>(lut_s);
    // per-lane LDS addresses of the taps in ring entry 0 (entry k adds k * GRP, an immediate offset)
    const uint8_t* aY[PX];
    const uint8_t* aC0[PX];
    const uint8_t* aC1[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) {
        aY[j] = wbuf + lY[j];
        aC0[j] = wbuf + CB + lC0[j];
        aC1[j] = wbuf + CB + lC1[j];
    }
    // BT.601 chroma-term constants: the additive ones in VGPRs so every term is one v_mad (a VOP3 reads one
    // scalar operand: the multiplier)
    uint32_t kb = kKBs, kg = kKGs, kr = kKRs;
    int cvg = kCVG, cug = kCUG;
    asm volatile("" : "+v"(kb), "+v"(kg), "+v"(kr), "+s"(cvg), "+s"(cug));
    auto uvt = [&](uint32_t U, uint32_t V) {
        // g = V * CVG + (U * CUG + K): two v_mad_i32_i24 (the sum of two products would select mul, mul, add3)
        int gu = __mul24((int)U, cug) + (int)kg;
        asm("" : "+v"(gu));  // keeps the association (no asm volatile: still scheduled freely)
        return UVs{__umul24(U, (uint32_t)kCUB) + kb, (uint32_t)(__mul24((int)V, cvg) + gu), __umul24(V, (uint32_t)kCVR) + kr};
    };
    // pixel column group j of row Y; v: LUT byte offsets (fp32) or bytes (u8), source channel order
    auto put = [&](int Y, int j, uint32_t v0, uint32_t v1, uint32_t v2) {
        if (!xin[j]) return;
        if (kAblate & 4) {  // diagnostics: no stores
            asm volatile("" ::"v"(v0), "v"(v1), "v"(v2));
            return;
        }
        if constexpr (NHWC) {
            // the LUT sections are in source channel order (loaded swapped for RGB), the store in output order; the
            // row offset goes in the VGPR offset (soffset 0: the store-data hazard of wide stores, see evam_pp_wave)
            const int l0 = (int)*reinterpret_cast<const uint32_t*>(lutb + v0);
            const int l1 = (int)*reinterpret_cast<const uint32_t*>(lutb + 1024 + v1);
            const int l2 = (int)*reinterpret_cast<const uint32_t*>(lutb + 2048 + v2);
            const evam_v3i q = {k_rgb ? l2 : l0, l1, k_rgb ? l0 : l2};
            __builtin_amdgcn_raw_buffer_store_b96(q, rsO0, vo[j] + (uint32_t)(Y * p_DW) * 12u, 0, EVAM_PP_STORE_AUX);
            return;
        }
        const int so = (int)((uint32_t)(Y * p_DW) * (uint32_t)esz);
        if constexpr (OUT == 1) {
            __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t*>(lutb + v0), rsO0, vo[j], so, EVAM_PP_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t*>(lutb + 1024 + v1), rsO1, vo[j], so, EVAM_PP_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t*>(lutb + 2048 + v2), rsO2, vo[j], so, EVAM_PP_STORE_AUX);
        } else if constexpr (OUT == 2) {
            // the low u16 of the entry: lane l holds columns l, l + 64, so a store instruction covers 128 contiguous bytes
            __builtin_amdgcn_raw_buffer_store_b16(*reinterpret_cast<const uint16_t*>(lutb + v0), rsO0, vo[j], so, EVAM_PP_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b16(*reinterpret_cast<const uint16_t*>(lutb + 1024 + v1), rsO1, vo[j], so, EVAM_PP_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b16(*reinterpret_cast<const uint16_t*>(lutb + 2048 + v2), rsO2, vo[j], so, EVAM_PP_STORE_AUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v0, rsO0, vo[j], so, EVAM_PP_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v1, rsO1, vo[j], so, EVAM_PP_STORE_AUX);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v2, rsO2, vo[j], so, EVAM_PP_STORE_AUX);
        }
    };
    auto put_fill = [&](int Y) {
#pragma unroll
        for (int j = 0; j < PX; j++) put(Y, j, fill0, fill1, fill2);
    };
    // letterbox rows above the ring: before its DMA in issue order, so they never enter the counted waits
    const int ra = n ? vr0 : Y1;
    for (int Y = Y0; Y < ra; Y++) put_fill(Y);

    // Progress-based priority (EVAM_PP_PRIO): waves of a SIMD otherwise share issue by age, so the youngest
    // workgroups' waves lag and end the launch alone; a wave lowers its priority as it passes each quarter of its
    // rows, so the ones behind get the issue slots when several are ready.
    ProgressPrio prio(P.prio != 0, n);
    const int nst = full ? NS * PX : NS;
    // one output row: row i of the tile's visible rows, ring entry kk (compile-time after unrolling)
    auto row = [&](int i, int kk, auto has_pad) {
        constexpr bool PADC = decltype(has_pad)::value;
        // row i's DMA landed. Issued after it: the DMA of rows i+1 .. i+D-1 (>= NMIN each) and the stores
        // of rows i-D+1 .. i-1 (nst each)
        constexpr int SD = D - 1;
        if (SD == 0) {  // nothing was issued after row i's DMA
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (i >= SD && i + D - 1 < n) {
            if (PX == 1 || !full) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * NMIN + SD * NS) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * NMIN + SD * NS * PX) : "memory");
        } else {
            vmcnt_exact(NMIN * (min(i + D - 1, n - 1) - i) + nst * min(i, SD));
        }
#ifdef EVAM_PP_TRACE
        if (i == 0) EVAM_WSTAMP(3);
#endif
        prio.step(i);
        const int Y = vr0 + i;
        const uint32_t wb0 = (uint32_t)__builtin_amdgcn_readlane(lb0, i), wb1 = (uint32_t)__builtin_amdgcn_readlane(lb1, i);
        const int ya = __builtin_amdgcn_readlane(lr0, i), yb = __builtin_amdgcn_readlane(lr1, i);
        const bool share = ((y0 + ya) >> 1) == ((y0 + yb) >> 1);
        if (kAblate & 2) {  // diagnostics: no pixel math (no tap reads)
            put_fill(Y);
        } else if constexpr (PK) {
            // BGRx: both taps of a source row are two adjacent dwords; channel c of the pair is one v_perm into
            // two u16 halves, and the horizontal pass one v_dot2 with the 16x weights
            const int eo = kk * GRP;
#pragma unroll
            for (int j = 0; j < PX; j++) {
                const uint32_t* ay = reinterpret_cast<const uint32_t*>(aY[j] + eo);
                const uint32_t qa0 = ay[0], qa1 = ay[1], qb0 = ay[SY / 4], qb1 = ay[SY / 4 + 1];
                uint32_t v[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const uint32_t sel = 0x0C000C00u | ((uint32_t)(4 + c) << 16) | (uint32_t)c;
                    const uint32_t ha = __builtin_amdgcn_udot2(
                        __builtin_bit_cast(evam_u16x2, __builtin_amdgcn_perm(qa1, qa0, sel)),
                        __builtin_bit_cast(evam_u16x2, wp[j]), 0u, false);
                    const uint32_t hb = __builtin_amdgcn_udot2(
                        __builtin_bit_cast(evam_u16x2, __builtin_amdgcn_perm(qb1, qb0, sel)),
                        __builtin_bit_cast(evam_u16x2, wp[j]), 0u, false);
                    v[c] = vfinal<OUT>(ha, hb, wb0, wb1);
                }
                if constexpr (PADC) {
                    v[0] = padc[j] ? fill0 : v[0];
                    v[1] = padc[j] ? fill1 : v[1];
                    v[2] = padc[j] ? fill2 : v[2];
                }
                put(Y, j, v[0], v[1], v[2]);
            }
        } else {
            const int eo = kk * GRP;  // this entry's offset from entry 0
            // raw taps of the entry into registers: luma bytes of both source rows, chroma of the first
            // chroma row and, when the second source row has its own, of the second
            uint32_t rY[PX][4], rC[PX][2][2], rE[PX][2][2];
            auto raw_c = [&](const uint8_t* a, int o, uint32_t (&c)[2]) {
                c[0] = a[o];
                c[1] = FMT == kNV12 ? a[o + 1] : a[o + SV];  // NV12: interleaved UV; I420: the V slot
            };
#pragma unroll
            for (int j = 0; j < PX; j++) {
                const uint8_t* ay = aY[j] + eo;
                rY[j][0] = ay[0]; rY[j][1] = ay[1]; rY[j][2] = ay[SY]; rY[j][3] = ay[SY + 1];
                raw_c(aC0[j], eo, rC[j][0]);
                raw_c(aC1[j], eo, rC[j][1]);
            }
            if (!share) {
#pragma unroll
                for (int j = 0; j < PX; j++) {
                    raw_c(aC0[j], eo + SC, rE[j][0]);
                    raw_c(aC1[j], eo + SC, rE[j][1]);
                }
            }
#pragma unroll
            for (int j = 0; j < PX; j++) {
                const UVs tA = uvt(rC[j][0][0], rC[j][0][1]), tB = uvt(rC[j][1][0], rC[j][1][1]);
                const uint32_t yA = luma_term(rY[j][0]), yB = luma_term(rY[j][1]);
                const uint32_t yC = luma_term(rY[j][2]), yD = luma_term(rY[j][3]);
                uint32_t h0[3], h1[3];
                h0[0] = hpass_sat(yA, tA.b, yB, tB.b, wp[j]);
                h0[1] = hpass_sat(yA, tA.g, yB, tB.g, wp[j]);
                h0[2] = hpass_sat(yA, tA.r, yB, tB.r, wp[j]);
                if (share) {  // both vertical taps in one chroma row: its terms serve both source rows
                    h1[0] = hpass_sat(yC, tA.b, yD, tB.b, wp[j]);
                    h1[1] = hpass_sat(yC, tA.g, yD, tB.g, wp[j]);
                    h1[2] = hpass_sat(yC, tA.r, yD, tB.r, wp[j]);
                    // distinct markers end the two branches, so the compiler does not merge their common
                    // tail behind register copies of the chroma terms
                    asm volatile("; strip: shared chroma row" ::"v"(h1[0]), "v"(h1[1]), "v"(h1[2]));
                } else {
                    const UVs tC = uvt(rE[j][0][0], rE[j][0][1]), tE = uvt(rE[j][1][0], rE[j][1][1]);
                    h1[0] = hpass_sat(yC, tC.b, yD, tE.b, wp[j]);
                    h1[1] = hpass_sat(yC, tC.g, yD, tE.g, wp[j]);
                    h1[2] = hpass_sat(yC, tC.r, yD, tE.r, wp[j]);
                    asm volatile("; strip: two chroma rows" ::"v"(h1[0]), "v"(h1[1]), "v"(h1[2]));
                }
                uint32_t v[3];
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = vfinal<OUT>(h0[c], h1[c], wb0, wb1);
                if constexpr (PADC) {
                    v[0] = padc[j] ? fill0 : v[0];
                    v[1] = padc[j] ? fill1 : v[1];
                    v[2] = padc[j] ? fill2 : v[2];
                }
                put(Y, j, v[0], v[1], v[2]);
            }
        }
        asm volatile("" ::: "memory");  // issue order is what the counted waits assume
        if (i + D < n) issue(i + D, kk);  // this entry's reads are done: the stores consumed them
        asm volatile("" ::: "memory");
    };
    auto ring = [&](auto has_pad) {
        for (int i0 = 0; i0 < n; i0 += D) {
#pragma unroll
            for (int kk = 0; kk < D; kk++)
                if (i0 + kk < n) row(i0 + kk, kk, has_pad);
        }
    };
    if (anypad) ring(std::true_type{});
    else ring(std::false_type{});
    // letterbox rows below the ring
    for (int Y = max(ra, vr1); Y < Y1; Y++) put_fill(Y);
#ifdef EVAM_PP_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last stores retired
    EVAM_WSTAMP(4);
    {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        EVAM_WTRACE_VAL(6, (unsigned long long)xcc);
    }
#endif
}

}  // namespace
