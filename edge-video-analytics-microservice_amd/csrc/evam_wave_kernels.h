// evam_pp_wave, the wave-row kernel (uniform geometry, independent waves), and store_vec, which only it uses. Source
// bytes: each wave stages the row segments of its next output row into its own LDS area by LDS-DMA while it converts
// the current one. LDS: the LUT, then per wave two buffers of [Y tap0][Y tap1][C tap0][C tap1][V tap0][V tap1]. Waits:
// per wave, vmcnt(3) (the previous row's stores stay in flight; vmcnt(1) for u8 NHWC); no barrier in the loop.
// Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// wave-row kernel (uniform geometry)
// ------------------------------------------------------------------------------------------------

// PX adjacent output pixels of one channel from one lane: a single buffer store of PX x 4 bytes (fp32),
// PX x 2 bytes (fp16 / bf16) or PX bytes (u8). lut == nullptr: u8 output.
template <int OUT, int PX>
__device__ __forceinline__ void store_vec(const __amdgpu_buffer_rsrc_t rs, uint32_t vo, int so, const float* lut,
                                          const int (&v)[PX]) {
    if constexpr (OUT == 1) {
        if constexpr (PX == 4) {
            evam_v4i q = {(int)__float_as_uint(lut[v[0]]), (int)__float_as_uint(lut[v[1]]),
                          (int)__float_as_uint(lut[v[2]]), (int)__float_as_uint(lut[v[3]])};
            __builtin_amdgcn_raw_buffer_store_b128(q, rs, vo, so, EVAM_PP_STORE_AUX);
        } else if constexpr (PX == 2) {
            evam_v2i q = {(int)__float_as_uint(lut[v[0]]), (int)__float_as_uint(lut[v[1]])};
            __builtin_amdgcn_raw_buffer_store_b64(q, rs, vo, so, EVAM_PP_STORE_AUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lut[v[0]]), rs, vo, so, EVAM_PP_STORE_AUX);
        }
    } else if constexpr (OUT == 2) {
        // 2-byte elements: two table reads packed per dword (no conversion), one store of 2 PX bytes; the address is
        // only 2-byte aligned (odd widths, odd slots), as the u8 path's dword stores are only byte aligned
        auto P2 = [&](int a, int b) { return (int)((uint32_t)lut_u16(lut, a) | ((uint32_t)lut_u16(lut, b) << 16)); };
        if constexpr (PX == 4) {
            evam_v2i q = {P2(v[0], v[1]), P2(v[2], v[3])};
            __builtin_amdgcn_raw_buffer_store_b64(q, rs, vo, so, EVAM_PP_STORE_AUX);
        } else if constexpr (PX == 2) {
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)P2(v[0], v[1]), rs, vo, so, EVAM_PP_STORE_AUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b16(lut_u16(lut, v[0]), rs, vo, so, EVAM_PP_STORE_AUX);
        }
    } else {
        if constexpr (PX == 4)
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) |
                                                      ((uint32_t)v[3] << 24), rs, vo, so, EVAM_PP_STORE_AUX);
        else if constexpr (PX == 2)
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(v[0] | (v[1] << 8)), rs, vo, so, EVAM_PP_STORE_AUX);
        else
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[0], rs, vo, so, EVAM_PP_STORE_AUX);
    }
}

// Uniform-geometry kernel built around independent waves. A workgroup owns a 64·PX-column x TH-row
// tile of one item; each of its four waves owns a contiguous quarter of the tile's rows and walks it
// one output row at a time, every lane producing PX adjacent pixels:
//  * The wave stages the source row segments its next row needs (luma taps, chroma taps; each the
//    tile's 16 B-aligned footprint) into its own double-buffered LDS area by LDS-DMA while it converts
//    the current row. Nothing is shared between waves, so there is no workgroup barrier in the loop:
//    the wait for a row's DMA is this wave's vmcnt, with the previous row's three stores still in flight.
//  * Horizontal results are kept per source row (H = 11-bit weighted sum of the two converted taps, per
//    channel). With REUSE (vertical upscales, where consecutive output rows share source rows) a source
//    row that the previous output row already filtered is neither staged nor converted again.
//  * When both vertical taps read the same 4:2:0 chroma row, its BT.601 chroma terms are computed once.
//  * Each channel of a row leaves as one PX-wide store per lane (dwordx4 for fp32 at PX = 4).
//  * NHWC (interleaved output, PX = 4): a lane's four pixels are 12 adjacent elements of the slot, so a row leaves as
//    one 12-byte store per lane (u8) or three 16-byte stores (fp32) that cover 3 KB contiguous per wave. The host
//    takes this variant only where every such store is aligned to its width: DW % 4 == 0 makes every row and slot
//    size a multiple of it, so the tensor's base address decides (4 bytes for u8, 16 for fp32).
template <int FMT, int OUT, int PX, bool REUSE, bool NHWC = false>
__global__ __launch_bounds__(kThreads) void evam_pp_wave(const WParams P) {
    static_assert(!NHWC || PX == 4, "the interleaved store is written for four pixels per lane");
    static_assert(!NHWC || OUT != 2, "interleaved 2-byte output is served by the generic kernel");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using T = FmtTraits<FMT>;
    constexpr bool kYUV = FMT == kNV12 || FMT == kI420;
    constexpr int TW = 64 * PX;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.x;
    // the launch parameters of the prologue in one batch of scalar loads (one wait): without the empty
    // asm use, branches split them into dependent round trips ahead of the first DMA
    asm volatile("" ::"s"(P.tiles_per_item), "s"(P.tiles_x), "s"(P.ytab), "s"(P.xtab), "s"(P.TH),
                 "s"(P.DH), "s"(P.DW), "s"(P.ox), "s"(P.rw));
    const int item = t / P.tiles_per_item;
    const int tile = t - item * P.tiles_per_item;
    const int ty = tile / P.tiles_x;
    const int tx = tile - ty * P.tiles_x;
    const ItemArg& it = P.items[item];
    const __attribute__((address_space(4))) XTab* xtab_s = (const __attribute__((address_space(4))) XTab*)(P.xtab);
    const uint8_t* p0 = it.plane[0];
    const uint8_t* p1 = it.plane[1];
    const uint8_t* p2 = it.plane[2];
    const int pitch0 = it.pitch[0], pitch1 = it.pitch[1], pitch2 = it.pitch[2];
    const int x0 = it.x0, y0 = it.y0, ox = P.ox, rw = P.rw;
    const size_t plane = (size_t)P.DW * P.DH;
    const size_t esz = out_esz(OUT);
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)(P.slot_offset + it.index * P.slot_stride) * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p1 ? p1 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(p2 ? p2 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    // output planes in store order (BGR, or RGB: planes 0 and 2 exchanged); NHWC: rsO0 is the whole slot
    const __amdgpu_buffer_rsrc_t rsO0 = __builtin_amdgcn_make_buffer_rsrc((void*)(!NHWC && P.color_rgb ? d2 : d0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO1 = __builtin_amdgcn_make_buffer_rsrc((void*)d1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsO2 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.color_rgb ? d0 : d2), (short)0, 0x7FFFFFFF, 0x00020000);

    float* lut_s = reinterpret_cast<float*>(smem);
    // fill values in output plane order (P.fill is already in output channel order)
    const int fo0 = P.fill & 0xFF, fo1 = (P.fill >> 8) & 0xFF, fo2 = (P.fill >> 16) & 0xFF;
    const int fb0 = P.color_rgb ? fo2 : fo0, fb2 = P.color_rgb ? fo0 : fo2;  // same, in BGR order

    const int X0 = tx * TW, Y0 = ty * P.TH, Y1 = min(Y0 + P.TH, P.DH);
    // visible (non-padding) columns of the tile -> source footprint (wave-uniform)
    const int Xv0 = max(X0, ox), Xv1 = min(min(X0 + TW, P.DW), ox + rw) - 1;
    const bool cols = Xv0 <= Xv1;
    int fsY = 0, nY = 0, fsC = 0, nC = 0;
    // both footprint taps in one batch of scalar loads (clamped indices: read even for padding tiles)
    const int fs0 = xtab_s[max(min(Xv0, P.DW - 1), 0)].s0, fs1 = xtab_s[max(min(Xv1, P.DW - 1), 0)].s1;
    if (cols) footprint_chunks(FMT, T::bpp, x0 + fs0, x0 + fs1, fsY, nY, fsC, nC);
    // per-lane column state for the PX pixels of this lane: the PX table loads go out together here and
    // are consumed after the first DMA is issued
    const int Xl = X0 + lane * PX;
    const bool xin = Xl < P.DW;  // DW % PX == 0: a lane's pixels are all in or all out
    XTab xts[PX];
#pragma unroll
    for (int j = 0; j < PX; j++) xts[j] = P.xtab[xin ? Xl + j : 0];
    uint32_t lY[PX], lC[PX], wa[PX];
    const uint32_t vo = (uint32_t)(xin ? Xl : 0) * (uint32_t)esz;

    // this wave's rows
    const int thw = (P.TH + 3) >> 2;
    const int Yw0 = Y0 + wave * thw, Yw1 = min(Yw0 + thw, Y1);
    uint8_t* const wbuf = smem + P.offBuf + wave * P.wave_bytes;
    const int half = P.wave_bytes >> 1;
    const int segY = P.segY, segC = P.segC;
    // buffer layout: [Y tap0][Y tap1][C tap0][C tap1][V tap0][V tap1]
    const int oY1 = segY, oC0 = 2 * segY, oC1 = 2 * segY + segC, oV0 = 2 * segY + 2 * segC, oV1 = oV0 + segC;

    LaneRows lr;  // this wave's rows (<= 64, host)
    lr.load(P.ytab, Yw0, Yw1 - Yw0, lane);

    // Staging decision for output row Y, given the source rows (pa, pb) whose H the wave holds.
    struct Plan {
        int ya, yb, b0, b1;
        bool pad, stA, stB, stCB;  // stage luma tap0 / tap1 rows; chroma of tap1 in its own slot
    };
    auto plan = [&](int Y, int pa, int pb) {
        Plan q;
        q.b0 = lr.B0(Y - Yw0);
        q.b1 = lr.B1(Y - Yw0);
        q.ya = y0 + lr.R0(Y - Yw0);
        q.yb = y0 + lr.R1(Y - Yw0);
        q.pad = (q.b0 | q.b1) == 0 || !cols;
        if (REUSE) {
            q.stA = q.ya != pa && q.ya != pb;
            q.stB = q.yb != q.ya && q.yb != pa && q.yb != pb;
        } else {
            q.stA = true;
            q.stB = q.yb != q.ya;
        }
        q.stCB = q.stB && !(q.stA && (q.ya >> 1) == (q.yb >> 1));
        return q;
    };
    auto dma = [&](const __amdgpu_buffer_rsrc_t rs, uint8_t* dst, int nck, int soff) {
        for (int c = 0; c < nck; c += 64) {
            if (lane + c < nck)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(dst + c * 16), 16,
                                                         (lane + c) * 16, soff, EVAM_PP_LOAD_AUX, 0);
        }
    };
    auto issue = [&](const Plan& q, uint8_t* buf) {
        if (q.pad || (kAblate & 16)) return;
        if (q.stA) {
            dma(rsY, buf, nY, q.ya * pitch0 + fsY);
            if constexpr (kYUV) dma(rsC, buf + oC0, nC, (q.ya >> 1) * pitch1 + fsC);
            if constexpr (FMT == kI420) dma(rsV, buf + oV0, nC, (q.ya >> 1) * pitch2 + fsC);
        }
        if (q.stB) {
            dma(rsY, buf + oY1, nY, q.yb * pitch0 + fsY);
            if (q.stCB) {
                if constexpr (kYUV) dma(rsC, buf + oC1, nC, (q.yb >> 1) * pitch1 + fsC);
                if constexpr (FMT == kI420) dma(rsV, buf + oV1, nC, (q.yb >> 1) * pitch2 + fsC);
            }
        }
    };

    // Horizontal pass of one staged source row (or two sharing their chroma row).
    auto hrow = [&](const uint8_t* sy, const uint8_t* sc, const uint8_t* sv, uint32_t (&H)[PX][3]) {
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const uint32_t tY0 = lY[j] & 0xFFFF, tY1 = lY[j] >> 16;
            int c0[3], c1[3];
            if constexpr (kYUV) {
                const uint32_t tC0 = lC[j] & 0xFFFF, tC1 = lC[j] >> 16;
                const uint8_t* svv = FMT == kNV12 ? sc + 1 : sv;
                hrow_sat(sy[tY0], sy[tY1], uv_terms_sat(sc[tC0], svv[tC0]), uv_terms_sat(sc[tC1], svv[tC1]),
                         (wa[j] >> 4) & 0x0FFF0FFFu, H[j]);
                continue;
            } else if constexpr (FMT == kBGRX) {
                const uint32_t q0 = *reinterpret_cast<const uint32_t*>(sy + tY0);
                const uint32_t q1 = *reinterpret_cast<const uint32_t*>(sy + tY1);
                c0[0] = q0 & 0xFF; c0[1] = (q0 >> 8) & 0xFF; c0[2] = (q0 >> 16) & 0xFF;
                c1[0] = q1 & 0xFF; c1[1] = (q1 >> 8) & 0xFF; c1[2] = (q1 >> 16) & 0xFF;
            } else {
                c0[0] = sy[tY0]; c0[1] = sy[tY0 + 1]; c0[2] = sy[tY0 + 2];
                c1[0] = sy[tY1]; c1[1] = sy[tY1 + 1]; c1[2] = sy[tY1 + 2];
            }
            const uint32_t a0 = wa[j] & 0xFFFF, a1 = wa[j] >> 16;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) H[j][ch] = __umul24(c0[ch], a0) + __umul24(c1[ch], a1);
        }
    };
    auto hrow2 = [&](const uint8_t* sya, const uint8_t* syb, const uint8_t* sc, const uint8_t* sv,
                     uint32_t (&HA)[PX][3], uint32_t (&HB)[PX][3]) {
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const uint32_t tY0 = lY[j] & 0xFFFF, tY1 = lY[j] >> 16;
            const uint32_t tC0 = lC[j] & 0xFFFF, tC1 = lC[j] >> 16;
            const uint8_t* svv = FMT == kNV12 ? sc + 1 : sv;
            const UVs sA = uv_terms_sat(sc[tC0], svv[tC0]), sB = uv_terms_sat(sc[tC1], svv[tC1]);
            const uint32_t wp = (wa[j] >> 4) & 0x0FFF0FFFu;
            hrow_sat(sya[tY0], sya[tY1], sA, sB, wp, HA[j]);
            hrow_sat(syb[tY0], syb[tY1], sA, sB, wp, HB[j]);
        }
    };

    auto store_row = [&](int Y, const int (&v)[3][PX]) {
        if (!xin || (kAblate & 4)) {
            if (kAblate & 4) asm volatile("" :: "v"(v[0][0]), "v"(v[1][0]), "v"(v[2][0]));
            return;
        }
        // Row offset in the VGPR offset, soffset 0. A >8-byte buffer store with an SGPR soffset is
        // exempt from the compiler's store-data hazard check, yet on gfx950 a VALU write right after
        // such a dwordx4 store corrupted the stored data (lanes 12-15 of each 16, first dword);
        // with soffset 0 the compiler inserts the wait state.
        if constexpr (NHWC) {
            // the lane's 12 elements in output channel order (RGB: B and R exchanged per pixel); the LUT sections
            // are per OUTPUT channel, so channel c of the output reads section c
            const uint32_t off3 = (vo + (uint32_t)(Y * P.DW) * (uint32_t)esz) * 3u;
            int e[3 * PX];
#pragma unroll
            for (int j = 0; j < PX; j++) {
                e[3 * j] = P.color_rgb ? v[2][j] : v[0][j];
                e[3 * j + 1] = v[1][j];
                e[3 * j + 2] = P.color_rgb ? v[0][j] : v[2][j];
            }
            if constexpr (OUT == 1) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    evam_v4i q;
#pragma unroll
                    for (int m = 0; m < 4; m++) q[m] = (int)__float_as_uint(lut_s[((4 * k + m) % 3) * 256 + e[4 * k + m]]);
                    __builtin_amdgcn_raw_buffer_store_b128(q, rsO0, off3 + 16u * k, 0, EVAM_PP_STORE_AUX);
                }
            } else {
                evam_v3i q;
#pragma unroll
                for (int k = 0; k < 3; k++)
                    q[k] = (int)((uint32_t)e[4 * k] | ((uint32_t)e[4 * k + 1] << 8) | ((uint32_t)e[4 * k + 2] << 16) |
                                 ((uint32_t)e[4 * k + 3] << 24));
                __builtin_amdgcn_raw_buffer_store_b96(q, rsO0, off3, 0, EVAM_PP_STORE_AUX);
            }
            return;
        }
        const uint32_t off = vo + (uint32_t)(Y * P.DW) * (uint32_t)esz;
        // the LUT is per output plane: B lands in plane 2 when the output is RGB
        store_vec<OUT, PX>(rsO0, off, 0, lut_s + (P.color_rgb ? 512 : 0), v[0]);
        store_vec<OUT, PX>(rsO1, off, 0, lut_s + 256, v[1]);
        store_vec<OUT, PX>(rsO2, off, 0, lut_s + (P.color_rgb ? 0 : 512), v[2]);
    };

    uint32_t HA[PX][3], HB[PX][3];  // H of source rows pa, pb (REUSE) / of this row's taps
#pragma unroll
    for (int j = 0; j < PX; j++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) HA[j][ch] = HB[j][ch] = 0;
    int pa = -1, pb = -1;
    // Prologue order: the first row's DMA needs only the item, the footprint and the row table, so it goes
    // out before the LUT load, its barrier and the per-lane column math, whose latency it then covers.
    Plan cur{};
    if (Yw0 < Yw1) {
        cur = plan(Yw0, pa, pb);
        issue(cur, wbuf);
    }
    if constexpr (OUT != 0) {
        for (int i = tid; i < 768; i += kThreads) lut_s[i] = P.lut[i];
        __syncthreads();  // every wave, including those without rows
    }
    if (Yw0 >= Yw1) return;
#pragma unroll
    for (int j = 0; j < PX; j++) {
        const XTab& xt = xts[j];
        wa[j] = (uint32_t)xt.a0 | ((uint32_t)xt.a1 << 16);
        lY[j] = lC[j] = 0;
        if (xin && wa[j] != 0) {
            const int ca = x0 + xt.s0, cb = x0 + xt.s1;
            lY[j] = (uint32_t)(ca * T::bpp - fsY) | ((uint32_t)(cb * T::bpp - fsY) << 16);
            if constexpr (FMT == kNV12)
                lC[j] = (uint32_t)(2 * (ca >> 1) - fsC) | ((uint32_t)(2 * (cb >> 1) - fsC) << 16);
            else if constexpr (FMT == kI420)
                lC[j] = (uint32_t)((ca >> 1) - fsC) | ((uint32_t)((cb >> 1) - fsC) << 16);
        }
    }
    int i = 0;
    for (int Y = Yw0; Y < Yw1; Y++, i++) {
        // this row's DMA landed; the previous row's stores (three, or the single 12-byte one of u8 NHWC) may stay
        // in flight
        if (i == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if constexpr (NHWC && OUT == 0) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        const uint8_t* buf = wbuf + (i & 1) * half;
        const int na = cur.pad ? pa : cur.ya, nb = cur.pad ? pb : cur.yb;
        Plan nxt{};
        if (Y + 1 < Yw1) {
            nxt = plan(Y + 1, na, nb);
            issue(nxt, wbuf + ((i + 1) & 1) * half);  // that buffer was last read by row Y - 1
        }
        // Keep every DMA of row Y + 1 ahead of row Y's stores: the vmcnt(3) above relies on that order.
        asm volatile("" ::: "memory");
        int v[3][PX];
        if (cur.pad || (kAblate & 2)) {
#pragma unroll
            for (int j = 0; j < PX; j++) { v[0][j] = fb0; v[1][j] = fo1; v[2][j] = fb2; }
        } else {
            uint32_t NA[PX][3], NB[PX][3];
            const bool shareC = kYUV && cur.stA && cur.stB && !cur.stCB;
            if (shareC) {
                if constexpr (kYUV) hrow2(buf, buf + oY1, buf + oC0, buf + oV0, NA, NB);
            } else {
                if (cur.stA) hrow(buf, buf + oC0, buf + oV0, NA);
                else {
#pragma unroll
                    for (int j = 0; j < PX; j++)
#pragma unroll
                        for (int ch = 0; ch < 3; ch++) NA[j][ch] = cur.ya == pa ? HA[j][ch] : HB[j][ch];
                }
                if (cur.stB) hrow(buf + oY1, buf + (cur.stCB ? oC1 : oC0), buf + (cur.stCB ? oV1 : oV0), NB);
                else {
#pragma unroll
                    for (int j = 0; j < PX; j++)
#pragma unroll
                        for (int ch = 0; ch < 3; ch++)
                            NB[j][ch] = cur.yb == cur.ya ? NA[j][ch] : (cur.yb == pa ? HA[j][ch] : HB[j][ch]);
                }
            }
            const uint32_t wb0 = (uint32_t)cur.b0, wb1 = (uint32_t)cur.b1;
#pragma unroll
            for (int j = 0; j < PX; j++) {
                const bool padc = wa[j] == 0;  // letterbox padding column
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const int r = vresize(NA[j][ch], NB[j][ch], wb0, wb1);
                    v[ch][j] = padc ? (ch == 0 ? fb0 : (ch == 1 ? fo1 : fb2)) : r;
                }
            }
            if (REUSE) {
#pragma unroll
                for (int j = 0; j < PX; j++)
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) { HA[j][ch] = NA[j][ch]; HB[j][ch] = NB[j][ch]; }
            }
        }
        store_row(Y, v);
        asm volatile("" ::: "memory");
        pa = na;
        pb = nb;
        cur = nxt;
    }
}

}  // namespace
