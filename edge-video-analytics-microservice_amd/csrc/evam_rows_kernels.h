// evam_pp_rows, the rows kernel (uniform geometry, host-built tables, no staging), and the helpers only it uses: UV3,
// uv_terms, y_plus_uv, Chroma<FMT>, chroma_terms. Source bytes: buffer loads straight from the frame through L1, the
// row offset wave-uniform in the SGPR offset and the column offset per lane; all taps of a row before any arithmetic.
// LDS: the LUT only (fp32 output). Waits: one __syncthreads() after the LUT; the loads' vmcnt waits are the compiler's.
// Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

namespace {

// BT.601 split into the chroma part (per chroma sample) and the per-luma part, so a chroma sample
// shared by two taps is converted once. Same integers as the generic kernel's yuv_to_bgr.
struct UV3 { int b, g, r; };
__device__ __forceinline__ UV3 uv_terms(int U, int V) {
    return UV3{__mul24(kCUB, U) + kKB, __mul24(kCVG, V) + __mul24(kCUG, U) + kKG, __mul24(kCVR, V) + kKR};
}
__device__ __forceinline__ void y_plus_uv(int Y, const UV3& t, int& b, int& g, int& r) {
    const int y = __mul24(max(Y, 16), kCY);
    b = clamp255((y + t.b) >> 20);
    g = clamp255((y + t.g) >> 20);
    r = clamp255((y + t.r) >> 20);
}

template <int FMT>
struct Chroma {  // raw chroma of one tap: NV12 packed UV (u16), I420 U and V bytes
    uint32_t u, v;
};
template <int FMT>
__device__ __forceinline__ UV3 chroma_terms(const Chroma<FMT>& c) {
    if constexpr (FMT == kNV12) return uv_terms((int)(c.u & 0xFF), (int)(c.u >> 8));
    else return uv_terms((int)c.u, (int)c.v);
}

// Uniform-geometry kernel: every item of the launch has the same crop size, resized size and
// placement, so the coefficient tables come precomputed from the host (XTab / YTab, L2-resident) and
// each wave walks whole 64-pixel row segments. Row pointers, vertical weights and the destination row
// are wave-uniform SGPR values; column offsets and horizontal weights are per-lane registers loaded
// once per workgroup. The inner loop therefore spends its VALU slots on the arithmetic alone. When
// both vertical taps read the same chroma row (4:2:0, ~half the rows) their chroma is loaded and
// converted once.
template <int FMT, int OUT>
__global__ __launch_bounds__(kThreads) void evam_pp_rows(const RParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using T = FmtTraits<FMT>;
    constexpr bool kYUV = FMT == kNV12 || FMT == kI420;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.x;
    const int item = t / P.tiles_per_item;
    const int tile = t - item * P.tiles_per_item;
    const int ty = tile / P.tiles_x;
    const int tx = tile - ty * P.tiles_x;
    const ItemArg& it = P.items[item];
    const __attribute__((address_space(4))) YTab* ytab = (const __attribute__((address_space(4))) YTab*)(P.ytab);
    const uint8_t* __restrict__ p0 = it.plane[0];
    const uint8_t* __restrict__ p1 = it.plane[1];
    const uint8_t* __restrict__ p2 = it.plane[2];
    const int pitch0 = it.pitch[0], pitch1 = it.pitch[1], pitch2 = it.pitch[2];
    const int x0 = it.x0, y0 = it.y0;
    const size_t plane = (size_t)P.DW * P.DH;
    const size_t esz = OUT == 1 ? 4 : 1;
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)(P.slot_offset + it.index * P.slot_stride) * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;
    // Buffer resources (wave-uniform). Offsets are always in range by construction, so the range
    // check is set wide open.
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p1 ? p1 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(p2 ? p2 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD0 = __builtin_amdgcn_make_buffer_rsrc((void*)d0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD1 = __builtin_amdgcn_make_buffer_rsrc((void*)d1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD2 = __builtin_amdgcn_make_buffer_rsrc((void*)d2, (short)0, 0x7FFFFFFF, 0x00020000);

    float* lut_s = reinterpret_cast<float*>(smem);
    if constexpr (OUT == 1) {
        for (int i = tid; i < 768; i += kThreads) lut_s[i] = P.lut[i];
        __syncthreads();
    }
    const int f0 = P.fill & 0xFF, f1 = (P.fill >> 8) & 0xFF, f2 = (P.fill >> 16) & 0xFF;

    // Which 64-pixel column segments and which rows of the tile this wave owns.
    const int X0 = tx * P.TW, Y0 = ty * P.TH, Y1 = min(Y0 + P.TH, P.DH);
    int seg0, seg_step, nseg, row0, row_step;
    if (P.nsegx >= 4) { seg0 = wave; seg_step = 4; nseg = P.nsegx >> 2; row0 = 0; row_step = 1; }
    else { seg0 = wave % P.nsegx; seg_step = 0; nseg = 1; row0 = wave / P.nsegx; row_step = 4 / P.nsegx; }

    // Per-lane column state, up to two segments per wave.
    uint32_t oY0[2], oY1[2], oC0[2], oC1[2], wa[2], xo[2];
    bool xin[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int X = X0 + (seg0 + j * seg_step) * 64 + lane;
        xin[j] = j < nseg && X < P.DW;
        const XTab xt = P.xtab[xin[j] ? X : 0];
        const int ca = x0 + xt.s0, cb = x0 + xt.s1;
        oY0[j] = (uint32_t)(ca * T::bpp);
        oY1[j] = (uint32_t)(cb * T::bpp);
        oC0[j] = FMT == kNV12 ? (uint32_t)(2 * (ca >> 1)) : (uint32_t)(ca >> 1);
        oC1[j] = FMT == kNV12 ? (uint32_t)(2 * (cb >> 1)) : (uint32_t)(cb >> 1);
        wa[j] = (uint32_t)xt.a0 | ((uint32_t)xt.a1 << 16);
        xo[j] = (uint32_t)(xin[j] ? X : 0);
    }

    for (int Y = Y0 + row0; Y < Y1; Y += row_step) {
        const int yr0 = ytab[Y].r0, yr1 = ytab[Y].r1, yb0 = ytab[Y].b0, yb1 = ytab[Y].b1;  // scalar loads
        const uint32_t orow = (uint32_t)(Y * P.DW);
        if ((yb0 | yb1) == 0 || (kAblate & 2)) {  // padding row (letterbox)
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (xin[j] && !(kAblate & 4)) store_px<OUT>(d0, d1, d2, lut_s, orow + xo[j], f0, f1, f2);
            continue;
        }
        const int ya = y0 + yr0, yb = y0 + yr1;
        // Wave-uniform row offsets go in the buffer instructions' SGPR offset; the per-lane column
        // offsets are the VGPR offsets: no per-tap address arithmetic at all.
        const int sY0 = ya * pitch0, sY1 = yb * pitch0;
        const int sC0 = (ya >> 1) * pitch1, sC1 = (yb >> 1) * pitch1;
        const int sV0 = (ya >> 1) * pitch2, sV1 = (yb >> 1) * pitch2;
        const uint32_t wb0 = (uint32_t)yb0, wb1 = (uint32_t)yb1;
        const int sO = (int)(orow * (uint32_t)esz);

        auto run = [&](auto share_tag) {
            constexpr bool kShare = decltype(share_tag)::value;
            // ---- gather: every tap of every owned segment, before any arithmetic ----
            uint32_t q[2][4][3];
            Chroma<FMT> ch[2][4];
            if (kAblate & 16) {  // diagnostics: no loads, arithmetic on synthetic bytes
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        q[j][k][0] = (oY0[j] + 37 * k) & 255; q[j][k][1] = (oY1[j] + k) & 255; q[j][k][2] = (oC0[j] + k) & 255;
                        ch[j][k].u = (oC1[j] * (k + 1)) & 0xFFFF; ch[j][k].v = (oC0[j] ^ k) & 255;
                    }
            } else
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if constexpr (kYUV) {
                    q[j][0][0] = __builtin_amdgcn_raw_buffer_load_b8(rsY, oY0[j], sY0, 0);
                    q[j][1][0] = __builtin_amdgcn_raw_buffer_load_b8(rsY, oY1[j], sY0, 0);
                    q[j][2][0] = __builtin_amdgcn_raw_buffer_load_b8(rsY, oY0[j], sY1, 0);
                    q[j][3][0] = __builtin_amdgcn_raw_buffer_load_b8(rsY, oY1[j], sY1, 0);
                    if constexpr (FMT == kNV12) {
                        ch[j][0].u = __builtin_amdgcn_raw_buffer_load_b16(rsC, oC0[j], sC0, 0);
                        ch[j][1].u = __builtin_amdgcn_raw_buffer_load_b16(rsC, oC1[j], sC0, 0);
                        if constexpr (!kShare) {
                            ch[j][2].u = __builtin_amdgcn_raw_buffer_load_b16(rsC, oC0[j], sC1, 0);
                            ch[j][3].u = __builtin_amdgcn_raw_buffer_load_b16(rsC, oC1[j], sC1, 0);
                        }
                    } else {
                        ch[j][0].u = __builtin_amdgcn_raw_buffer_load_b8(rsC, oC0[j], sC0, 0);
                        ch[j][0].v = __builtin_amdgcn_raw_buffer_load_b8(rsV, oC0[j], sV0, 0);
                        ch[j][1].u = __builtin_amdgcn_raw_buffer_load_b8(rsC, oC1[j], sC0, 0);
                        ch[j][1].v = __builtin_amdgcn_raw_buffer_load_b8(rsV, oC1[j], sV0, 0);
                        if constexpr (!kShare) {
                            ch[j][2].u = __builtin_amdgcn_raw_buffer_load_b8(rsC, oC0[j], sC1, 0);
                            ch[j][2].v = __builtin_amdgcn_raw_buffer_load_b8(rsV, oC0[j], sV1, 0);
                            ch[j][3].u = __builtin_amdgcn_raw_buffer_load_b8(rsC, oC1[j], sC1, 0);
                            ch[j][3].v = __builtin_amdgcn_raw_buffer_load_b8(rsV, oC1[j], sV1, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int sr = (k >> 1) ? sY1 : sY0;
                        const uint32_t o = (k & 1) ? oY1[j] : oY0[j];
                        if constexpr (FMT == kBGRX) {
                            q[j][k][0] = __builtin_amdgcn_raw_buffer_load_b32(rsY, o, sr, 0);
                        } else {
                            q[j][k][0] = __builtin_amdgcn_raw_buffer_load_b8(rsY, o, sr, 0);
                            q[j][k][1] = __builtin_amdgcn_raw_buffer_load_b8(rsY, o + 1, sr, 0);
                            q[j][k][2] = __builtin_amdgcn_raw_buffer_load_b8(rsY, o + 2, sr, 0);
                        }
                    }
                }
                if (j + 1 >= nseg) break;
            }
            // ---- arithmetic + stores ----
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (j < nseg && xin[j]) {
                    if (kAblate & 8) {  // diagnostics: loads only
                        uint32_t acc = ch[j][0].u + ch[j][1].u + (kShare ? 0u : ch[j][2].u + ch[j][3].u);
#pragma unroll
                        for (int k = 0; k < 4; k++) acc += q[j][k][0];
                        asm volatile("" :: "v"(acc));
                        continue;
                    }
                    const uint32_t a0 = wa[j] & 0xFFFF, a1 = wa[j] >> 16;  // 15-bit
                    int c[4][3];
                    if constexpr (kYUV) {
                        const UV3 tA = chroma_terms<FMT>(ch[j][0]);
                        const UV3 tB = chroma_terms<FMT>(ch[j][1]);
                        const UV3 tC = kShare ? tA : chroma_terms<FMT>(ch[j][2]);
                        const UV3 tD = kShare ? tB : chroma_terms<FMT>(ch[j][3]);
                        y_plus_uv((int)q[j][0][0], tA, c[0][0], c[0][1], c[0][2]);
                        y_plus_uv((int)q[j][1][0], tB, c[1][0], c[1][1], c[1][2]);
                        y_plus_uv((int)q[j][2][0], tC, c[2][0], c[2][1], c[2][2]);
                        y_plus_uv((int)q[j][3][0], tD, c[3][0], c[3][1], c[3][2]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            if constexpr (FMT == kBGRX) {
                                c[k][0] = q[j][k][0] & 0xFF; c[k][1] = (q[j][k][0] >> 8) & 0xFF; c[k][2] = (q[j][k][0] >> 16) & 0xFF;
                            } else {
                                c[k][0] = (int)q[j][k][0]; c[k][1] = (int)q[j][k][1]; c[k][2] = (int)q[j][k][2];
                            }
                        }
                    }
                    int v[3];
#pragma unroll
                    for (int ch3 = 0; ch3 < 3; ch3++) {
                        const uint32_t D0 = __umul24(c[0][ch3], a0) + __umul24(c[1][ch3], a1);
                        const uint32_t D1 = __umul24(c[2][ch3], a0) + __umul24(c[3][ch3], a1);
                        v[ch3] = vresize(D0, D1, wb0, wb1);
                    }
                    if (kAblate & 4) {
                        asm volatile("" :: "v"(v[0]), "v"(v[1]), "v"(v[2]));
                    } else {
                        if (P.color_rgb) { const int tmp = v[0]; v[0] = v[2]; v[2] = tmp; }
                        if (wa[j] == 0) {  // letterbox padding column (zero weights): the fill, in output plane order
                            v[0] = f0; v[1] = f1; v[2] = f2;
                        }
                        const uint32_t vo = xo[j] * (uint32_t)esz;
                        if constexpr (OUT == 1) {
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lut_s[v[0]]), rsD0, vo, sO, EVAM_PP_STORE_AUX);
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lut_s[256 + v[1]]), rsD1, vo, sO, EVAM_PP_STORE_AUX);
                            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lut_s[512 + v[2]]), rsD2, vo, sO, EVAM_PP_STORE_AUX);
                        } else {
                            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[0], rsD0, vo, sO, EVAM_PP_STORE_AUX);
                            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[1], rsD1, vo, sO, EVAM_PP_STORE_AUX);
                            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[2], rsD2, vo, sO, EVAM_PP_STORE_AUX);
                        }
                    }
                }
            }
        };
        if constexpr (kYUV) {
            if ((ya >> 1) == (yb >> 1)) run(std::true_type{});
            else run(std::false_type{});
        } else {
            run(std::false_type{});
        }
    }
}

}  // namespace
