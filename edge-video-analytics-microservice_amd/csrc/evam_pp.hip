// evam_pp.hip — MI355X (gfx950) frame pre-processing backend: fused colour-convert + OpenCV-exact
// INTER_LINEAR resize + letterbox/central-crop placement + normalisation + NCHW batch packing.
//
// Drop-in for DL Streamer 2022.1's `opencv` pre-proc backend (ImagePreprocessor::Convert, third
// party) that EVAM selects through pipelines/*/pipeline.json element properties
// (pipelines/object_detection/vehicle/pipeline.json:5,13-18; pipelines/object_classification/
// vehicle_attributes/pipeline.json:4-5,12-23; pipelines/action_recognition/general/pipeline.json:3-4).
// The C ABI is declared in include/evam_pp.h; SURVEY.md §8 is the scope table.
//
// Design (DESIGN.md has the full write-up):
//  * One launch per (source format, call) and group of items; the host planner (evam_plan.h) picks the kernel family
//    per group (DESIGN.md §4 has the table): strip, band, wave, staged or rows for items of one geometry, roi for
//    per-item geometry, and the generic kernel for whatever those do not plan.
//  * Every family computes the same integers: the OpenCV coefficient tables in the exact double/float operation
//    sequence of hal::resize (no FMA contraction: built -ffp-contract=off), the four taps of an output pixel converted
//    to BGR (BT.601 20-bit fixed point), the 11-bit horizontal pass and the VResizeLinear 32s->8u vertical pass, the u8
//    result mapped through the per-channel normalisation LUT (fp32 out) and stored planar NCHW, or, for a tensor with
//    layout = EVAM_LAYOUT_NHWC, as the slot's interleaved H x W x 3 image (a NHWC template parameter on the strip,
//    band, wave and generic kernels: only the store epilogue differs). fp16 / bf16 output (EVAM_DTYPE_F16 / _BF16) is
//    the same path with a table of 16-bit patterns and 2-byte stores (OUT = 2 on the generic, strip, ROI and wave
//    kernels; interleaved 16-bit output: the generic kernel only).
//  * The families differ in how source bytes reach the arithmetic: the generic and rows kernels gather taps straight
//    from the frame through L1; the others stage source row segments in LDS by LDS-DMA, per workgroup (staged, roi) or
//    per wave with counted vmcnt waits and no barrier in the loop (wave, strip, band). Each family's header says how.
//  * Letterbox padding never touches the source. Nothing is MFMA-shaped: the path is HBM-bound integer gather work
//    (roofline: HBM, 8 TB/s).
//
// One translation unit. This file: the generic, rows, staged, wave and roi kernel families (each with the helpers only
// it uses next to it), the kernel tables, launch_kernel and resident_per_cu (HipKernels, the planner's HIP backend),
// HipRings, struct evam_pp, run_impl and the evam_pp_run entry points. Included:
//  * evam_params.h (kernel-argument structs) and evam_plan.h (the host planner), both HIP-free;
//  * evam_kernel_common.h (device helpers that two or more families share), evam_strip_kernels.h and
//    evam_band_kernels.h (those two families, each with the helpers only it uses);
//  * the device-resident ROI lists, JPEG, JPEG-decode, tracker and DetectionOutput kernels and entry points
//    (evam_{rois,jpeg,jpeg_dec,track,detout}_kernels.h and _api.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include <immintrin.h>

#include "../../include/evam_pp.h"

#define EVAM_HD __host__ __device__
#include "evam_geom.h"
#include "evam_params.h"
#include "evam_plan.h"
#include "evam_rings.h"
#include "evam_clip_simd.h"
#include "evam_jpeg_dec.h"
#include "evam_track.h"
#include "evam_detout.h"

namespace {

using namespace evam;

}  // namespace

// Device code. evam_kernel_common.h and the family headers reopen the anonymous namespace at file scope, so a kernel's
// symbol does not depend on where its text lives.
#include "evam_kernel_common.h"

namespace {

// Workgroups are dispatched round-robin over the 8 XCDs (block b runs on XCD b % 8). Remap so each
// XCD walks a contiguous run of tiles: neighbouring tiles of one frame share source rows at their
// edges, and those rows then hit the same L2. Bijective for any grid size.
__device__ inline int xcd_tile(int b, int grid) {
    const int q = grid >> 3, r = grid & 7, x = b & 7, i = b >> 3;
    return x < r ? x * (q + 1) + i : r * (q + 1) + (x - r) * q + i;
}

// BT.601 20-bit fixed point (OpenCV uvToRGBuv + yRGBuvToRGBA). Arguments are raw bytes; every
// product fits the full-rate 24-bit multiplier.
__device__ __forceinline__ void yuv_to_bgr(int Y, int U, int V, int& b, int& g, int& r) {
    const int y = __mul24(max(Y, 16), kCY);  // max(Y-16,0)*CY + 16*CY; the 16*CY is folded into kK*
    const int ruv = __mul24(kCVR, V) + kKR;
    const int guv = __mul24(kCVG, V) + __mul24(kCUG, U) + kKG;
    const int buv = __mul24(kCUB, U) + kKB;
    b = clamp255((y + buv) >> 20);
    g = clamp255((y + guv) >> 20);
    r = clamp255((y + ruv) >> 20);
}

// Raw bytes of one source pixel, read straight from the frame (global memory, through L1/L2).
// Plane bases are wave-uniform (SGPR) and offsets 32-bit, so each load is one saddr-form instruction.
template <int FMT>
__device__ __forceinline__ void load_tap(const uint8_t* __restrict__ p0, const uint8_t* __restrict__ p1,
                                         const uint8_t* __restrict__ p2, uint32_t oy, uint32_t oc, uint32_t ov,
                                         uint32_t (&v)[3]) {
    if constexpr (FMT == kNV12) {
        v[0] = p0[oy];
        v[1] = *reinterpret_cast<const uint16_t*>(p1 + oc);
    } else if constexpr (FMT == kI420) {
        v[0] = p0[oy];
        v[1] = p1[oc];
        v[2] = p2[ov];
    } else if constexpr (FMT == kBGRX) {
        v[0] = *reinterpret_cast<const uint32_t*>(p0 + oy);
    } else {
        v[0] = p0[oy];
        v[1] = p0[oy + 1];
        v[2] = p0[oy + 2];
    }
}

template <int FMT>
__device__ __forceinline__ void to_bgr(const uint32_t (&v)[3], int& b, int& g, int& r) {
    if constexpr (FMT == kNV12) {
        yuv_to_bgr((int)v[0], (int)(v[1] & 0xFF), (int)(v[1] >> 8), b, g, r);
    } else if constexpr (FMT == kI420) {
        yuv_to_bgr((int)v[0], (int)v[1], (int)v[2], b, g, r);
    } else if constexpr (FMT == kBGRX) {
        b = v[0] & 0xFF; g = (v[0] >> 8) & 0xFF; r = (v[0] >> 16) & 0xFF;
    } else {
        b = (int)v[0]; g = (int)v[1]; r = (int)v[2];
    }
}

// One workgroup per output tile (TW x TH pixels of one item). The workgroup builds the OpenCV
// coefficient tables of its columns and rows in LDS (device-side, exact double/float sequence), then
// every lane gathers the four taps of its pixels directly from the frame in HBM — luma and chroma
// bytes through L1, adjacent lanes sharing cache lines — converts them to BGR, runs both resize passes,
// maps the u8 result through the normalisation LUT and stores the three planes. No staging, no barrier
// after the tables: the memory pipeline overlaps loads of many pixels and many waves.
template <int FMT, int OUT, bool NHWC = false>
__global__ __launch_bounds__(kThreads) void evam_pp_kernel(const KParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using T = FmtTraits<FMT>;
    const int tid = threadIdx.x;
    const int t = blockIdx.x;
    const int item = t / P.tiles_per_item;
    const int tile = t - item * P.tiles_per_item;
    const int ty = tile / P.tiles_x;
    const int tx = tile - ty * P.tiles_x;
    // Descriptors are read-only for the launch: the constant address space makes them scalar loads.
    const __attribute__((address_space(4))) ItemDesc* it =
        (const __attribute__((address_space(4))) ItemDesc*)(P.items) + item;
    const uint8_t* __restrict__ p0 = it->plane[0];
    const uint8_t* __restrict__ p1 = it->plane[1];
    const uint8_t* __restrict__ p2 = it->plane[2];
    const int pitch0 = it->pitch[0], pitch1 = it->pitch[1], pitch2 = it->pitch[2];
    const int x0 = it->x0, y0 = it->y0, cw = it->cw, ch = it->ch;
    const int rw = it->rw, rh = it->rh, ox = it->ox, oy = it->oy;
    const double scx = it->scale_x, scy = it->scale_y;
    const int X0 = tx * P.TW, Y0 = ty * P.TH;
    const int X1 = min(X0 + P.TW, P.DW), Y1 = min(Y0 + P.TH, P.DH);
    const size_t plane = (size_t)P.DW * P.DH;
    const size_t esz = out_esz(OUT);
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)(P.slot_offset + it->index * P.slot_stride) * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;

    float* lut_s = reinterpret_cast<float*>(smem);
    if constexpr (OUT != 0) {
        for (int i = tid; i < 768; i += kThreads) lut_s[i] = P.lut[i];
    }
    ColEntry* coltab = reinterpret_cast<ColEntry*>(smem + P.offCol);
    RowEntry* rowtab = reinterpret_cast<RowEntry*>(smem + P.offRow);
    for (int lx = tid; lx < P.TW; lx += kThreads) {
        ColEntry e;
        const int dx = X0 + lx - ox;
        if (X0 + lx < X1 && dx >= 0 && dx < rw) {
            int sx, a0, a1;
            linear_coef(dx, scx, cw, true, sx, a0, a1);
            const int ca = x0 + sx, cb = x0 + min(sx + 1, cw - 1);
            e.oY0 = ca * T::bpp;
            e.oY1 = cb * T::bpp;
            e.oC0 = FMT == kNV12 ? 2 * (ca >> 1) : (ca >> 1);
            e.a0 = (uint16_t)(a0 << 4);
            e.a1 = (uint16_t)(a1 << 4);
        } else {
            e.oY0 = 0; e.oY1 = 0; e.oC0 = 0; e.a0 = 0; e.a1 = 0;
        }
        coltab[lx] = e;
    }
    for (int ly = tid; ly < P.TH; ly += kThreads) {
        RowEntry e;
        const int dy = Y0 + ly - oy;
        if (Y0 + ly < Y1 && dy >= 0 && dy < rh) {
            int sy, b0, b1;
            linear_coef(dy, scy, ch, false, sy, b0, b1);
            const int ya = y0 + min(max(sy, 0), ch - 1);
            const int yb = y0 + min(max(sy + 1, 0), ch - 1);
            e.y0 = ya * pitch0;
            e.y1 = yb * pitch0;
            e.c0 = (ya >> 1) * pitch1;
            e.c1 = (yb >> 1) * pitch1;
            e.v0 = FMT == kI420 ? (ya >> 1) * pitch2 : 0;
            e.v1 = FMT == kI420 ? (yb >> 1) * pitch2 : 0;
            e.b0 = b0 << 8;
            e.b1 = b1 << 8;
        } else {
            e.y0 = 0; e.y1 = 0; e.c0 = 0; e.c1 = 0; e.b0 = 0; e.b1 = 0; e.v0 = 0; e.v1 = 0;
        }
        rowtab[ly] = e;
    }
    __syncthreads();

    const int f0 = P.fill & 0xFF, f1 = (P.fill >> 8) & 0xFF, f2 = (P.fill >> 16) & 0xFF;
    const int npx = P.TW * P.TH;
    // (lx, ly) of pixel p = tid + k * 256, advanced incrementally (no per-pixel division).
    const int qstep = kThreads / P.TW, rstep = kThreads - qstep * P.TW;
    int ly = tid / P.TW;
    int lx = tid - ly * P.TW;
    const uint32_t o_tile = (uint32_t)(Y0 * P.DW + X0);

    // Software pipeline, one pixel deep: the tap loads of pixel k+1 are issued before pixel k is
    // converted, so every wave always has a pixel's loads in flight while it computes.
    struct Px {
        uint32_t raw[4][3];
        uint32_t o, wa, wb0, wb1;
        int mode;  // 0: outside the tile, 1: padding / fill, 2: image pixel
    };
    auto gather = [&](int p, Px& x) {
        const int cx = lx, cy = ly;
        lx += rstep;
        ly += qstep;
        if (lx >= P.TW) { lx -= P.TW; ly++; }
        const bool in_tile = p < npx && X0 + cx < X1 && Y0 + cy < Y1;
        const ColEntry ce = coltab[in_tile ? cx : 0];
        const RowEntry re = rowtab[in_tile ? cy : 0];
        x.wa = (uint32_t)ce.a0 | ((uint32_t)ce.a1 << 16);
        x.wb0 = (uint32_t)re.b0;
        x.wb1 = (uint32_t)re.b1;
        const bool img = in_tile && x.wa != 0 && (x.wb0 | x.wb1) != 0 && !(kAblate & 2);
        x.mode = !in_tile ? 0 : (img ? 2 : 1);
        x.o = o_tile + __umul24((uint32_t)cy, (uint32_t)P.DW) + (uint32_t)cx;
        if (kAblate & 16) {  // diagnostics: no loads, math on synthetic bytes
            for (int k = 0; k < 4; k++) { x.raw[k][0] = (ce.oY0 + k) & 255; x.raw[k][1] = (re.y0 + ce.oC0 * k) & 0xFFFF; x.raw[k][2] = k; }
            return;
        }
        // Table offsets are valid addresses even for padding / out-of-tile lanes: no selects here.
        const uint32_t oc1 = FMT == kNV12 ? ((uint32_t)ce.oY1 & ~1u) : ((uint32_t)ce.oY1 >> 1);  // tap-1 chroma
        load_tap<FMT>(p0, p1, p2, (uint32_t)(re.y0 + ce.oY0), (uint32_t)(re.c0 + ce.oC0), (uint32_t)(re.v0 + ce.oC0),
                      x.raw[0]);
        load_tap<FMT>(p0, p1, p2, (uint32_t)(re.y0 + ce.oY1), (uint32_t)re.c0 + oc1, (uint32_t)re.v0 + oc1, x.raw[1]);
        load_tap<FMT>(p0, p1, p2, (uint32_t)(re.y1 + ce.oY0), (uint32_t)(re.c1 + ce.oC0), (uint32_t)(re.v1 + ce.oC0),
                      x.raw[2]);
        load_tap<FMT>(p0, p1, p2, (uint32_t)(re.y1 + ce.oY1), (uint32_t)re.c1 + oc1, (uint32_t)re.v1 + oc1, x.raw[3]);
    };
    auto finish = [&](const Px& x) {
        if (x.mode == 0) return;
        if (x.mode == 1) {
            if (!(kAblate & 4)) store_px<OUT, NHWC>(d0, d1, d2, lut_s, x.o, f0, f1, f2);
            return;
        }
        if (kAblate & 8) {  // diagnostics: loads only, trivial math
            uint32_t acc = 0;
            for (int k = 0; k < 4; k++) acc += x.raw[k][0] + x.raw[k][1] + x.raw[k][2];
            asm volatile("" :: "v"(acc));
            return;
        }
        const uint32_t a0 = x.wa & 0xFFFF, a1 = x.wa >> 16;  // 15-bit
        int bA, gA, rA, bB, gB, rB;
        to_bgr<FMT>(x.raw[0], bA, gA, rA);
        to_bgr<FMT>(x.raw[1], bB, gB, rB);
        const uint32_t Db0 = __umul24(bA, a0) + __umul24(bB, a1);
        const uint32_t Dg0 = __umul24(gA, a0) + __umul24(gB, a1);
        const uint32_t Dr0 = __umul24(rA, a0) + __umul24(rB, a1);
        to_bgr<FMT>(x.raw[2], bA, gA, rA);
        to_bgr<FMT>(x.raw[3], bB, gB, rB);
        const uint32_t Db1 = __umul24(bA, a0) + __umul24(bB, a1);
        const uint32_t Dg1 = __umul24(gA, a0) + __umul24(gB, a1);
        const uint32_t Dr1 = __umul24(rA, a0) + __umul24(rB, a1);
        const int vb = vresize(Db0, Db1, x.wb0, x.wb1);
        const int vg = vresize(Dg0, Dg1, x.wb0, x.wb1);
        const int vr = vresize(Dr0, Dr1, x.wb0, x.wb1);
        if (kAblate & 4) {
            asm volatile("" :: "v"(vb), "v"(vg), "v"(vr));  // keep the math alive
            return;
        }
        if (P.color_rgb)
            store_px<OUT, NHWC>(d0, d1, d2, lut_s, x.o, vr, vg, vb);
        else
            store_px<OUT, NHWC>(d0, d1, d2, lut_s, x.o, vb, vg, vr);
    };
    if (tid >= npx) return;
    Px cur, nxt;
    gather(tid, cur);
    for (int p = tid + kThreads; p < npx; p += kThreads) {
        gather(p, nxt);
        finish(cur);
        cur = nxt;
    }
    finish(cur);
}

// BT.601 split into the chroma part (per chroma sample) and the per-luma part, so a chroma sample
// shared by two taps is converted once. Same integers as yuv_to_bgr.
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

__device__ __forceinline__ void vmcnt_at_most(int n) {
    n = __builtin_amdgcn_readfirstlane(n);
    if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (n >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (n >= 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Staged uniform-geometry kernel. A workgroup owns a TW x TH tile (TW = 64 x NSEGX) and walks it in
// groups of R output rows. For each group the source row segments its taps need (two luma rows and
// two chroma rows per output row, each at most kSlot bytes wide) are brought into LDS by LDS-DMA —
// one 16 B/lane buffer_load ... lds per row segment, the row offset in the SGPR offset — into one of
// NBUF staging buffers, NBUF - 1 groups ahead of the group being converted: the DMA of several groups
// is in flight while the workgroup converts, which is what hides HBM latency when the frames stream
// from HBM rather than from the Infinity Cache. Taps are then LDS byte reads with immediate slot
// offsets, so neither the staging nor the gather costs VALU address arithmetic, and VMEM carries only
// wide loads and the planar stores. The DMA and the stores share vmcnt, which retires in issue order:
// every wave counts the VMEM operations it issues (all its branches are wave-uniform, so the count is
// exact) and waits for group g with vmcnt(operations issued after group g's DMA), so stores and later
// groups' DMA stay in flight.
template <int FMT, int OUT, int R, int NSEGX, int NBUF>
__global__ __launch_bounds__(kThreads) void evam_pp_staged(const SParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using T = FmtTraits<FMT>;
    constexpr bool kYUV = FMT == kNV12 || FMT == kI420;
    constexpr int NP = FMT == kI420 ? 3 : (FMT == kNV12 ? 2 : 1);  // staged planes
    constexpr int NS = 2 * R * NP;                                   // slots per staging buffer
    constexpr int SPW = NSEGX > 4 ? NSEGX / 4 : 1;                   // column segments per wave
    constexpr int RSTEP = NSEGX >= 4 ? 1 : 4 / NSEGX;                // waves sharing a column segment
    constexpr int RPW = R / RSTEP;                                   // rows per wave per group
    static_assert(NSEGX <= 4 && NBUF == 2, "retired shapes (round 5): full-width tiles, 2 KB slots, 3 buffers");
    constexpr int SLOT_MAX = kSlot;                                  // largest staged row segment
    const int SLOT = P.slot_bytes;                                   // this launch's segment (<= SLOT_MAX)
    static_assert(R % RSTEP == 0, "R must be a multiple of 4 / NSEGX");
    static_assert(NSEGX <= 4 || R == 1, "full-width (2 KB slot) tiles stage one row per group");
    static_assert(NBUF >= 2 && NBUF <= 3, "2 or 3 staging buffers");
    constexpr int TW = 64 * NSEGX;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Prologue critical path: the launch parameters, then (in parallel) the item's arguments, the tile's
    // row table and its column footprint (from the parameters when tiles_x <= kTCols), then the first
    // DMA. Two batches of scalar loads, one wait each: (1) the launch parameters, (2) the item's
    // arguments and the tile column's footprint (the row table's vector load goes out between them).
    // Without the empty asm uses, branches on parameters split the loads into ~6 dependent round trips
    // before the first DMA (C2 +0.5 to +3 %, C5 +0.4 to +1.4 %: profiles/r02zz_prologue_batch_ab.txt).
    const int p_xcd = P.xcd_remap, p_tpi = P.tiles_per_item, p_tx = P.tiles_x, p_TH = P.TH, p_DH = P.DH;
    const int p_grid = gridDim.x;
    asm volatile("" ::"s"(p_xcd), "s"(p_tpi), "s"(p_tx), "s"(p_TH), "s"(p_DH), "s"(p_grid), "s"(P.ytab), "s"(P.ox),
                 "s"(P.rw), "s"(P.slot_bytes), "s"(P.offBuf), "s"(P.color_rgb), "s"(P.DW),
                 "s"(P.ntcol));
    const int t_x = xcd_tile(blockIdx.x, p_grid);
    const int t = p_xcd ? t_x : (int)blockIdx.x;
    const int item = t / p_tpi;
    const int tile = t - item * p_tpi;
    const int ty = tile / p_tx;
    const int tx = tile - ty * p_tx;
    const int Y0 = ty * p_TH, Y1 = min(Y0 + p_TH, p_DH);
    const int rows = Y1 - Y0;
    // The tile's row table (<= 64 rows, host-checked), one row per lane in every wave: per-group lookups
    // are v_readlane instead of dependent scalar loads from L2 (~1 us per group in the loop's critical
    // path when the frames stream from HBM, profiles/r02_skeleton.txt).
    LaneRows lr;
    lr.load(P.ytab, Y0, rows, lane);
    const ItemArg& it = P.items[item];
    const __attribute__((address_space(4))) XTab* xtab_s = (const __attribute__((address_space(4))) XTab*)(P.xtab);
    const uint8_t* p0 = it.plane[0];
    const uint8_t* p1 = it.plane[1];
    const uint8_t* p2 = it.plane[2];
    const int pitch0 = it.pitch[0], pitch1 = it.pitch[1], pitch2 = it.pitch[2];
    const int x0 = it.x0, y0 = it.y0, ox = P.ox, rw = P.rw;
    const ColSpan tc = P.tcol[min(tx, kTCols - 1)];
    const int p_ntcol = P.ntcol, p_index = it.index;
    asm volatile("" ::"s"(p0), "s"(p1), "s"(p2), "s"(pitch0), "s"(pitch1), "s"(pitch2), "s"(x0), "s"(y0),
                 "s"(p_index), "s"(tc.x), "s"(tc.y), "s"(P.dst), "s"(P.slot_offset), "s"(P.slot_stride));
    const size_t plane = (size_t)P.DW * P.DH;
    const size_t esz = OUT == 1 ? 4 : 1;
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)(P.slot_offset + it.index * P.slot_stride) * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p1 ? p1 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(p2 ? p2 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    // plane of source channel 0 / 2 (B / R): swapped for RGB order
    const __amdgpu_buffer_rsrc_t rsD0 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.color_rgb ? d2 : d0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD1 = __builtin_amdgcn_make_buffer_rsrc((void*)d1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD2 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.color_rgb ? d0 : d2), (short)0, 0x7FFFFFFF, 0x00020000);

    float* lut_s = reinterpret_cast<float*>(smem);
    // fill in source channel order (P.fill is in output plane order); fp32: LUT byte offsets
    const uint32_t fq0 = P.fill & 0xFF, fq1 = (P.fill >> 8) & 0xFF, fq2 = (P.fill >> 16) & 0xFF;
    const uint32_t fsh = OUT == 1 ? 2 : 0;
    const uint32_t fillv[3] = {(P.color_rgb ? fq2 : fq0) << fsh, fq1 << fsh, (P.color_rgb ? fq0 : fq2) << fsh};

    const int X0 = tx * TW;
    const int rph = NSEGX >= 4 ? 0 : wave / NSEGX;
    // visible (non-padding) columns of the tile -> source footprint (wave-uniform)
    const int Xv0 = max(X0, ox), Xv1 = min(min(X0 + TW, P.DW), ox + rw) - 1;
    const bool cols = Xv0 <= Xv1;
    int fsY = 0, nY = 0, fsC = 0, nC = 0;
    if (cols) {
        int s0, s1;
        if (tx < p_ntcol) { s0 = tc.x; s1 = tc.y; }
        else { s0 = xtab_s[Xv0].s0; s1 = xtab_s[Xv1].s1; }
        footprint_chunks(FMT, T::bpp, x0 + s0, x0 + s1, fsY, nY, fsC, nC);
    }
    if (kAblate & 128) return;  // diagnostics: prologue parameters only
    // per-lane column state for each of this wave's SPW 64-column segments (seg = wave + 4 j, or
    // wave % NSEGX for narrow tiles), filled once the first DMA is in flight: LDS byte offsets of the taps
    // inside a slot, weights
    int X[SPW];
    bool xin[SPW], wave_stores[SPW];  // wave_stores: lane 0 of this wave stores segment j (wave-uniform)
    uint32_t lY0[SPW], lY1[SPW], lC0[SPW], lC1[SPW], wa[SPW], wp[SPW], xo[SPW];  // wp: a0 | a1 << 16, plain
#pragma unroll
    for (int j = 0; j < SPW; j++) {
        const int seg = NSEGX >= 4 ? wave + 4 * j : wave % NSEGX;
        X[j] = X0 + seg * 64 + lane;
        xin[j] = X[j] < P.DW;
        wave_stores[j] = X0 + seg * 64 < P.DW;
        xo[j] = (uint32_t)(xin[j] ? X[j] : 0) * (uint32_t)esz;
        lY0[j] = lY1[j] = lC0[j] = lC1[j] = wa[j] = wp[j] = 0;
    }
    const int ngroups = (rows + R - 1) / R;
    // letterbox padding columns anywhere in this tile (the per-pixel fill select is skipped otherwise)
    const bool anypadc = Xv0 > X0 || Xv1 < min(X0 + TW, P.DW) - 1;

    // ---- LDS-DMA of group g into buffer `buf` (slot s = plane * 2R + 2 * row + tap) ----
    // Returns the number of VMEM instructions this wave issued (wave-uniform; nY, nC >= 1 whenever
    // `cols`, so lane 0 is active in every issued instruction).
    // Static DMA roles: with 2R = 4 the (row, tap) pairs of a group are exactly the four waves, so wave
    // w stages row w >> 1, tap w & 1 of every plane. Otherwise the slots are dealt round-robin.
    const int dr = wave >> 1, dtap = wave & 1;
    auto issue = [&](int g, uint8_t* buf) -> int {
        if (!cols || (kAblate & 16)) return 0;
        if constexpr (2 * R == 4) {
            const int Y = Y0 + g * R + dr;
            if (Y >= Y1) return 0;
            const int b0 = lr.B0(Y - Y0), b1 = lr.B1(Y - Y0);
            if ((b0 | b1) == 0) return 0;  // padding row: nothing to stage
            const int ya = y0 + lr.R0(Y - Y0), yb = y0 + lr.R1(Y - Y0);
            const int yr = dtap ? yb : ya;
            int n = 0;
#pragma unroll
            for (int c0 = 0; c0 < SLOT_MAX / 16; c0 += 64) {  // one wave-wide 1 KB DMA per 64 chunks
                if (c0 >= nY) break;
                if (lane + c0 < nY)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        rsY, (__attribute__((address_space(3))) void*)(buf + wave * SLOT + c0 * 16), 16, (lane + c0) * 16,
                        yr * pitch0 + fsY, EVAM_PP_LOAD_AUX, 0);
                n++;
            }
            if constexpr (NP >= 2) {
                if (dtap && (ya >> 1) == (yb >> 1)) return n;  // chroma row shared by both taps
#pragma unroll
                for (int c0 = 0; c0 < SLOT_MAX / 16; c0 += 64) {
                    if (c0 >= nC) break;
                    if (lane + c0 < nC) {
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(
                            rsC, (__attribute__((address_space(3))) void*)(buf + (2 * R + wave) * SLOT + c0 * 16), 16,
                            (lane + c0) * 16, (yr >> 1) * pitch1 + fsC, EVAM_PP_LOAD_AUX, 0);
                        if constexpr (NP >= 3)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                                rsV, (__attribute__((address_space(3))) void*)(buf + (4 * R + wave) * SLOT + c0 * 16), 16,
                                (lane + c0) * 16, (yr >> 1) * pitch2 + fsC, EVAM_PP_LOAD_AUX, 0);
                    }
                    n += NP - 1;
                }
            }
            return n;
        } else {
            int n = 0;
#pragma unroll
            for (int s0 = 0; s0 < NS; s0 += 4) {
                const int s = s0 + wave;
                if (s >= NS) continue;
                const int pl = s / (2 * R), loc = s - pl * 2 * R, r = loc >> 1, tap = loc & 1;
                const int Y = Y0 + g * R + r;
                if (Y >= Y1) continue;
                const int b0 = lr.B0(Y - Y0), b1 = lr.B1(Y - Y0);
                if ((b0 | b1) == 0) continue;  // padding row: nothing to stage
                const int ya = y0 + lr.R0(Y - Y0), yb = y0 + lr.R1(Y - Y0);
                const int yr = tap ? yb : ya;
                if (pl > 0 && tap && (ya >> 1) == (yb >> 1)) continue;  // chroma row shared by both taps
                const int nck = pl == 0 ? nY : nC;
#pragma unroll
                for (int c0 = 0; c0 < SLOT_MAX / 16; c0 += 64) {  // one wave-wide 1 KB DMA per 64 chunks
                    if (c0 >= nck) break;
                    __attribute__((address_space(3))) void* dstl =
                        (__attribute__((address_space(3))) void*)(buf + s * SLOT + c0 * 16);
                    if (lane + c0 < nck) {
                        const int co = (lane + c0) * 16;
                        if (pl == 0)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, dstl, 16, co, yr * pitch0 + fsY, EVAM_PP_LOAD_AUX, 0);
                        else if (pl == 1)
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsC, dstl, 16, co, (yr >> 1) * pitch1 + fsC, EVAM_PP_LOAD_AUX, 0);
                        else
                            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, dstl, 16, co, (yr >> 1) * pitch2 + fsC, EVAM_PP_LOAD_AUX, 0);
                    }
                    n++;
                }
            }
            return n;
        }
    };

    // ---- convert + resize + normalise + store the rows of group g owned by this wave ----
    // Channel routing: v[c] holds source channel c (B, G, R). It is stored to output plane c, or 2 - c for
    // RGB order, through swapped plane resources; the LDS LUT is loaded with its sections in source
    // channel order (prologue), so the per-pixel path carries no swap. For fp32 output the vertical
    // pass yields 4 * v, the LUT byte offset, directly ((x + 2) & ~3 instead of (x + 2) >> 2).
    // Returns the number of stores this wave issued: 3 per owned row when the wave stores at all (the
    // padding-column select is branchless, so every storing row issues exactly three).
    auto compute = [&](int g, const uint8_t* buf) -> int {
        int n = 0;
#pragma unroll
        for (int kj = 0; kj < RPW * SPW; kj++) {
            const int k = kj / SPW, j = kj % SPW;
            const int r = rph + k * RSTEP;
            const int Y = Y0 + g * R + r;
            if (Y >= Y1 || !wave_stores[j]) continue;
            const int b0 = lr.B0(Y - Y0), b1 = lr.B1(Y - Y0);
            const int sO = (int)((uint32_t)(Y * P.DW) * (uint32_t)esz);
            n += 3;
            auto put = [&](const uint32_t (&v)[3]) {
                if (kAblate & 4) {
                    asm volatile("" :: "v"(v[0]), "v"(v[1]), "v"(v[2]));
                    return;
                }
                if (!xin[j]) return;  // lane 0 is in: the wave still issues all three stores
                if constexpr (OUT == 1) {
                    const uint8_t* lb = reinterpret_cast<const uint8_t*>(lut_s);
                    __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t*>(lb + v[0]), rsD0, xo[j], sO, EVAM_PP_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t*>(lb + 1024 + v[1]), rsD1, xo[j], sO, EVAM_PP_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b32(*reinterpret_cast<const uint32_t*>(lb + 2048 + v[2]), rsD2, xo[j], sO, EVAM_PP_STORE_AUX);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[0], rsD0, xo[j], sO, EVAM_PP_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[1], rsD1, xo[j], sO, EVAM_PP_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[2], rsD2, xo[j], sO, EVAM_PP_STORE_AUX);
                }
            };
            if ((b0 | b1) == 0 || (kAblate & 2)) {  // padding row (wave-uniform)
                put(fillv);
                continue;
            }
            const bool padc = wa[j] == 0;  // letterbox padding column: taps at valid offsets, value replaced
            const uint32_t wb0 = (uint32_t)b0, wb1 = (uint32_t)b1;
            const uint8_t* sy0 = buf + (2 * r) * SLOT;
            const uint8_t* sy1 = sy0 + SLOT;
            const uint8_t* sc0 = buf + (2 * R + 2 * r) * SLOT;
            const uint32_t lY0j = lY0[j], lY1j = lY1[j], lC0j = lC0[j], lC1j = lC1[j], wpj = wp[j];
            uint32_t v[3];
            if constexpr (kYUV) {
                const int ya = y0 + lr.R0(Y - Y0), yb = y0 + lr.R1(Y - Y0);
                const bool share = (ya >> 1) == (yb >> 1);
                const uint8_t* sc1 = share ? sc0 : sc0 + SLOT;
                // NV12: U and V of a tap are adjacent bytes of the staged UV row; I420: same offset in the
                // U and V slots.
                const uint8_t* sv0 = FMT == kNV12 ? sc0 + 1 : sc0 + 2 * R * SLOT;
                const uint8_t* sv1 = FMT == kNV12 ? sc1 + 1 : sc1 + 2 * R * SLOT;
                const UVs tA = uv_terms_sat(sc0[lC0j], sv0[lC0j]);
                const UVs tB = uv_terms_sat(sc0[lC1j], sv0[lC1j]);
                const uint32_t yA = luma_term(sy0[lY0j]), yB = luma_term(sy0[lY1j]);
                const uint32_t yC = luma_term(sy1[lY0j]), yD = luma_term(sy1[lY1j]);
                const uint32_t h0[3] = {hpass_sat(yA, tA.b, yB, tB.b, wpj), hpass_sat(yA, tA.g, yB, tB.g, wpj),
                                        hpass_sat(yA, tA.r, yB, tB.r, wpj)};
                uint32_t h1[3];
                // both vertical taps in one chroma row (wave-uniform, ~half the rows of a 2:1 chroma
                // downscale): its terms are reused instead of read and converted again. The second row's
                // horizontal pass is written out in both branches, so the shared path carries no copies of
                // the chroma terms.
                if (share) {
                    h1[0] = hpass_sat(yC, tA.b, yD, tB.b, wpj);
                    h1[1] = hpass_sat(yC, tA.g, yD, tB.g, wpj);
                    h1[2] = hpass_sat(yC, tA.r, yD, tB.r, wpj);
                } else {
                    const UVs tC = uv_terms_sat(sc1[lC0j], sv1[lC0j]);
                    const UVs tD = uv_terms_sat(sc1[lC1j], sv1[lC1j]);
                    h1[0] = hpass_sat(yC, tC.b, yD, tD.b, wpj);
                    h1[1] = hpass_sat(yC, tC.g, yD, tD.g, wpj);
                    h1[2] = hpass_sat(yC, tC.r, yD, tD.r, wpj);
                }
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = vfinal<OUT>(h0[c], h1[c], wb0, wb1);
                if (anypadc) {  // wave-uniform: most launches have no padding column at all (C2, C4, C5)
#pragma unroll
                    for (int c = 0; c < 3; c++) v[c] = padc ? fillv[c] : v[c];
                }
                put(v);
                continue;
            }
            const uint32_t a0 = wa[j] & 0xFFFF, a1 = wa[j] >> 16;  // 15-bit
            int c[4][3];
            {  // packed sources (BGRx / BGR)
                const uint8_t* rowp[2] = {sy0, sy1};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint8_t* sp = rowp[q >> 1] + ((q & 1) ? lY1j : lY0j);
                    if constexpr (FMT == kBGRX) {
                        const uint32_t px = *reinterpret_cast<const uint32_t*>(sp);
                        c[q][0] = px & 0xFF; c[q][1] = (px >> 8) & 0xFF; c[q][2] = (px >> 16) & 0xFF;
                    } else {
                        c[q][0] = sp[0]; c[q][1] = sp[1]; c[q][2] = sp[2];
                    }
                }
            }
#pragma unroll
            for (int ch3 = 0; ch3 < 3; ch3++) {
                const uint32_t D0 = __umul24(c[0][ch3], a0) + __umul24(c[1][ch3], a1);
                const uint32_t D1 = __umul24(c[2][ch3], a0) + __umul24(c[3][ch3], a1);
                v[ch3] = padc ? fillv[ch3] : vfinal<OUT>(D0, D1, wb0, wb1);
            }
            put(v);
        }
        return n;
    };

    uint8_t* const bufs = smem + P.offBuf;
    // Prologue: the first NBUF - 1 groups' DMA goes out before the LUT and column-table loads, so their
    // latencies overlap instead of adding up. q[j]: VMEM operations issued up to the end of the DMA of
    // group g + j (j < NBUF - 1), for the counted waits below.
    int issued = 0;
    int q[NBUF - 1];
#pragma unroll
    for (int j = 0; j < NBUF - 1; j++) {
        if (j < ngroups) issued += __builtin_amdgcn_readfirstlane(issue(j, bufs + j * P.buf_bytes));
        q[j] = issued;
    }
    asm volatile("" ::: "memory");
    if constexpr (OUT == 1) {  // sections in source channel order (B, G, R): see compute
        if (!(kAblate & 32))   // diagnostics: 32 skips the LUT load
            for (int i = tid; i < 768; i += kThreads) lut_s[i] = P.lut[P.color_rgb ? 512 - (i & ~255) + (i & 255) : i];
    }
#pragma unroll
    for (int j = 0; j < SPW; j++) {
        const XTab xt = P.xtab[xin[j] ? X[j] : 0];
        wa[j] = (uint32_t)xt.a0 | ((uint32_t)xt.a1 << 16);
        wp[j] = (wa[j] >> 4) & 0x0FFF0FFFu;
        if (xin[j] && wa[j] != 0) {
            const int ca = x0 + xt.s0, cb = x0 + xt.s1;
            lY0[j] = (uint32_t)(ca * T::bpp - fsY);
            lY1[j] = (uint32_t)(cb * T::bpp - fsY);
            lC0[j] = FMT == kNV12 ? (uint32_t)(2 * (ca >> 1) - fsC) : (uint32_t)((ca >> 1) - fsC);
            lC1[j] = FMT == kNV12 ? (uint32_t)(2 * (cb >> 1) - fsC) : (uint32_t)((cb >> 1) - fsC);
        }
    }
    int bi = 0;                 // buffer of group g
    int bn = NBUF - 1;          // buffer of group g + NBUF - 1
    if ((kAblate & 64) && ngroups != -7) {  // diagnostics: prologue only
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" :: "v"(lY0[0]), "v"(lC0[0]), "v"(wa[0]), "v"(lY1[0]), "v"(lC1[0]));
        return;
    }
    // Stores this wave issues for a full group (3 per owned row; the padding select is branchless).
    int st_full = 0;
#pragma unroll
    for (int j = 0; j < SPW; j++) st_full += wave_stores[j] ? 3 * RPW : 0;
    st_full = __builtin_amdgcn_readfirstlane(st_full);
    for (int g = 0; g < ngroups; g++) {
        // This wave's share of group g's DMA landed; everything issued after it (later groups' DMA, the
        // previous groups' stores) may stay in flight. The first iteration also covers the prologue's
        // global loads (LUT, column table), which were issued after the DMA.
        if (g == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if constexpr (NBUF == 2) {
            // Two buffers: only the stores of group g - 1 (a full group: group g exists) were issued
            // after group g's DMA, and their count is a per-wave constant, so the wait is one
            // immediate, not the counted ladder (scalar instructions are shared by the CU's waves).
            if (st_full == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (SPW == 1 || st_full == 3 * RPW) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(3 * RPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 * RPW) : "memory");
        } else {
            vmcnt_at_most(issued - q[0]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave's DMA for g landed; every wave done reading g-1
#pragma unroll
        for (int j = 0; j + 1 < NBUF - 1; j++) q[j] = q[j + 1];
        if (g + NBUF - 1 < ngroups) issued += __builtin_amdgcn_readfirstlane(issue(g + NBUF - 1, bufs + bn * P.buf_bytes));
        q[NBUF - 2] = issued;
        asm volatile("" ::: "memory");  // the next groups' DMA stays ahead of this group's stores
        issued += __builtin_amdgcn_readfirstlane(compute(g, bufs + bi * P.buf_bytes));
        asm volatile("" ::: "memory");
        bi = bi + 1 == NBUF ? 0 : bi + 1;
        bn = bn + 1 == NBUF ? 0 : bn + 1;
    }
}

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

#include "evam_strip_kernels.h"
#include "evam_band_kernels.h"

namespace {

template <int N>
__device__ __forceinline__ void wait_vmcnt_stores(int nk) {
    // s_waitcnt takes an immediate: vmcnt(N * nk) for the wave-uniform store-step count nk.
    switch (nk) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * N) : "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(3 * N) : "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * N) : "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(5 * N) : "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 * N) : "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(7 * N) : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(%0)" :: "n"(8 * N) : "memory"); break;
    }
}

// Staged kernel for batches whose items differ in geometry (gvaclassify ROI batches, mixed crops).
// The host passes the caller's raw ROI array; each workgroup resolves its item's crop, resized size
// and placement on the device (roi_geometry, the host's own rules) and owns all DW columns x TH rows
// of that item:
//  * OpenCV coefficient tables for its columns / rows are built in LDS (exact double/float sequence);
//  * rows are walked in groups whose size R adapts to the item: as many output rows as the staging
//    buffer holds for this crop's width (narrow crops: many rows per group, few barriers), capped so
//    the R x DW pixels cover the 256 lanes at most kRoiK times;
//  * a group's source row segments (luma taps and chroma taps, each exactly the item's footprint)
//    are packed back to back in LDS and arrive by LDS-DMA while the previous group is converted;
//  * the group's R x DW output pixels are packed densely onto the lanes (pixel p = tid + 256 k), so a
//    72-wide classifier row keeps every lane busy and every store is row-contiguous.
// 7 resident workgroups per CU need <= 96 SGPRs (800 / (96 + 16)); the occupancy API does not count
// SGPRs (MI355X_MICROARCH.md, Residency): uncapped, the kernel's ~106 allowed only 6 and a 1,600-ROI
// batch ran a second round (profiles/r02r_c3_roi_timeline_before.json).
// DEV (evam_pp_run_device_rois): the records were written by evam_pp_roi_records from a device-resident ROI list, one
// per (list entry, row tile) of the list's capacity; a record with an empty row range (an entry past the list's count,
// or an invalid one) ends its workgroup before any DMA is issued. A sibling instantiation: DEV = false compiles to the
// code it had before the parameter existed.
template <int FMT, int OUT, int PX, int NB, bool DEV = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_num_sgpr(96))) void evam_pp_roi(const QParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    static_assert(NB == 2, "two staging buffers (three were retired in round 5)");
    using T = FmtTraits<FMT>;
    constexpr bool kYUV = FMT == kNV12 || FMT == kI420;
    constexpr int NP = FMT == kI420 ? 3 : (FMT == kNV12 ? 2 : 1);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the parameters of the prologue in one batch of scalar loads, so the record's PCIe read below is not
    // queued behind a kernarg round trip for the diagnostics test
    asm volatile("" ::"s"(P.recs), "s"(P.lut), "s"(P.color_rgb), "s"(P.mode), "s"(P.placement),
                 "s"(P.DW), "s"(P.DH));
    if (kAblate & 128) return;  // diagnostics: launch cost only
    EVAM_STAMP(0);
    // The whole 64-byte record in one scalar load, issued first (field-by-field loads became up to three
    // dependent round trips per wave). The record slot is device memory the host wrote through its BAR
    // mapping (PinRing, HipRings::pinned_alloc), or pinned host memory read over PCIe where the platform does
    // not map device memory (~1-2 us more under load). Its latency overlaps the LUT load below.
    typedef unsigned int u32x16 __attribute__((ext_vector_type(16)));
    const u32x16 rec = *((const __attribute__((address_space(4))) u32x16*)(P.recs) + blockIdx.x);
    if constexpr (DEV) {
        if ((rec[15] >> 16) <= (rec[15] & 0xFFFF)) return;  // no rows: nothing issued yet, the LDS is untouched
    }
    // The LUT by LDS-DMA, issued first: no VGPR waits on it, and group 0's wait (everything older than its
    // DMA) covers it. Loaded into registers and stored it held the row-table barrier, and so the first DMA,
    // up to ~15 us for the last workgroups behind the chip's first DMA burst (profiles/r03l_c3_roi_timeline.json).
    // Sections in source channel order (B, G, R): RGB output swaps the B / R output planes instead of the
    // values (see rsD0 / rsD2), so the per-pixel path carries no swap.
    float* lut_s = reinterpret_cast<float*>(smem);
    if constexpr (OUT != 0) {
        const int c0 = wave * 48, c = c0 + lane, sec = c >> 6;  // 192 chunks of 16 B: 48 per wave
        const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc((void*)P.lut, (short)0, 3072, 0x00020000);
        if (lane < 48)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsL, (__attribute__((address_space(3))) void*)(smem + c0 * 16), 16,
                                                     (uint32_t)(((P.color_rgb ? 2 - sec : sec) * 64 + (c & 63)) * 16), 0, 0, 0);
    }
    // RoiRec as dwords: plane[0..2] 0-5, pitch[0..2] 6-8, width | height << 16 9, x y w h 10-13, item 14,
    // row0 | row1 << 16 15
    static_assert(offsetof(RoiRec, pitch) == 24 && offsetof(RoiRec, width) == 36 && offsetof(RoiRec, x) == 40 &&
                  offsetof(RoiRec, item) == 56 && offsetof(RoiRec, row0) == 60, "RoiRec dword map");
    auto ptr_of = [](unsigned lo, unsigned hi) {
        return reinterpret_cast<const uint8_t*>(((uint64_t)hi << 32) | lo);
    };
    const int item = (int)rec[14];
    const uint32_t wh = rec[9];
    const uint32_t rr01 = rec[15];
    const int fw = wh & 0xFFFF, fh = wh >> 16;
    const int rx = (int)rec[10], ry = (int)rec[11], rwd = (int)rec[12], rht = (int)rec[13];
    const uint8_t* p0 = ptr_of(rec[0], rec[1]);
    const uint8_t* p1 = ptr_of(rec[2], rec[3]);
    const uint8_t* p2 = ptr_of(rec[4], rec[5]);
    const int pitch0 = (int)rec[6], pitch1 = (int)rec[7], pitch2 = (int)rec[8];
    Geom g;
    roi_geometry(FMT, fw, fh, true, rx, ry, rwd, rht, P.mode, P.placement, P.DW, P.DH,
                 g);  // never empty: the host validated every item
    const int x0 = __builtin_amdgcn_readfirstlane(g.x0), y0 = __builtin_amdgcn_readfirstlane(g.y0);
    const int cw = __builtin_amdgcn_readfirstlane(g.cw), ch = __builtin_amdgcn_readfirstlane(g.ch);
    const int rw = __builtin_amdgcn_readfirstlane(g.rw), rh = __builtin_amdgcn_readfirstlane(g.rh);
    const int ox = __builtin_amdgcn_readfirstlane(g.ox), oy = __builtin_amdgcn_readfirstlane(g.oy);
    EVAM_STAMP(1);
    // diagnostics: stop after the geometry (64) / after the per-lane setup (32)
    if ((kAblate & 64) && rw != -7) return;
    const double scx = 1. / ((double)rw / cw), scy = 1. / ((double)rh / ch);
    const size_t plane = (size_t)P.DW * P.DH;
    const size_t esz = out_esz(OUT);
    const int slot = P.slot_offset + item * P.slot_stride;
    uint8_t* const d0 = reinterpret_cast<uint8_t*>(P.dst) + (size_t)slot * 3 * plane * esz;
    uint8_t* const d1 = d0 + plane * esz;
    uint8_t* const d2 = d1 + plane * esz;
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p0, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p1 ? p1 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(p2 ? p2 : p0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD0 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.color_rgb ? d2 : d0), (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD1 = __builtin_amdgcn_make_buffer_rsrc((void*)d1, (short)0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD2 = __builtin_amdgcn_make_buffer_rsrc((void*)(P.color_rgb ? d0 : d2), (short)0, 0x7FFFFFFF, 0x00020000);

    // Prologue order: the row table is built first; group 0's DMA (it needs only the row table and the
    // analytic footprint) goes out before the column table and the per-lane setup are built, so its
    // latency overlaps them. The column table holds each column's packed tap offsets into the staged rows and
    // weights (lY, lC, wa: what every lane reading the column needs), so the per-lane setup is table reads.
    uint4* ct = reinterpret_cast<uint4*>(smem + P.offXT);
    YTab* yt = reinterpret_cast<YTab*>(smem + P.offYT);
    const int DW = P.DW;
    const int Y0 = __builtin_amdgcn_readfirstlane(rr01 & 0xFFFF), Y1 = __builtin_amdgcn_readfirstlane(rr01 >> 16);
    const int rows = Y1 - Y0;
    for (int ly = tid; ly < rows; ly += kThreads) {
        YTab e;
        e.r0 = 0; e.r1 = 0; e.b0 = 0; e.b1 = 0;
        const int dy = Y0 + ly - oy;
        if (dy >= 0 && dy < rh) {
            int sy, b0, b1;
            linear_coef(dy, scy, ch, false, sy, b0, b1);
            e.r0 = min(max(sy, 0), ch - 1);
            e.r1 = min(max(sy + 1, 0), ch - 1);
            e.b0 = b0 << 8;
            e.b1 = b1 << 8;
        }
        yt[ly] = e;
    }
    int fsY, nY, fsC, nC;
    item_footprint(FMT, T::bpp, x0, cw, rw, ox, scx, DW, fsY, nY, fsC, nC);
    fsY = __builtin_amdgcn_readfirstlane(fsY);
    nY = __builtin_amdgcn_readfirstlane(nY);
    fsC = __builtin_amdgcn_readfirstlane(fsC);
    nC = __builtin_amdgcn_readfirstlane(nC);
    // Staging buffer layout for a group of R output rows, one plane region after the other:
    //   Y: segment (2 r + tap) at (2 r + tap) * segY;   C (U / UV): at offC + (2 r + tap) * segC;
    //   V (I420): at offC + 2 R segC + (2 r + tap) * segC.
    // Each plane region is contiguous, so its 16-byte chunks are staged by wave-wide LDS-DMA with one
    // per-lane source offset each: 64 chunks (of any rows and taps) per instruction.
    const int segY = nY * 16, segC = nC * 16;
    const int rowb = 2 * segY + 2 * (NP - 1) * segC;
    // Lanes own runs of PX adjacent pixels of one row (DW % PX == 0, host): a "quad" q of the
    // group's R x QW quads covers row q / QW, columns PX * (q % QW) ...
    constexpr int KQ = kRoiK / PX;                // max quads per lane per group
    const int QW = DW / PX;
    int R = rowb > 0 ? P.buf_bytes / rowb : rows;
    R = min(R, (KQ * kThreads) / QW);
    R = max(1, min(R, rows));
    const int offC = 2 * R * segY;
    const int nq = R * QW;                        // quads per full group
    const int K = (nq + kThreads - 1) / kThreads;
    // store steps this wave issues in a full group: k with some lane of the wave holding a quad
    int nk_w = 0;
    for (int k = 0; k < K; k++) nk_w += (k * kThreads + wave * 64 < nq) ? 1 : 0;
    // q / n for q < 2^16 by one mul_hi: m = ceil(2^32 / n) is exact there (n = 1: the identity).
    const uint32_t mY = nY > 1 ? (uint32_t)((0x100000000ull + nY - 1) / nY) : 0u;
    const uint32_t mC = nC > 1 ? (uint32_t)((0x100000000ull + nC - 1) / nC) : 0u;
    // Row table visible: LDS writes only (lgkmcnt) and a raw barrier. __syncthreads() would add vmcnt(0) and
    // hold every wave until the LUT's LDS-DMA landed; group 0's wait below covers the LUT instead.
    lds_barrier();
    EVAM_STAMP(8);
    // One plane region of group grp: chunk q -> (segment, chunk) -> (row, tap) -> source offset.
    // Returns the number of DMA instructions this wave issued (wave-uniform: an instruction with no active
    // lane is skipped), for the counted waits of the three-buffer pipeline.
    auto issue_plane = [&](int grp, uint8_t* base, int nr, int n, uint32_t m, int pl) -> int {
        const int nq = 2 * nr * n;
        int cnt = 0;
        for (int q0 = wave * 64; q0 < nq; q0 += 4 * 64) {
            const int q = q0 + lane;
            const int seg = n > 1 ? (int)__umulhi((uint32_t)q, m) : q;
            const int c = q - seg * n;
            const int r = seg >> 1, tap = seg & 1;
            const YTab e = yt[min(grp * R + r, rows - 1)];
            const int ya = y0 + e.r0, yb = y0 + e.r1;
            bool on = q < nq && (e.b0 | e.b1) != 0;           // padding rows stage nothing
            if (pl > 0) on = on && !(tap && (ya >> 1) == (yb >> 1));  // chroma row shared by both taps
            __attribute__((address_space(3))) void* dstl = (__attribute__((address_space(3))) void*)(base + q0 * 16);
            if (on) {
                const int yr = tap ? yb : ya;
                if (pl == 0)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsY, dstl, 16, yr * pitch0 + fsY + c * 16, 0, EVAM_PP_LOAD_AUX, 0);
                else if (pl == 1)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsC, dstl, 16, (yr >> 1) * pitch1 + fsC + c * 16, 0, EVAM_PP_LOAD_AUX, 0);
                else
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, dstl, 16, (yr >> 1) * pitch2 + fsC + c * 16, 0, EVAM_PP_LOAD_AUX, 0);
            }
        }
        return cnt;
    };
    auto issue = [&](int grp, uint8_t* buf) -> int {
        if (nY == 0 || (kAblate & 16)) return 0;  // no visible columns: every pixel is fill
        const int nr = min(R, rows - grp * R);
        int cnt = issue_plane(grp, buf, nr, nY, mY, 0);
        if constexpr (NP >= 2) cnt += issue_plane(grp, buf + offC, nr, nC, mC, 1);
        if constexpr (NP >= 3) cnt += issue_plane(grp, buf + offC + 2 * R * segC, nr, nC, mC, 2);
        return __builtin_amdgcn_readfirstlane(cnt);
    };
    uint8_t* const buf0 = smem + P.offBuf;
    uint8_t* const buf1 = buf0 + P.buf_bytes;
    issue(0, buf0);
    static_assert(sizeof(uint4) == sizeof(XTab), "column entries take the host's XTab carve");
    for (int X = tid; X < DW; X += kThreads) {
        uint4 e = {0u, 0u, 0u, 0u};  // (lY, lC, wa, 0); all 0: padding column
        const int dx = X - ox;
        if (dx >= 0 && dx < rw) {
            int sx, a0, a1;
            linear_coef(dx, scx, cw, true, sx, a0, a1);
            const int ca = x0 + sx, cb = x0 + min(sx + 1, cw - 1);
            e.x = (uint32_t)(ca * T::bpp - fsY) | ((uint32_t)(cb * T::bpp - fsY) << 16);
            if constexpr (FMT == kNV12)
                e.y = (uint32_t)(2 * (ca >> 1) - fsC) | ((uint32_t)(2 * (cb >> 1) - fsC) << 16);
            else if constexpr (FMT == kI420)
                e.y = (uint32_t)((ca >> 1) - fsC) | ((uint32_t)((cb >> 1) - fsC) << 16);
            e.z = ((uint32_t)a0 << 4) | ((uint32_t)a1 << 20);
        }
        ct[X] = e;
    }
    lds_barrier();  // column table visible to the per-lane setup; group 0's DMA stays in flight
    EVAM_STAMP(9);
    // fill in source channel order (P.fill is in output plane order); fp32: LUT byte offsets
    const uint32_t fsh = OUT != 0 ? 2 : 0;
    const uint32_t fq0 = P.fill & 0xFF, fq1 = (P.fill >> 8) & 0xFF, fq2 = (P.fill >> 16) & 0xFF;
    const uint32_t f0 = (P.color_rgb ? fq2 : fq0) << fsh, f1 = fq1 << fsh, f2 = (P.color_rgb ? fq0 : fq2) << fsh;
    // Per-lane state for quad steps k < K, identical for every group: row of the quad inside the
    // group; per pixel packed LDS tap offsets (tap 0 low, tap 1 high half) and horizontal weights.
    uint32_t lY[KQ][PX], lC[KQ][PX], wa[KQ][PX];
    int rr[KQ];
#pragma unroll
    for (int k = 0; k < KQ; k++) {
        const uint32_t q = (uint32_t)(tid + k * kThreads);  // < 2^16: mulhi by ceil(2^32 / QW) is q / QW exactly
        const bool v = k < K && (int)q < nq;
        const int r = v ? (QW > 1 ? (int)__umulhi(q, P.mqw) : (int)q) : 0;
        const int c0 = v ? ((int)q - r * QW) * PX : 0;
        rr[k] = v ? r : -1;
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const uint4 e = ct[c0 + j];
            lY[k][j] = e.x;
            lC[k][j] = e.y;
            wa[k][j] = e.z;
        }
    }
    const int ngroups = (rows + R - 1) / R;
#ifdef EVAM_PP_TRACE
    {
        EVAM_STAMP(2);
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        EVAM_TRACE_VAL(4, (unsigned long long)cw | ((unsigned long long)ch << 32));
        EVAM_TRACE_VAL(5, (unsigned long long)ngroups | ((unsigned long long)R << 32));
        EVAM_TRACE_VAL(6, (unsigned long long)xcc | ((unsigned long long)hw << 32));
    }
#endif
    if ((kAblate & 32) && ngroups != -7) {
        asm volatile("" :: "v"(lY[0][0]), "v"(lC[0][0]), "v"(wa[0][0]), "v"(rr[0]), "s"(mY), "s"(mC));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // group 0's DMA lands before the LDS is released
        return;
    }

    auto compute = [&](int grp, const uint8_t* buf) {
        const uint32_t gbase = (uint32_t)((Y0 + grp * R) * DW);
#pragma unroll
        for (int k = 0; k < KQ; k++) {
            if (k >= K) break;
            const int ly = grp * R + rr[k];
            if (rr[k] < 0 || ly >= rows) continue;
            const YTab e = yt[ly];
            const bool padrow = (e.b0 | e.b1) == 0 || (kAblate & 2);  // letterbox padding row
            const uint8_t* sy0 = buf + 2 * rr[k] * segY;
            const uint8_t* sy1 = sy0 + segY;
            const uint8_t* sc0 = buf + offC + 2 * rr[k] * segC;
            const uint8_t* sc1 = sc0;
            if constexpr (kYUV) {
                const int ya = y0 + e.r0, yb = y0 + e.r1;
                sc1 = (ya >> 1) == (yb >> 1) ? sc0 : sc0 + segC;
            }
            const uint32_t wb0 = (uint32_t)e.b0, wb1 = (uint32_t)e.b1;
            uint32_t v[3][PX];  // source channel c (B, G, R); fp32: 4 x value, the LUT byte offset
#pragma unroll
            for (int j = 0; j < PX; j++) {
                if (padrow || wa[k][j] == 0) {  // padding row / column
                    v[0][j] = f0; v[1][j] = f1; v[2][j] = f2;
                    continue;
                }
                const uint32_t a0 = wa[k][j] & 0xFFFF, a1 = wa[k][j] >> 16;
                const uint32_t tY0 = lY[k][j] & 0xFFFF, tY1 = lY[k][j] >> 16;
                int c[4][3];
                if constexpr (kYUV) {
                    const uint32_t tC0 = lC[k][j] & 0xFFFF, tC1 = lC[k][j] >> 16;
                    const uint8_t* sv0 = FMT == kNV12 ? sc0 + 1 : sc0 + 2 * R * segC;
                    const uint8_t* sv1 = FMT == kNV12 ? sc1 + 1 : sc1 + 2 * R * segC;
                    const uint32_t wp = (wa[k][j] >> 4) & 0x0FFF0FFFu;
                    uint32_t H0[3], H1[3];
                    hrow_sat(sy0[tY0], sy0[tY1], uv_terms_sat(sc0[tC0], sv0[tC0]), uv_terms_sat(sc0[tC1], sv0[tC1]), wp, H0);
                    hrow_sat(sy1[tY0], sy1[tY1], uv_terms_sat(sc1[tC0], sv1[tC0]), uv_terms_sat(sc1[tC1], sv1[tC1]), wp, H1);
#pragma unroll
                    for (int ch3 = 0; ch3 < 3; ch3++) v[ch3][j] = vfinal<OUT>(H0[ch3], H1[ch3], wb0, wb1);
                    continue;
                }
                {  // packed sources (BGRx / BGR)
                    const uint8_t* tap[4] = {sy0 + tY0, sy0 + tY1, sy1 + tY0, sy1 + tY1};
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if constexpr (FMT == kBGRX) {
                            const uint32_t px = *reinterpret_cast<const uint32_t*>(tap[q]);
                            c[q][0] = px & 0xFF; c[q][1] = (px >> 8) & 0xFF; c[q][2] = (px >> 16) & 0xFF;
                        } else {
                            c[q][0] = tap[q][0]; c[q][1] = tap[q][1]; c[q][2] = tap[q][2];
                        }
                    }
                }
#pragma unroll
                for (int ch3 = 0; ch3 < 3; ch3++) {
                    const uint32_t D0 = __umul24(c[0][ch3], a0) + __umul24(c[1][ch3], a1);
                    const uint32_t D1 = __umul24(c[2][ch3], a0) + __umul24(c[3][ch3], a1);
                    v[ch3][j] = vfinal<OUT>(D0, D1, wb0, wb1);
                }
            }
            // soffset 0: the row offset is in voffset (a > 8-byte store with an SGPR soffset misses
            // the compiler's store-data hazard wait on gfx950, see evam_pp_wave)
            const uint32_t vo = (gbase + (uint32_t)(tid + k * kThreads) * PX) * (uint32_t)esz;
            if (kAblate & 4) {
                asm volatile("" :: "v"(v[0][0]), "v"(v[1][0]), "v"(v[2][0]));
                continue;
            }
            const uint8_t* lb = reinterpret_cast<const uint8_t*>(lut_s);
            store_off<OUT, PX>(rsD0, vo, lb, v[0]);
            store_off<OUT, PX>(rsD1, vo, lb + 1024, v[1]);
            store_off<OUT, PX>(rsD2, vo, lb + 2048, v[2]);
        }
    };


    // progress-based priority (EVAM_PP_PRIO): 3 -> 0 over the quarters of the workgroup's row groups
    ProgressPrio prio(P.prio != 0, ngroups);
    for (int grp = 0; grp < ngroups; grp++) {
        prio.step(grp);
        // Wait for this wave's share of group grp's DMA. Group grp-1 was full (only the last group can
        // be partial), so this wave issued at least 3 stores for each of its nk_w store steps after
        // that DMA: those may stay in flight.
        if (grp > 0) wait_vmcnt_stores<3>(nk_w);
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave's DMA for grp landed; every wave done reading grp-1
        if (grp == 0) EVAM_STAMP(10);
        if (grp + 1 < ngroups) issue(grp + 1, (grp & 1) ? buf0 : buf1);
        asm volatile("" ::: "memory");  // the next group's DMA stays ahead of this group's stores
        compute(grp, (grp & 1) ? buf1 : buf0);
        asm volatile("" ::: "memory");
    }
    EVAM_STAMP(3);
}

}  // namespace

#include "evam_rois_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(EVAM_PP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

int fmt_id(int fourcc) {
    switch (fourcc) {
    case EVAM_FOURCC_NV12: return kNV12;
    case EVAM_FOURCC_I420: return kI420;
    case EVAM_FOURCC_BGRX:
    case EVAM_FOURCC_BGRA: return kBGRX;
    case EVAM_FOURCC_BGR: return kBGR;
    default: return -1;
    }
}


int item_geometry(int f, int W, int H, const evam_roi* roi, const evam_preproc& cfg, int DW, int DH, Geom& g) {
    return roi_geometry(f, W, H, roi != nullptr, roi ? roi->x : 0, roi ? roi->y : 0, roi ? roi->w : 0,
                        roi ? roi->h : 0, cfg.resize_mode, cfg.placement, DW, DH, g);
}

void build_lut(const evam_preproc& cfg, float* lut) {
    const volatile float alpha = (float)(((double)cfg.range[1] - (double)cfg.range[0]) / 255.0);
    const volatile float beta = cfg.range[0];
    for (int c = 0; c < 3; c++)
        for (int u = 0; u < 256; u++) {
            volatile float v = (float)u;
            if (cfg.norm_flags & EVAM_NORM_RANGE) {
                volatile float m = v * alpha;
                v = m + beta;
            }
            if (cfg.norm_flags & EVAM_NORM_MEAN_STD) {
                volatile float s = v - cfg.mean[c];
                v = s / cfg.std[c];
            }
            lut[c * 256 + u] = v;
        }
}

// fp32 bits -> fp16 bits, round to nearest even, in integer arithmetic: subnormals, overflow to +-inf, NaN stays
// (quiet) NaN, the sign of zero is kept.
uint16_t f32_to_f16_bits(uint32_t x) {
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u | ((a >> 13) & 0x3FFu));
    if (a >= 0x38800000u) {  // >= 2^-14: a normal fp16, or past its range
        const uint32_t r = a - 0x38000000u;  // exponent bias 127 -> 15
        const uint32_t q = (r + 0xFFFu + ((r >> 13) & 1u)) >> 13;  // a mantissa carry moves into the exponent
        return (uint16_t)(sign | std::min(q, 0x7C00u));
    }
    const uint32_t e = a >> 23;
    if (e < 102) return (uint16_t)sign;  // < 2^-25: below half of the smallest subnormal
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, sh = 126 - e;  // value = m * 2^-sh units of 2^-24, sh in 14..24
    uint32_t q = m >> sh;
    const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    if (rem > half || (rem == half && (q & 1u))) q++;  // q == 0x400: the smallest normal
    return (uint16_t)(sign | q);
}
// fp32 bits -> bf16 bits, round to nearest even.
uint16_t f32_to_bf16_bits(uint32_t x) {
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

// The 768 table elements [c][u] in cfg.out_dtype: build_lut's fp32 value, narrowed once for the 16-bit types.
// `out`: 768 floats (F32) or 768 u16 (F16 / BF16). The caller validated out_dtype and std.
void norm_table(const evam_preproc& cfg, void* out) {
    if (cfg.out_dtype == EVAM_DTYPE_F32) {
        build_lut(cfg, static_cast<float*>(out));
        return;
    }
    float f[768];
    build_lut(cfg, f);
    uint16_t* o = static_cast<uint16_t*>(out);
    for (int i = 0; i < 768; i++) {
        uint32_t b;
        memcpy(&b, &f[i], 4);
        o[i] = cfg.out_dtype == EVAM_DTYPE_F16 ? f32_to_f16_bits(b) : f32_to_bf16_bits(b);
    }
}

// ---- kernel tables: runtime arguments -> template instantiation, one definition per family ----
// A family's variants (evam_plan.h: *Variants, shared with the planner's CPU check) say which combinations are
// instantiated (built) and where one sits in its table (index); here the family adds the values each template
// parameter takes (fill). expand_kernels() walks the product of the lists and calls the
// family's put<...>() once per combination; the lookup reads the table through the same index(). Both the
// occupancy query of a plan and the launch take the pointer from here, so a plan cannot be sized for one
// instantiation and launched as another, and a new template parameter is one more list and one more digit in
// one place. A combination that is not built looks up to nullptr: the call fails (launch_kernel), no neighbour
// is launched in its place.
template <int... V> struct Vals {};
using Fmts = Vals<kNV12, kI420, kBGRX, kBGR>;
using Outs = Vals<0, 1, 2>;  // out_kind()
using Bools = Vals<0, 1>;
using Pxs = Vals<1, 2, 4>;

template <class Fam, int... Done>
void expand_kernels(const void** t) { Fam::template put<Done...>(t); }
template <class Fam, int... Done, int... H, class... Rest>
void expand_kernels(const void** t, Vals<H...>, Rest... rest) { (expand_kernels<Fam, Done..., H>(t, rest...), ...); }

template <class Fam>
const void* kernel_at(int index) {
    struct Table {
        const void* fn[table_size(Fam::kDims)] = {};
        Table() { Fam::fill(fn); }
    };
    static const Table t;
    return index < 0 ? nullptr : t.fn[index];
}

struct GenericKernels : GenericVariants {
    template <int F, int O, int N>
    static void put(const void** t) { t[index(F, O, N)] = (const void*)evam_pp_kernel<F, O, N != 0>; }
    static void fill(const void** t) { expand_kernels<GenericKernels>(t, Fmts{}, Outs{}, Bools{}); }
};
const void* generic_kernel(int f, int out_dtype, bool nhwc) {
    const void* fn = kernel_at<GenericKernels>(GenericKernels::index(f, out_kind(out_dtype), nhwc));
    if (!fn) fail(EVAM_PP_ERR_UNSUPPORTED, "no generic kernel for format %d, out_dtype %d, nhwc %d", f, out_dtype, (int)nhwc);
    return fn;
}

struct RowsKernels : RowsVariants {
    template <int F, int O>
    static void put(const void** t) { t[index(F, O)] = (const void*)evam_pp_rows<F, O>; }
    static void fill(const void** t) { expand_kernels<RowsKernels>(t, Fmts{}, Bools{}); }
};
const void* rows_kernel(int f, int out_dtype) {
    const void* fn = kernel_at<RowsKernels>(RowsKernels::index(f, out_kind(out_dtype)));
    if (!fn) fail(EVAM_PP_ERR_UNSUPPORTED, "no row kernel for format %d, out_dtype %d", f, out_dtype);
    return fn;
}

struct StagedKernels : StagedVariants {
    template <int F, int O, int R, int NSEGX, int NBUF>
    static void put(const void** t) {
        if constexpr (built(R, NSEGX, NBUF)) t[index(F, O, R, NSEGX, NBUF)] = (const void*)evam_pp_staged<F, O, R, NSEGX, NBUF>;
    }
    static void fill(const void** t) { expand_kernels<StagedKernels>(t, Fmts{}, Bools{}, Vals<1, 2>{}, Pxs{}, Vals<2>{}); }
};
const void* staged_kernel(int f, int out_dtype, int R, int nsegx, int nbuf) {
    const void* fn = kernel_at<StagedKernels>(StagedKernels::index(f, out_kind(out_dtype), R, nsegx, nbuf));
    if (!fn)
        fail(EVAM_PP_ERR_UNSUPPORTED, "no staged kernel for format %d, out_dtype %d, R %d, nsegx %d, nbuf %d", f, out_dtype, R,
             nsegx, nbuf);
    return fn;
}

struct WaveKernels : WaveVariants {
    template <int F, int O, int PX, int R, int N>
    static void put(const void** t) {
        if constexpr (built(O, PX, N)) t[index(F, O, PX, R, N)] = (const void*)evam_pp_wave<F, O, PX, R != 0, N != 0>;
    }
    static void fill(const void** t) { expand_kernels<WaveKernels>(t, Fmts{}, Outs{}, Pxs{}, Bools{}, Bools{}); }
};
const void* wave_kernel(int f, int out_dtype, int px, bool reuse, bool nhwc) {
    const void* fn = kernel_at<WaveKernels>(WaveKernels::index(f, out_kind(out_dtype), px, reuse, nhwc));
    if (!fn)
        fail(EVAM_PP_ERR_UNSUPPORTED, "no wave kernel for format %d, out_dtype %d, px %d, reuse %d, nhwc %d", f, out_dtype, px,
             (int)reuse, (int)nhwc);
    return fn;
}

struct StripKernels : StripVariants {
    template <int F, int O, int PX, int PR, int N>
    static void put(const void** t) {
        if constexpr (built(O, N)) t[index(F, O, PX, PR, N)] = (const void*)evam_pp_strip<F, O, kStripD, PX, PR, N != 0>;
    }
    static void fill(const void** t) {
        expand_kernels<StripKernels>(t, Vals<kNV12, kI420, kBGRX>{}, Outs{}, Vals<1, 2>{}, Bools{}, Bools{});
    }
};
const void* strip_kernel(int f, int out_dtype, int px, int pr, bool nhwc) {
    const void* fn = kernel_at<StripKernels>(StripKernels::index(f, out_kind(out_dtype), px, pr, nhwc));
    if (!fn)
        fail(EVAM_PP_ERR_UNSUPPORTED, "no strip kernel for format %d, out_dtype %d, px %d, paired %d, nhwc %d", f, out_dtype, px,
             pr, (int)nhwc);
    return fn;
}

struct BandKernels : BandVariants {
    template <int F, int O, int PX, int DD, int N>
    static void put(const void** t) {
        if constexpr (built(O, PX, DD, N)) t[index(F, O, PX, DD, N)] = (const void*)evam_pp_band<F, O, PX, DD, N != 0>;
    }
    static void fill(const void** t) { expand_kernels<BandKernels>(t, Vals<kNV12, kI420>{}, Bools{}, Pxs{}, Bools{}, Bools{}); }
};
const void* band_kernel(int f, int out_dtype, int px, bool dd, bool nhwc) {
    const void* fn = kernel_at<BandKernels>(BandKernels::index(f, out_kind(out_dtype), px, dd, nhwc));
    if (!fn)
        fail(EVAM_PP_ERR_UNSUPPORTED, "no band kernel for format %d, out_dtype %d, px %d, dd %d, nhwc %d", f, out_dtype, px,
             (int)dd, (int)nhwc);
    return fn;
}

struct RoiKernels : RoiVariants {
    template <int F, int O, int PX, int DEV>
    static void put(const void** t) {
        if constexpr (built(PX, DEV)) t[index(F, O, PX, DEV)] = (const void*)evam_pp_roi<F, O, PX, 2, DEV != 0>;
    }
    static void fill(const void** t) { expand_kernels<RoiKernels>(t, Fmts{}, Outs{}, Pxs{}, Bools{}); }
};
const void* roi_kernel(int f, int out_dtype, int px, bool dev) {
    const void* fn = kernel_at<RoiKernels>(RoiKernels::index(f, out_kind(out_dtype), px, dev));
    if (!fn) fail(EVAM_PP_ERR_UNSUPPORTED, "no ROI kernel for format %d, out_dtype %d, px %d, dev %d", f, out_dtype, px, (int)dev);
    return fn;
}

// Every kernel above takes one parameter struct by value, so the argument array has a single entry, and the
// host-stub address from its table is what the launch, hipFuncSetAttribute and the occupancy query all receive.
// `big_lds`: the families whose LDS carve can pass 64 KB (generic, staged, ROI) raise the kernel's limit first.
// fn == nullptr: the lookup found no instantiation and has recorded which.
int launch_kernel(const void* fn, dim3 grid, dim3 block, int lds, hipStream_t stream, const void* params,
                  bool big_lds = false) {
    if (!fn) return EVAM_PP_ERR_UNSUPPORTED;
    if (big_lds && lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    void* args[] = {const_cast<void*>(params)};
    hipError_t e = hipLaunchKernel(fn, grid, block, args, (size_t)lds, stream);
    if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return EVAM_PP_OK;
}

// Workgroups of `fn` (256 threads, `lds` bytes of dynamic LDS) resident per CU: registers and LDS both
// count. Cached per (kernel, LDS size): the query runs once per shape, not per call.
int resident_per_cu(const void* fn, int lds, int threads = kThreads) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, int>, int> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({fn, lds, threads});
    if (it != cache.end()) return it->second;
    int n = 0;
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, (size_t)lds) != hipSuccess || n <= 0)
        n = std::max(1, std::min(8, (160 * 1024) / std::max(lds, 1)));
    cache[{fn, lds, threads}] = n;
    return n;
}

// HIP backend of the planner (evam_plan.h): the families' lookups above and the occupancy query.
struct HipKernels {
    static const void* rows(int f, int out_dtype) { return rows_kernel(f, out_dtype); }
    static const void* staged(int f, int out_dtype, int R, int nsegx, int nbuf) { return staged_kernel(f, out_dtype, R, nsegx, nbuf); }
    static const void* wave(int f, int out_dtype, int px, bool reuse, bool nhwc) { return wave_kernel(f, out_dtype, px, reuse, nhwc); }
    static const void* strip(int f, int out_dtype, int px, int pr, bool nhwc) { return strip_kernel(f, out_dtype, px, pr, nhwc); }
    static const void* band(int f, int out_dtype, int px, bool dd, bool nhwc) { return band_kernel(f, out_dtype, px, dd, nhwc); }
    static const void* roi(int f, int out_dtype, int px, bool dev) { return roi_kernel(f, out_dtype, px, dev); }
    static int resident(const void* fn, int lds) { return resident_per_cu(fn, lds); }
};

// HIP backend of the descriptor rings (evam_rings.h): events, streams, pinned and device memory. Every
// failure is reported through fail() with the HIP error string.
struct HipRings {
    using Event = hipEvent_t;
    using Stream = hipStream_t;
    static int err(hipError_t e, const char* what) {
        return e == hipSuccess ? 0 : fail(EVAM_PP_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    }
    int event_create(Event* e) { return err(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate"); }
    int event_destroy(Event e) { return err(hipEventDestroy(e), "hipEventDestroy"); }
    int event_record(Event e, Stream s) { return err(hipEventRecord(e, s), "hipEventRecord"); }
    int event_sync(Event e) { return err(hipEventSynchronize(e), "hipEventSynchronize"); }
    int stream_create(Stream* s) { return err(hipStreamCreateWithFlags(s, hipStreamNonBlocking), "hipStreamCreate"); }
    int stream_destroy(Stream s) { return err(hipStreamDestroy(s), "hipStreamDestroy"); }
    int stream_wait(Stream s, Event e) { return err(hipStreamWaitEvent(s, e, 0), "hipStreamWaitEvent"); }
    int stream_sync(Stream s) { return err(hipStreamSynchronize(s), "hipStreamSynchronize"); }
    // ROI record slots: fine-grained device memory that the host writes through the platform's BAR mapping of it
    // (one 64-byte scalar load per workgroup from device memory instead of a PCIe read from host memory: ~4.5 us
    // less per 1,600-workgroup launch, tools/microbench/rec_hostwrite.hip), where the allocation is mapped
    // read-write into this process; else pinned, coherent host memory (EVAM_PP_REC_DEVICE=0 forces that).
    bool rec_device = true;
    static bool host_mapped_rw(const void* p, size_t n) {
        FILE* f = fopen("/proc/self/maps", "r");
        if (!f) return false;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p), e = a + n;
        char line[512];
        bool ok = false;
        while (!ok && fgets(line, sizeof(line), f)) {
            unsigned long lo = 0, hi = 0;
            char perm[8] = {};
            if (sscanf(line, "%lx-%lx %7s", &lo, &hi, perm) == 3 && lo <= a && e <= hi) ok = perm[0] == 'r' && perm[1] == 'w';
        }
        fclose(f);
        return ok;
    }
    int pinned_alloc(uint8_t** h, const uint8_t** d, size_t n, bool* wc) {
        *wc = false;
        if (rec_device) {
            void* p = nullptr;
            if (hipExtMallocWithFlags(&p, n, hipDeviceMallocFinegrained) == hipSuccess) {
                if (host_mapped_rw(p, n)) {
                    *h = static_cast<uint8_t*>(p);
                    *d = static_cast<const uint8_t*>(p);
                    *wc = true;
                    return 0;
                }
                (void)hipFree(p);
            } else {
                (void)hipGetLastError();
            }
        }
        if (hipHostMalloc((void**)h, n, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            *h = nullptr;
            return fail(EVAM_PP_ERR_OOM, "evam_pp_run: hipHostMalloc(%zu) failed", n);
        }
        void* dp = nullptr;
        if (int rc = err(hipHostGetDevicePointer(&dp, *h, 0), "hipHostGetDevicePointer")) return rc;
        *d = reinterpret_cast<const uint8_t*>(dp);
        return 0;
    }
    int pinned_free(uint8_t* h, bool wc) { return wc ? err(hipFree(h), "hipFree") : err(hipHostFree(h), "hipHostFree"); }
    int host_alloc(uint8_t** h, size_t n) {
        if (hipHostMalloc((void**)h, n, hipHostMallocDefault) != hipSuccess) {
            *h = nullptr;
            return fail(EVAM_PP_ERR_OOM, "evam_pp_run: hipHostMalloc(%zu) failed", n);
        }
        return 0;
    }
    int host_free(uint8_t* h) { return err(hipHostFree(h), "hipHostFree"); }
    int dev_alloc(uint8_t** d, size_t n) {
        if (hipMalloc((void**)d, n) != hipSuccess) {
            *d = nullptr;
            return fail(EVAM_PP_ERR_OOM, "evam_pp_run: hipMalloc(%zu) failed", n);
        }
        return 0;
    }
    int dev_free(uint8_t* d) { return err(hipFree(d), "hipFree"); }
    int copy_h2d(uint8_t* dst, const uint8_t* src, size_t n, Stream s) {
        return err(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, s), "hipMemcpyAsync");
    }
};
using DescRing = DescRingT<HipRings>;
using PinRing = PinRingT<HipRings>;

#include "evam_jpeg_kernels.h"
#include "evam_jpeg_dec_kernels.h"
#include "evam_track_kernels.h"
#include "evam_detout_kernels.h"

// evam_pp_decode_jpeg: device scratch (grown on demand, reused) and the pinned staging of the file bytes.
enum { kJdUp = 0, kJdStream, kJdFirst, kJdSlots, kJdCoef, kJdPlanes, kJdCount };
struct JdecScratch {
    void* buf[kJdCount] = {};
    size_t cap[kJdCount] = {};
    uint8_t* pin = nullptr;        // pinned staging: tables, output descriptors, file bytes of one call
    size_t pin_cap = 0;
    hipEvent_t pin_ev = nullptr;   // recorded behind the copy out of pin
    bool pin_busy = false;
    std::vector<JdecFile> parsed;  // per-call scratch
};

}  // namespace

#ifdef EVAM_PP_HOST_PROF
// Diagnostic build: cumulative host time from entry to each mark of evam_pp_run, printed at destroy.
#include <chrono>
static double g_hp[12];
static long g_hp_n;
#define HP_START const auto hp_t0 = std::chrono::steady_clock::now(); double hp_t[12] = {}
#define HP(i) (hp_t[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - hp_t0).count())
#else
#define HP_START (void)0
#define HP(i) (void)0
#endif

namespace {

struct RecFrame { __m128i l[3]; };  // a record's bytes 0-47 for one source (bytes 40-47 zero)
RecFrame rec_frame(const evam_image& s) {
    RoiRec r;
    memset(&r, 0, sizeof(r));
    for (int p = 0; p < 3; p++) { r.plane[p] = s.planes[p]; r.pitch[p] = s.pitch[p]; }
    r.width = (uint16_t)s.width; r.height = (uint16_t)s.height;
    RecFrame f;
    memcpy(&f, &r, sizeof(f));
    return f;
}

}  // namespace

struct evam_pp {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    int opt_stats = 0, opt_timing = 0;
    evam_pp_stats stats{};
    std::vector<uint8_t> h_block;  // this call's descriptor block, built on the host
    DescRing ring;
    PinRing pin;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_switch = nullptr;
    bool timed = false;
    TabCache tab_cache;
    evam_preproc lut_key{};        // cfg the cached LUT was built from (norm fields + dtype)
    bool lut_valid = false;
    float lut[768];
    Knobs knobs;                   // EVAM_PP_* tuning knobs, read once at evam_pp_create
    std::vector<int> sc_fmt;       // per-call scratch, kept to avoid reallocation
    std::vector<int> sc_bucket;
    std::vector<int> sc_sfmt;      // per-call source format ids
    std::vector<int> sc_order;
    std::vector<int> sc_members;   // item indices grouped by source format
    std::vector<Geom> sc_geo;
    std::vector<int> sc_units;     // ROI work units: (item, row0, row1, cost)
    std::vector<int> sc_start;     // ROI unit counting sort: bucket starts
    std::vector<int> sc_slot;      // ROI units in launch order
    std::vector<uint8_t> sc_seen;  // evam_pp_run_slots: output slots taken
    std::vector<uint32_t> sc_plan; // roi_launch_order scratch
    std::vector<RecFrame> sc_frames;  // per source: the frame half of its ROI records
    int memo_key[4] = {-1, -1, -1, -1};  // (format, staging buffer, row cap, DH) of memo_rg
    std::vector<uint32_t> memo_rg;       // per crop width: rows per group | groups of the whole height << 16
    TParams sc_tparams;            // strip-kernel arguments (3.5 KB: kept off the stack)
    std::vector<XTab> sc_xt;       // interleaved output: the tables a group's kernel choice is planned on
    std::vector<YTab> sc_yt;
    int nhwc_key[4][16] = {};      // per format: what the last interleaved uniform group's choice depended on
    int nhwc_ok[4] = {-1, -1, -1, -1};  // ... and the choice: 1 strip / wave kernel, 0 generic kernel (-1: none yet)
    JpegScratch jpeg;              // evam_pp_encode_jpeg: device scratch and the tables' key
    JdecScratch jdec;              // evam_pp_decode_jpeg: device scratch and pinned staging
    // Device-resident ROI lists. Both buffers are written and read by kernels only, all on the handle's stream, so
    // stream order makes their reuse safe with any number of calls in flight (evam_pp_set_stream orders a new stream
    // behind the old one); they grow by hipFree + hipMalloc, and hipFree waits for the kernels that still use them.
    void* dev_recs = nullptr;      // evam_pp_run_device_rois: RoiRec x cap x tiles
    size_t dev_recs_cap = 0;
    void* dev_cnt = nullptr;       // evam_pp_ssd_rois: per-item counts, then per-item list offsets
    size_t dev_cnt_cap = 0;
    std::vector<uint8_t> h_aux;    // their host-built block (per-source table / per-item sizes, transforms, labels)
    DescRing ring_ssd;             // evam_pp_ssd_rois' block: a ring of its own, so that a detect -> classify chain that
                                   // alternates it with evam_pp_run_device_rois' block re-uploads neither when unchanged
    DescRing ring_trk;             // evam_pp_track_device_rois' block (stream runs, item table, classify label set)
    void* dev_detout = nullptr;    // evam_pp_detection_output: per-class kept counts and keys (kernels only, as above)
    size_t dev_detout_cap = 0;
};

namespace {

// A failed evam_pp_run after its pinned slot was taken: drain the stream (PinRingT::abandon), so a run
// whose fence the failed call should have recorded cannot leave slots that kernels still read.
struct PinGuard {
    evam_pp* h;
    bool armed = false;
    ~PinGuard() {
        if (armed) {
            HipRings b;
            (void)h->pin.abandon(b, h->stream);
        }
    }
};

}  // namespace

extern "C" {

int evam_pp_abi_version(void) { return EVAM_PP_ABI_VERSION; }

#ifdef EVAM_PP_TRACE
// Diagnostic builds: copy the first n_wg workgroups' trace records (kTraceSlots x u64 each) of the last
// traced launch.
// host == NULL: clear the trace buffer (before the launch to trace).
int evam_pp_debug_trace(unsigned long long* host, int n_wg) {
    if (!host) {
        void* a = nullptr;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipGetSymbolAddress(&a, HIP_SYMBOL(g_evam_trace)));
        HIP_TRY(hipMemset(a, 0, sizeof(g_evam_trace)));
        return EVAM_PP_OK;
    }
    if (n_wg <= 0 || n_wg > kTraceWGs) return EVAM_PP_ERR_INVALID_ARG;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_evam_trace),
                                sizeof(unsigned long long) * kTraceSlots * (size_t)n_wg));
    return EVAM_PP_OK;
}
#endif

const char* evam_pp_last_error(void) { return g_last_error.c_str(); }

int evam_pp_create(int hip_device, void* hip_stream, evam_pp** out) {
    if (!out) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_create: out is NULL");
    *out = nullptr;
    if (kAblate != 0) {  // a stage-removal diagnostic build computes invalid tensors: never by accident
        const char* ok = getenv("EVAM_PP_DIAGNOSTIC_BUILD_OK");
        if (!ok || strcmp(ok, "1") != 0)
            return fail(EVAM_PP_ERR_UNSUPPORTED, "evam_pp_create: diagnostic build (EVAM_PP_ABLATE=%d) refused; "
                        "set EVAM_PP_DIAGNOSTIC_BUILD_OK=1 for profiling runs", kAblate);
        fprintf(stderr, "[evam_pp] DIAGNOSTIC BUILD (EVAM_PP_ABLATE=%d): outputs are invalid\n", kAblate);
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(EVAM_PP_ERR_NO_DEVICE, "evam_pp_create: no HIP device");
    if (hip_device < 0 || hip_device >= n)
        return fail(EVAM_PP_ERR_NO_DEVICE, "evam_pp_create: device %d out of range [0,%d)", hip_device, n);
    HIP_TRY(hipSetDevice(hip_device));
    evam_pp* h = new (std::nothrow) evam_pp();
    if (!h) return fail(EVAM_PP_ERR_OOM, "evam_pp_create: out of host memory");
    h->device = hip_device;
    h->knobs.read();
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess || h->n_cu <= 0)
        h->n_cu = 256;
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
        delete h;
        return fail(EVAM_PP_ERR_HIP, "evam_pp_create: hipEventCreate failed");
    }
    *out = h;
    return EVAM_PP_OK;
}

void evam_pp_destroy(evam_pp* h) {
    if (!h) return;
#ifdef EVAM_PP_HOST_PROF
    if (g_hp_n) {
        fprintf(stderr, "[host prof] %ld steady calls, mean us from entry at marks 1..10:", g_hp_n);
        for (int i = 1; i <= 10; i++) fprintf(stderr, " %.2f", g_hp[i] / g_hp_n);
        fprintf(stderr, "\n");
    }
#endif
    (void)hipSetDevice(h->device);
    if (h->ring.have_copy || h->ring_ssd.have_copy || h->ring_trk.have_copy || h->pin.cur >= 0) {
        (void)hipStreamSynchronize(h->stream);
        if (h->ring.have_copy) (void)hipStreamSynchronize(h->ring.copy);
        if (h->ring_ssd.have_copy) (void)hipStreamSynchronize(h->ring_ssd.copy);
        if (h->ring_trk.have_copy) (void)hipStreamSynchronize(h->ring_trk.copy);
    }
    HipRings b;
    h->ring.release(b);
    h->ring_ssd.release(b);
    h->ring_trk.release(b);
    h->pin.release(b);
    for (void* p : h->jpeg.buf)
        if (p) (void)hipFree(p);  // waits for kernels that still use it
    for (void* p : h->jdec.buf)
        if (p) (void)hipFree(p);
    if (h->jdec.pin_busy) (void)hipEventSynchronize(h->jdec.pin_ev);
    if (h->jdec.pin) (void)hipHostFree(h->jdec.pin);
    if (h->jdec.pin_ev) (void)hipEventDestroy(h->jdec.pin_ev);
    if (h->dev_recs) (void)hipFree(h->dev_recs);
    if (h->dev_cnt) (void)hipFree(h->dev_cnt);
    if (h->dev_detout) (void)hipFree(h->dev_detout);
    if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

int evam_pp_set_stream(evam_pp* h, void* hip_stream) {
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_set_stream: NULL handle");
    hipStream_t ns = reinterpret_cast<hipStream_t>(hip_stream);
    if (ns != h->stream && (h->ring.cur >= 0 || h->pin.cur >= 0 || h->ring_ssd.cur >= 0 || h->ring_trk.cur >= 0)) {
        // Order the new stream behind everything already launched on the old one, so the descriptor
        // slots' fences (recorded on the current stream) keep covering earlier kernels.
        HIP_TRY(hipSetDevice(h->device));
        if (!h->ev_switch) HIP_TRY(hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->ev_switch, h->stream));
        HIP_TRY(hipStreamWaitEvent(ns, h->ev_switch, 0));
    }
    h->stream = ns;
    return EVAM_PP_OK;
}

int evam_pp_set_option(evam_pp* h, int option, int value) {
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_set_option: NULL handle");
    if (option == EVAM_OPT_STATS) h->opt_stats = value != 0;
    else if (option == EVAM_OPT_TIMING) h->opt_timing = value != 0;
    else return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_set_option: unknown option %d", option);
    return EVAM_PP_OK;
}

int evam_pp_sync(evam_pp* h) {
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_sync: NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EVAM_PP_OK;
}

int evam_pp_get_stats(evam_pp* h, evam_pp_stats* out) {
    if (!h || !out) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_get_stats: NULL argument");
    if (h->timed) {
        HIP_TRY(hipEventSynchronize(h->ev1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        h->stats.last_kernel_ms = ms;
    }
    *out = h->stats;
    return EVAM_PP_OK;
}

int evam_pp_linear_table(int src_size, int dst_size, int is_x, int32_t* ofs, int16_t* c0, int16_t* c1) {
    if (src_size <= 0 || dst_size <= 0 || !ofs || !c0 || !c1)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_linear_table: bad arguments");
    const double scale = 1. / ((double)dst_size / src_size);
    for (int d = 0; d < dst_size; d++) {
        int s, a, b;
        linear_coef(d, scale, src_size, is_x != 0, s, a, b);
        ofs[d] = s;
        c0[d] = (int16_t)a;
        c1[d] = (int16_t)b;
    }
    return EVAM_PP_OK;
}

int evam_pp_norm_table(const evam_preproc* cfg, void* out) {
    if (!cfg || !out) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_norm_table: NULL argument");
    if (cfg->out_dtype == EVAM_DTYPE_U8)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_norm_table: u8 output has no normalisation table");
    if (cfg->out_dtype != EVAM_DTYPE_F32 && cfg->out_dtype != EVAM_DTYPE_F16 && cfg->out_dtype != EVAM_DTYPE_BF16)
        return fail(EVAM_PP_ERR_UNSUPPORTED, "evam_pp_norm_table: unknown out_dtype %d", cfg->out_dtype);
    if (cfg->norm_flags & EVAM_NORM_MEAN_STD)
        for (int c = 0; c < 3; c++)
            if (cfg->std[c] == 0.f) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_norm_table: std[%d] == 0", c);
    norm_table(*cfg, out);
    return EVAM_PP_OK;
}

}  // extern "C"

namespace {

// The sources of a call: format, size, plane pointers and pitches.
int validate_sources(const evam_image* srcs, int n_srcs) {
    for (int i = 0; i < n_srcs; i++) {
        const evam_image& s = srcs[i];
        const int f = fmt_id(s.fourcc);
        if (f < 0) return fail(EVAM_PP_ERR_UNSUPPORTED, "evam_pp_run: srcs[%d] fourcc 0x%08x unsupported", i, s.fourcc);
        if (s.width <= 0 || s.height <= 0 || s.width > 32768 || s.height > 32768)
            return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: srcs[%d] bad size %dx%d", i, s.width, s.height);
        if ((f == kNV12 || f == kI420) && ((s.width | s.height) & 1))
            return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: srcs[%d] 4:2:0 frame must have even size (%dx%d)", i, s.width, s.height);
        for (int p = 0; p < fmt_nplanes(f); p++) {
            const int row_bytes = p == 0 ? s.width * fmt_bpp(f) : (f == kNV12 ? s.width : s.width / 2);
            const int rows = p == 0 ? s.height : s.height / 2;
            if (!s.planes[p]) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: srcs[%d].planes[%d] is NULL", i, p);
            if (((uintptr_t)s.planes[p] & 15) || (s.pitch[p] & 15))
                return fail(EVAM_PP_ERR_ALIGNMENT, "evam_pp_run: srcs[%d] plane %d pointer/pitch (%d) not 16-byte aligned", i, p, s.pitch[p]);
            if (s.pitch[p] < row_bytes)
                return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: srcs[%d] plane %d pitch %d < row bytes %d", i, p, s.pitch[p], row_bytes);
            // the kernels address a plane through buffer resources with 32-bit byte offsets
            if ((int64_t)s.pitch[p] * rows > INT32_MAX)
                return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: srcs[%d] plane %d (%d x %d B) exceeds 2 GiB", i, p, rows, s.pitch[p]);
        }
    }
    return 0;
}

// The first kLutBytes of a call's descriptor block: the normalisation table of cfg (zeros for u8 output), from the
// handle's cached copy.
void block_lut(evam_pp* h, const evam_preproc* cfg, uint8_t* blk) {
    if (cfg->out_dtype == EVAM_DTYPE_U8) {
        memset(blk, 0, kLutBytes);
        return;
    }
    // The LUT depends only on the dtype and the normalisation fields: rebuilt when they change.
    evam_preproc key{};
    key.out_dtype = cfg->out_dtype;
    key.norm_flags = cfg->norm_flags;
    memcpy(key.range, cfg->range, sizeof(key.range));
    memcpy(key.mean, cfg->mean, sizeof(key.mean));
    memcpy(key.std, cfg->std, sizeof(key.std));
    if (!h->lut_valid || memcmp(&key, &h->lut_key, sizeof(key)) != 0) {
        if (cfg->out_dtype == EVAM_DTYPE_F16 || cfg->out_dtype == EVAM_DTYPE_BF16) {
            // norm_table's 16-bit elements, one per 4-byte entry (low half; the kernels read only that)
            uint16_t t16[768];
            norm_table(*cfg, t16);
            for (int i = 0; i < 768; i++) {
                const uint32_t b = t16[i];
                memcpy(&h->lut[i], &b, 4);
            }
        } else {
            norm_table(*cfg, h->lut);
        }
        h->lut_key = key;
        h->lut_valid = true;
    }
    memcpy(blk, h->lut, kLutBytes);
}

// The checks of dst and cfg that evam_pp_run(_slots) and evam_pp_run_device_rois share, in the order both report them.
int check_output(const char* who, const evam_preproc* cfg, const evam_tensor* dst) {
    if (!dst->data) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: dst->data is NULL", who);
    if (dst->c != 3) return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: dst must have 3 channels (got %d)", who, dst->c);
    if (dst->n <= 0 || dst->h <= 0 || dst->w <= 0)
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: bad dst shape %dx%dx%dx%d", who, dst->n, dst->c, dst->h, dst->w);
    if (cfg->out_dtype != EVAM_DTYPE_U8 && cfg->out_dtype != EVAM_DTYPE_F32 && cfg->out_dtype != EVAM_DTYPE_F16 &&
        cfg->out_dtype != EVAM_DTYPE_BF16)
        return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: unknown out_dtype %d", who, cfg->out_dtype);
    if (cfg->resize_mode < 0 || cfg->resize_mode > 2)
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: unknown resize_mode %d", who, cfg->resize_mode);
    if ((cfg->norm_flags & EVAM_NORM_MEAN_STD) && cfg->out_dtype != EVAM_DTYPE_U8)
        for (int c = 0; c < 3; c++)
            if (cfg->std[c] == 0.f) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: std[%d] == 0", who, c);
    const int64_t plane = (int64_t)dst->w * dst->h;
    if (plane * 3 * (int64_t)dst->n > ((int64_t)1 << 40)) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: dst too large", who);
    // The kernels address one output plane with 32-bit byte offsets.
    if (plane * out_esz(out_kind(cfg->out_dtype)) > INT32_MAX)
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: dst plane %dx%d exceeds 2 GiB", who, dst->w, dst->h);
    return 0;
}

uint32_t pack_fill(const evam_preproc* cfg) {
    return (uint32_t)cfg->fill[0] | ((uint32_t)cfg->fill[1] << 8) | ((uint32_t)cfg->fill[2] << 16);
}

// The launch fields of the ROI kernel's arguments (the planner has set the rest), for records at `recs`.
void roi_launch_fields(QParams& q, const RoiRec* recs, const float* lut, const evam_preproc* cfg, const evam_tensor* dst,
                       int slot_offset, int slot_stride, int prio) {
    q.recs = recs;
    q.lut = lut;
    q.dst = dst->data;
    q.mode = cfg->resize_mode;
    q.placement = cfg->placement;
    q.slot_offset = slot_offset;
    q.slot_stride = slot_stride;
    q.color_rgb = cfg->color_order == EVAM_COLOR_RGB;
    q.fill = pack_fill(cfg);
    q.prio = prio;
}

// evam_pp_run and evam_pp_run_slots. slots == NULL: item i -> slot dst->slot_offset + i * dst->slot_stride; else item i
// -> slot slots[i]. The kernels read one output index per item (ItemArg / ItemDesc .index, RoiRec .item) and compute
// slot = slot_offset + index * slot_stride, so an explicit table travels as index = slots[i], offset 0, stride 1.
int run_impl(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi* items, int n_items, const evam_preproc* cfg,
             const evam_tensor* dst, const int32_t* slots, evam_transform* out_xform) {
    HP_START;
    if (!h || !srcs || !cfg || !dst) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: NULL argument");
    if (n_srcs <= 0) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: n_srcs must be > 0");
    if (!items) n_items = n_srcs;
    if (n_items <= 0) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: n_items must be > 0");
    if (int rc = check_output("evam_pp_run", cfg, dst)) return rc;
    const bool half = cfg->out_dtype == EVAM_DTYPE_F16 || cfg->out_dtype == EVAM_DTYPE_BF16;  // 2-byte elements
    const int DW = dst->w, DH = dst->h;
    const int64_t plane = (int64_t)DW * DH;
    const int esz = out_esz(out_kind(cfg->out_dtype));
    if (dst->layout != EVAM_LAYOUT_NCHW && dst->layout != EVAM_LAYOUT_NHWC)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: unknown dst layout %d", dst->layout);
    const bool nhwc = dst->layout == EVAM_LAYOUT_NHWC;
    // One interleaved slot is addressed with 32-bit byte offsets too: its last element is at 3 * plane - 1.
    if (nhwc && plane * 3 * esz > INT32_MAX)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: interleaved dst slot %dx%dx3 exceeds 2 GiB", DH, DW);
    if (nhwc && ((uintptr_t)dst->data & (uintptr_t)(esz - 1)))
        return fail(EVAM_PP_ERR_ALIGNMENT, "evam_pp_run: dst->data is not aligned to its %d-byte elements", esz);
    const Knobs& kn = h->knobs;

    if (int rc = validate_sources(srcs, n_srcs)) return rc;

    HP(1);
    // ---- pass 1 (integer only): item -> source, format, clipped crop; validation ----
    std::vector<int>& fmt = h->sc_fmt;
    std::vector<Geom>& geo = h->sc_geo;
    fmt.resize(n_items);
    geo.resize(n_items);
    int count[4] = {0, 0, 0, 0};
    int rep[4] = {-1, -1, -1, -1};
    int max_cw[4] = {0, 0, 0, 0}, max_ch[4] = {0, 0, 0, 0};
    uint32_t x0_mask[4] = {0, 0, 0, 0};  // crop origins x0 mod 32 present (wave-kernel staging bound)
    bool uniform[4] = {true, true, true, true};
    if (slots) {
        // an explicit slot per item: each inside the batch, no two items into one slot
        std::vector<uint8_t>& seen = h->sc_seen;
        seen.assign((size_t)dst->n, 0);
        for (int i = 0; i < n_items; i++) {
            const int32_t sl = slots[i];
            if (sl < 0 || sl >= dst->n)
                return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run_slots: slots[%d] = %d outside tensor batch %d", i, sl,
                            dst->n);
            if (seen[sl]++)
                return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run_slots: slot %d given to two items (slots[%d])", sl, i);
        }
    } else {
        // output slots are linear in the item index: the first and the last bound them all
        for (int i : {0, n_items - 1}) {
            const int64_t slot = (int64_t)dst->slot_offset + (int64_t)i * dst->slot_stride;
            if (slot < 0 || slot >= dst->n)
                return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: item %d -> slot %lld outside tensor batch %d", i,
                            (long long)slot, dst->n);
        }
    }
    const int slot_offset = slots ? 0 : dst->slot_offset, slot_stride = slots ? 1 : dst->slot_stride;
    std::vector<int>& sfmt = h->sc_sfmt;  // per source: format id (looked up once, not per ROI)
    sfmt.resize(n_srcs);
    bool one_fmt = true, one_size = true;
    for (int i = 0; i < n_srcs; i++) {
        sfmt[i] = fmt_id(srcs[i].fourcc);
        one_fmt &= sfmt[i] == sfmt[0];
        one_size &= srcs[i].width == srcs[0].width && srcs[i].height == srcs[0].height;
    }
    static const bool has_avx2 = __builtin_cpu_supports("avx2");
    if (one_fmt && one_size && items && n_items >= 8 && has_avx2 && kn.host_simd &&
        clip_rois_avx2(items, n_items, n_srcs, srcs[0].width, srcs[0].height, sfmt[0] == kNV12 || sfmt[0] == kI420,
                       geo.data(), max_cw[sfmt[0]], max_ch[sfmt[0]], x0_mask[sfmt[0]], uniform[sfmt[0]])) {
        const int f = sfmt[0];
        std::fill(fmt.begin(), fmt.end(), f);
        count[f] = n_items; rep[f] = 0;
    } else if (one_fmt && items && n_items > 0 && n_srcs > 0) {
        // every source in one format (the common case: one decoder): the group's counters live in registers
        // instead of arrays indexed by the item's format (a store-to-load chain per ROI: C3 pass 1 ~7 -> ~4 us)
        const int f = sfmt[0];
        int mcw = 0, mch = 0, rcw = 0, rch = 0;
        uint32_t xm = 0;
        bool uni = true;
        for (int i = 0; i < n_items; i++) {
            const evam_roi& r = items[i];
            if ((unsigned)r.src_index >= (unsigned)n_srcs)
                return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: items[%d].src_index %d out of range", i, r.src_index);
            const evam_image& s = srcs[r.src_index];
            fmt[i] = f;
            Geom& g = geo[i];
            if (roi_clip(f, s.width, s.height, true, r.x, r.y, r.w, r.h, g))
                return fail(EVAM_PP_ERR_EMPTY_ROI, "evam_pp_run: items[%d] ROI (%d,%d,%d,%d) is empty after clipping to %dx%d",
                            i, r.x, r.y, r.w, r.h, s.width, s.height);
            mcw = std::max(mcw, g.cw);
            mch = std::max(mch, g.ch);
            xm |= 1u << (g.x0 & 31);
            if (i == 0) { rcw = g.cw; rch = g.ch; }
            uni &= g.cw == rcw && g.ch == rch;  // geometry = f(cw, ch)
        }
        count[f] = n_items; max_cw[f] = mcw; max_ch[f] = mch; x0_mask[f] = xm; rep[f] = 0; uniform[f] = uni;
    } else
    for (int i = 0; i < n_items; i++) {
        const evam_roi* r = items ? &items[i] : nullptr;
        const int si = items ? r->src_index : i;
        if ((unsigned)si >= (unsigned)n_srcs)
            return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: items[%d].src_index %d out of range", i, si);
        const evam_image& s = srcs[si];
        const int f = sfmt[si];
        fmt[i] = f;
        Geom& g = geo[i];
        if (roi_clip(f, s.width, s.height, r != nullptr, r ? r->x : 0, r ? r->y : 0, r ? r->w : 0, r ? r->h : 0, g))
            return fail(EVAM_PP_ERR_EMPTY_ROI, "evam_pp_run: items[%d] ROI (%d,%d,%d,%d) is empty after clipping to %dx%d",
                        i, r ? r->x : 0, r ? r->y : 0, r ? r->w : 0, r ? r->h : 0, s.width, s.height);
        count[f]++;
        max_cw[f] = std::max(max_cw[f], g.cw);
        max_ch[f] = std::max(max_ch[f], g.ch);
        x0_mask[f] |= 1u << (g.x0 & 31);
        if (rep[f] < 0) rep[f] = i;
        else if (g.cw != geo[rep[f]].cw || g.ch != geo[rep[f]].ch) uniform[f] = false;  // geometry = f(cw, ch)
    }
    HP(2);
    // item indices grouped by format, in call order within a format
    std::vector<int>& members = h->sc_members;
    members.resize(n_items);
    int mfirst[5] = {0, 0, 0, 0, 0};
    for (int f = 0; f < 4; f++) mfirst[f + 1] = mfirst[f] + count[f];
    if (n_items == count[fmt[0]]) {  // one format: call order
        for (int i = 0; i < n_items; i++) members[i] = i;
    } else {
        int fill_at[4] = {mfirst[0], mfirst[1], mfirst[2], mfirst[3]};
        for (int i = 0; i < n_items; i++) members[fill_at[fmt[i]]++] = i;
    }

    // ---- per format group: kernel choice ----
    //   uniform geometry        -> staged / wave / row kernels: host-built tables, items in kernel arguments
    //   per-item geometry       -> ROI kernel: raw ROI rect + source (RoiRec), geometry resolved on the device
    //   ROI plan impossible     -> generic kernel, per-item ItemDesc in the descriptor block
    enum { kPathNone, kPathUniform, kPathRoi, kPathGeneric };
    // I420 paired chroma addresses both chroma planes from one buffer resource based at the lower one: for every
    // item, the upper plane's offset from the lower plus its extent must fit the resource's 0x7FFFFFFF bytes (else
    // no pairing for the group)
    auto strip_pair_ok = [&](int f) {
        bool ok = true;
        if (f == kI420 && kn.strip_pair)
            for (int m = 0; m < n_items && ok; m++) {
                if (fmt[m] != f) continue;
                const evam_image& sr = srcs[items ? items[m].src_index : m];
                const int64_t d = (int64_t)((intptr_t)sr.planes[2] - (intptr_t)sr.planes[1]);
                const int64_t ext = (int64_t)sr.pitch[d >= 0 ? 2 : 1] * (sr.height / 2);
                ok = (d >= 0 ? d : -d) + ext <= (int64_t)0x7FFFFFFF;
            }
        return ok;
    };
    // Interleaved output takes the strip kernel in fp32 (12-byte stores, dword-aligned as the elements are) and the
    // band (u8) and wave kernels' four-pixel stores where they are aligned to their width: DW % 4 == 0 makes every row and slot
    // size a multiple of it, so the tensor's base decides (4 bytes for u8, 16 for fp32).
    const bool nhwc_wave_ok = DW % 4 == 0 && ((uintptr_t)dst->data & (uintptr_t)(esz == 4 ? 15 : 3)) == 0;
    // Uniform group f's plan (plan_uniform: the one kernel-choice cascade) on the host tables xt / yt.
    UniformParams up;  // not cleared here: a plan_* function clears the struct it fills
    auto plan_group = [&](int f, const XTab* xt, const YTab* yt, bool pair_ok) {
        const UniformGroup u{f, geo[rep[f]], DW, DH, count[f], cfg->out_dtype, h->n_cu, xt, yt, x0_mask[f], kn, pair_ok, nhwc,
                             nhwc_wave_ok};
        return plan_uniform(HipKernels{}, u, h->sc_tparams, up);
    };
    // Does a uniform-geometry kernel serve interleaved uniform group f? Decided here, ahead of the descriptor block, so
    // that only a group the generic kernel serves puts its items' descriptors (which change with every set of
    // frames) into it; the launch below plans again with the same arguments. Memoised on those arguments.
    // The same question for a planar 16-bit group: the strip kernel, or the wave kernel where rows share source rows;
    // where fp32 would fall to the staged or row kernels (not instantiated for 2-byte elements) the generic kernel
    // serves the group, which needs its descriptors in the block too.
    auto planned_uniform_ok = [&](int f) {
        const int i = rep[f];
        const evam_roi* r = items ? &items[i] : nullptr;
        const evam_image& s = srcs[items ? r->src_index : i];
        Geom& g = geo[i];
        roi_geometry(f, s.width, s.height, r != nullptr, r ? r->x : 0, r ? r->y : 0, r ? r->w : 0, r ? r->h : 0,
                     cfg->resize_mode, cfg->placement, DW, DH, g);
        const bool pair_ok = strip_pair_ok(f);
        const int key[16] = {1, g.cw, g.ch, g.rw, g.rh, g.ox, g.oy, DW, DH, cfg->out_dtype, count[f], (int)x0_mask[f],
                             (int)nhwc_wave_ok, (int)pair_ok, g.x0 & 31, (int)nhwc};
        if (h->nhwc_ok[f] >= 0 && memcmp(key, h->nhwc_key[f], sizeof(key)) == 0) return h->nhwc_ok[f] == 1;
        h->sc_xt.resize((size_t)DW);
        h->sc_yt.resize((size_t)DH);
        build_tables(g, DW, DH, h->tab_cache, h->sc_xt.data(), h->sc_yt.data());
        const bool ok = plan_group(f, h->sc_xt.data(), h->sc_yt.data(), pair_ok).family != 0;
        memcpy(h->nhwc_key[f], key, sizeof(key));
        h->nhwc_ok[f] = ok ? 1 : 0;
        return ok;
    };
    int path[4];
    QParams qp[4];
    int qlds[4] = {0, 0, 0, 0}, qbase[4] = {1, 1, 1, 1}, qrec[4] = {0, 0, 0, 0};
    int64_t qslots[4] = {0, 0, 0, 0};
    const void* qfn[4] = {nullptr, nullptr, nullptr, nullptr};
    bool any_generic = false, any_roi = false;
    for (int f = 0; f < 4; f++) {
        path[f] = kPathNone;
        if (!count[f]) continue;
        // Interleaved output: uniform geometry tries the strip kernel (fp32 downscales) and the wave kernel (the rest,
        // where its wide stores are aligned), see the launches below; the generic kernel serves everything else.
        // 16-bit output: interleaved is the generic kernel's; planar uniform groups take the strip or wave kernel.
        if (nhwc) path[f] = !half && uniform[f] && kn.rows && planned_uniform_ok(f) ? kPathUniform : kPathGeneric;
        else if (half && uniform[f] && kn.rows) path[f] = planned_uniform_ok(f) ? kPathUniform : kPathGeneric;
        else if (uniform[f] && kn.rows) path[f] = kPathUniform;
        else if (kn.roi && plan_roi(HipKernels{}, f, DW, DH,cfg->out_dtype, kn.roi_px, row_bytes_bound(f, max_cw[f]), count[f], h->n_cu,
                                    kn, qp[f], qbase[f], qlds[f], qslots[f], qfn[f])) path[f] = kPathRoi;
        else path[f] = kPathGeneric;
        any_generic |= path[f] == kPathGeneric;
        any_roi |= path[f] == kPathRoi;
    }
    // Full geometry on the host only where something consumes it.
    const bool all_geo = out_xform != nullptr || h->opt_stats;
    int64_t src_bytes = 0;
    for (int i = 0; i < n_items; i++) {
        const int f = fmt[i];
        if (!all_geo && path[f] == kPathRoi) continue;
        if (!all_geo && path[f] == kPathUniform && i != rep[f]) continue;  // same crop size: rep's geometry
        Geom& g = geo[i];
        const evam_roi* r = items ? &items[i] : nullptr;
        const evam_image& s = srcs[items ? r->src_index : i];
        roi_geometry(f, s.width, s.height, r != nullptr, r ? r->x : 0, r ? r->y : 0, r ? r->w : 0, r ? r->h : 0,
                     cfg->resize_mode, cfg->placement, DW, DH, g);
        if (out_xform) {
            evam_transform& t = out_xform[i];
            t.scale_x = (float)((double)g.rw / g.cw);
            t.scale_y = (float)((double)g.rh / g.ch);
            t.crop_x = g.x0; t.crop_y = g.y0; t.crop_w = g.cw; t.crop_h = g.ch;
            t.pad_x = g.ox; t.pad_y = g.oy;
            t.resized_w = g.rw; t.resized_h = g.rh;
        }
        if (h->opt_stats) src_bytes += item_src_bytes(f, g, DW, DH);
    }

    HP(3);
    // ---- descriptor block (device-resident, re-uploaded only when its bytes change) ----
    // [LUT][ItemDesc x (items of generic groups)][per uniform group: XTab x DW, YTab x DH]
    // Everything in it is a function of the configuration and the geometry, not of the frames, so a new
    // set of frames of the same geometry reuses the resident block.
    size_t nbytes = kLutBytes;
    const size_t desc_off = nbytes;
    int n_desc = 0;
    for (int f = 0; f < 4; f++)
        if (path[f] == kPathGeneric) n_desc += count[f];
    nbytes += sizeof(ItemDesc) * (size_t)n_desc;
    size_t tab_off[4] = {0, 0, 0, 0};
    for (int f = 0; f < 4; f++) {
        if (path[f] != kPathUniform) continue;
        tab_off[f] = nbytes;
        nbytes += sizeof(XTab) * (size_t)DW + sizeof(YTab) * (size_t)DH;
    }
    // ROI groups: [per ROI group: RoiRec x tiles], in a pinned zero-copy slot (PinRing). A group has
    // count x base tiles, plus up to one extra tile per ROI when its longest crops are split in two.
    size_t rec_off[4] = {0, 0, 0, 0}, dyn_bytes = 0;
    if (any_roi) {
        for (int f = 0; f < 4; f++) {
            if (path[f] != kPathRoi) continue;
            rec_off[f] = dyn_bytes;
            dyn_bytes += sizeof(RoiRec) * (size_t)count[f] * (size_t)qbase[f];
            // tail split: up to n_cu ROIs become kn.roi_tail row tiles each
            if (qbase[f] == 1 && kn.roi_tail > 1)
                dyn_bytes += sizeof(RoiRec) * (size_t)std::min(count[f], h->n_cu) * (size_t)(kn.roi_tail - 1);
        }
    }
    h->h_block.resize(nbytes);
    uint8_t* blk = h->h_block.data();
    block_lut(h, cfg, blk);
    int first[4] = {0, 0, 0, 0};
    {
        ItemDesc* desc = reinterpret_cast<ItemDesc*>(blk + desc_off);
        int order = 0;
        for (int f = 0; f < 4; f++) {
            if (path[f] == kPathGeneric) {
                first[f] = order;
                for (int m = mfirst[f]; m < mfirst[f + 1]; m++) {
                    const int i = members[m];
                    const evam_image& s = srcs[items ? items[i].src_index : i];
                    ItemDesc& d = desc[order++];
                    for (int p = 0; p < 3; p++) { d.plane[p] = s.planes[p]; d.pitch[p] = s.pitch[p]; }
                    const Geom& g = geo[i];
                    d.x0 = g.x0; d.y0 = g.y0; d.cw = g.cw; d.ch = g.ch;
                    d.rw = g.rw; d.rh = g.rh; d.ox = g.ox; d.oy = g.oy;
                    d.index = slots ? slots[i] : i;  // the slot offset / stride are launch parameters: the block survives clip-ring steps
                    d.pad_ = 0;
                    d.scale_x = 1. / ((double)g.rw / g.cw);
                    d.scale_y = 1. / ((double)g.rh / g.ch);
                }
            } else if (path[f] == kPathUniform) {
                XTab* xt = reinterpret_cast<XTab*>(blk + tab_off[f]);
                YTab* yt = reinterpret_cast<YTab*>(xt + DW);
                build_tables(geo[rep[f]], DW, DH, h->tab_cache, xt, yt);
            }
        }
    }
    (void)any_generic;
    HP(4);
    HIP_TRY(hipSetDevice(h->device));
    uint8_t* dyn = nullptr;
    const uint8_t* d_dyn = nullptr;
    PinGuard pin_guard{h};
    bool dyn_wc = false;
    if (any_roi) {
        HipRings b;
        b.rec_device = kn.rec_device != 0;
        if (int rc = h->pin.acquire(b, dyn_bytes, &dyn, &d_dyn, &dyn_wc)) return rc;
        pin_guard.armed = true;
        HP(5);
        // Launch order: largest estimated work first (counting sort on 64 buckets of the staged
        // bytes, crop width x touched rows). Workgroups are dispatched in order as slots free, so
        // the long ROIs start first and the short ones fill the tail.
        const bool sort = kn.roi_sort != 0;
        // the frame half of the records, once per source (a record then takes three of its lines from here)
        std::vector<RecFrame>& rfr = h->sc_frames;
        rfr.resize((size_t)n_srcs);
        for (int s = 0; s < n_srcs; s++) rfr[s] = rec_frame(srcs[s]);
        for (int f = 0; f < 4; f++) {
            if (path[f] != kPathRoi) continue;
            RoiRec* rr = reinterpret_cast<RoiRec*>(dyn + rec_off[f]);
            // One record per work unit, assembled in four XMM registers and written as one 64-byte line into its
            // launch slot: the frame's lines, the caller's rect (w <= 0 without items: the full frame), the output
            // index and the tile's rows.
            const RecFrame* rf = rfr.data();
            auto put_rec = [&](int pos, int i, int row0, int row1) {
                const RecFrame& F = rf[items ? items[i].src_index : i];
                const __m128i rect = items ? _mm_loadu_si128(reinterpret_cast<const __m128i*>(&items[i].x)) : _mm_setzero_si128();
                const uint64_t tail = (uint64_t)(uint32_t)(slots ? slots[i] : i) |
                                      ((uint64_t)((uint32_t)(uint16_t)row0 | ((uint32_t)(uint16_t)row1 << 16)) << 32);
                const __m128i l2 = _mm_unpacklo_epi64(F.l[2], rect);
                const __m128i l3 = _mm_unpackhi_epi64(rect, _mm_set_epi64x((long long)tail, 0));
                __m128i* dst = reinterpret_cast<__m128i*>(&rr[pos]);
                if (dyn_wc) {  // write-combined device memory: the 64-byte line as four streaming stores
                    _mm_stream_si128(dst + 0, F.l[0]);
                    _mm_stream_si128(dst + 1, F.l[1]);
                    _mm_stream_si128(dst + 2, l2);
                    _mm_stream_si128(dst + 3, l3);
                } else {
                    _mm_store_si128(dst + 0, F.l[0]);
                    _mm_store_si128(dst + 1, F.l[1]);
                    _mm_store_si128(dst + 2, l2);
                    _mm_store_si128(dst + 3, l3);
                }
            };
            // Work units (one workgroup each): one per ROI, or per row tile of TH rows for outputs taller than one
            // tile. Units launch largest first; beyond the resident workgroups the dispatcher starts each remaining
            // unit as a slot frees up. (Row tiles of a few row groups per ROI, EVAM_PP_ROI_UNIT, measured slower for
            // two rounds and were retired in round 5.)
            const QParams& q = qp[f];
            const int base = qbase[f];
            const int pxr = roi_px(kn.roi_px, DW, false);
            const int rcap = std::max(1, ((kRoiK / pxr) * kThreads) / (DW / pxr));
            int nu = 0;
            if (base == 1) {
                // One unit per ROI (the default), planned in four passes over the ROIs with no unit list
                // (roi_launch_order, evam_geom.h): row groups per ROI, the bytes pre-order, the tail split, one
                // counting sort by (row groups, bytes), the snake deal, and each record written into its slot.
                // Tail split: every ROI does the same pixel work (DW x DH), so when the ROIs do not divide
                // evenly over the CUs the last `tail` ROIs in launch order land as one extra workgroup on
                // `tail` CUs, whose SIMDs then convert 1 / floor(count / n_cu) more pixels than the others and
                // end the launch (profiles/r03s_c3_roi_timeline_lut_dma.json: the last workgroups to finish
                // are those narrow, compute-dense crops). Splitting those ROIs into kn.roi_tail row tiles —
                // as long as every unit stays resident — gives each of the CUs a fraction of an ROI instead.
                // Snake deal: workgroup p starts on XCD p % 8 and within it on CU (p / 8) % 32, so each band of n_cu
                // consecutive positions puts one unit on every CU; reversing every other band gives each CU one large
                // and one small unit per two bands instead of always the k-th largest of every band (per-CU work
                // balance is what bounds a one-round launch: profiles/r05ze_c3_head_split_ab.txt,
                // r05zd_c3_xcd_frames_devrec_ab.txt).
                // Rows per group and groups per ROI depend on an ROI only through its crop width: memoised per
                // handle for this launch's (format, staging buffer, row cap, DH).
                const int mkey[4] = {f, q.buf_bytes, rcap, DH};
                if (memcmp(mkey, h->memo_key, sizeof(mkey)) != 0) {
                    memcpy(h->memo_key, mkey, sizeof(mkey));
                    h->memo_rg.clear();
                }
                if ((int)h->memo_rg.size() <= max_cw[f]) h->memo_rg.resize((size_t)max_cw[f] + 1, 0u);
                uint32_t* rgm = h->memo_rg.data();  // R | groups of the whole height << 16 (0: not yet known)
                auto rg = [&](int cw) {
                    uint32_t& e = rgm[cw];
                    if (!e) {
                        const int R = std::max(1, std::min(std::min(q.buf_bytes / row_bytes_bound(f, cw), rcap), DH));
                        e = (uint32_t)R | ((uint32_t)((DH + R - 1) / R) << 16);
                    }
                    return e;
                };
                HP(6);
                if (kn.roi_xcd && items && h->n_cu >= 8) {
                    // experiment (EVAM_PP_ROI_XCD=1): the sorted units, then each frame's units on one XCD
                    std::vector<int>& un = h->sc_units;  // per sorted position: item, row0, row1, cost
                    un.assign(4 * ((size_t)count[f] * (size_t)std::max(1, kn.roi_tail) + 1), -1);
                    nu = roi_launch_order(members.data() + mfirst[f], count[f], geo.data(), DH, h->n_cu, qslots[f],
                                          kn.roi_tail, sort, false, rg, h->sc_plan, [&](int q, int i, int r0, int r1) {
                                              const int R = (int)(rg(geo[i].cw) & 0xFFFF);
                                              int* u = &un[4 * (size_t)q];
                                              u[0] = i; u[1] = r0; u[2] = r1; u[3] = (r1 - r0 + R - 1) / R;
                                          });
                    std::vector<int>& fr = h->sc_start;
                    std::vector<int>& co = h->sc_bucket;
                    fr.resize(nu);
                    co.resize(nu);
                    for (int q = 0; q < nu; q++) { fr[q] = items[un[4 * q]].src_index; co[q] = un[4 * q + 3]; }
                    roi_xcd_deal(fr.data(), co.data(), nu, n_srcs, h->n_cu, 8, h->sc_slot, h->sc_order);
                    for (int q = 0; q < nu; q++) put_rec(h->sc_slot[q], un[4 * q], un[4 * q + 1], un[4 * q + 2]);
                } else {
                    nu = roi_launch_order(members.data() + mfirst[f], count[f], geo.data(), DH, h->n_cu, qslots[f],
                                          kn.roi_tail, sort, kn.roi_snake != 0, rg, h->sc_plan, put_rec);
                }
                HP(7);
            } else {
                // outputs taller than one tile (DH > TH): row tiles of TH rows per ROI, the same order rules
                std::vector<int>& bucket = h->sc_bucket;
                bucket.resize(n_items);
                std::vector<int>& ord = h->sc_order;
                roi_largest_first(members.data() + mfirst[f], count[f], geo.data(), DH, sort, bucket.data(), ord);
                HP(6);
                std::vector<int>& un = h->sc_units;  // (item, row0, row1, cost) per unit
                un.clear();
                int maxcost = 1;
                for (size_t p = 0; p < ord.size(); p++) {
                    const int i = ord[p];
                    const int R = std::max(1, std::min(std::min(q.buf_bytes / row_bytes_bound(f, geo[i].cw), rcap), DH));
                    for (int t = 0; t < base; t++) {
                        const int y0 = t * q.TH;
                        const int y1 = std::min(DH, (t + 1) * q.TH);
                        const int cost = (y1 - y0 + R - 1) / R;
                        maxcost = std::max(maxcost, cost);
                        un.insert(un.end(), {i, y0, y1, cost});
                    }
                }
                HP(7);
                // stable counting sort of the units by cost, largest first, then the snake deal
                nu = (int)(un.size() / 4);
                std::vector<int>& start = h->sc_start;
                start.assign((size_t)maxcost + 2, 0);
                for (int u = 0; u < nu; u++) start[maxcost - un[4 * u + 3] + 1]++;
                for (int c = 0; c <= maxcost; c++) start[c + 1] += start[c];
                std::vector<int>& order = h->sc_slot;
                order.resize(nu);
                for (int u = 0; u < nu; u++) order[start[maxcost - un[4 * u + 3]]++] = u;
                if (kn.roi_snake) {
                    const int band = std::max(1, h->n_cu);
                    for (int b0 = band; b0 < nu; b0 += 2 * band) std::reverse(order.begin() + b0, order.begin() + std::min(nu, b0 + band));
                }
                for (int pos = 0; pos < nu; pos++) {
                    const int u = order[pos];
                    put_rec(pos, un[4 * u], un[4 * u + 1], un[4 * u + 2]);
                }
            }
            if (dyn_wc && nu > 0) {
                // The records reach device memory before the launch's doorbell. The fence only drains this core's
                // write-combining buffers into the PCIe posted-write stream; a read from the slot cannot complete
                // ahead of those posted writes (PCIe ordering: a read does not pass posted writes), so once it
                // returns every record is in device memory (the HIP runtime publishes host-written device kernel
                // arguments the same way: a read-back of the last byte after the fence).
                _mm_sfence();
                _mm_mfence();
                (void)*reinterpret_cast<const volatile uint32_t*>(reinterpret_cast<const uint8_t*>(&rr[nu - 1]) +
                                                                  sizeof(RoiRec) - 4);
            }
            const int nrec = nu;
            qrec[f] = nrec;
        }
    }
    HP(8);
    const uint8_t* d_block = nullptr;
    {
        HipRings b;
        if (int rc = h->ring.upload(b, h->stream, h->h_block.data(), h->h_block.size(), &d_block)) return rc;
    }
    HP(9);

    // ---- launches ----
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev0, h->stream));
    int launches = 0;
    uint32_t kmask = 0;
    const uint32_t fill = pack_fill(cfg);
    const int color_rgb = cfg->color_order == EVAM_COLOR_RGB;
    const float* lut_d = reinterpret_cast<const float*>(d_block);
    // Kernel-argument items of one uniform launch: members [m0, m0 + n) of format group f.
    auto fill_args = [&](ItemArg* a, int m0, int n) {
        for (int k = 0; k < n; k++) {
            const int i = members[m0 + k];
            const evam_image& s = srcs[items ? items[i].src_index : i];
            for (int p = 0; p < 3; p++) { a[k].plane[p] = s.planes[p]; a[k].pitch[p] = s.pitch[p]; }
            a[k].x0 = geo[i].x0;
            a[k].y0 = geo[i].y0;
            a[k].index = slots ? slots[i] : i;
        }
    };
    for (int f = 0; f < 4; f++) {
        if (path[f] == kPathNone) continue;
        if (path[f] == kPathRoi) {
            QParams& q = qp[f];
            roi_launch_fields(q, reinterpret_cast<const RoiRec*>(d_dyn + rec_off[f]), lut_d, cfg, dst, slot_offset, slot_stride,
                              kn.prio);
            const int64_t grid = qrec[f];
            if (grid > 0x7FFFFFFF) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: too many tiles");
            if (int rc = launch_kernel(qfn[f], dim3((unsigned)grid), dim3(kThreads), qlds[f], h->stream, &q, true)) return rc;
            launches++; kmask |= EVAM_KERNEL_ROI;
            continue;
        }
        if (path[f] == kPathUniform) {
            const Geom& g0 = geo[rep[f]];
            const XTab* xt_d = reinterpret_cast<const XTab*>(d_block + tab_off[f]);
            const YTab* yt_d = reinterpret_cast<const YTab*>(xt_d + DW);
            const XTab* hx = reinterpret_cast<const XTab*>(h->h_block.data() + tab_off[f]);
            const LaunchPlan k = plan_group(f, hx, reinterpret_cast<const YTab*>(hx + DW), strip_pair_ok(f));
            if (!k.family)  // the early decision asked the same function the same question
                return fail(EVAM_PP_ERR_HIP, "evam_pp_run: the interleaved or 16-bit group's plan did not repeat (internal error)");
            auto common = [&](auto& p) {
                p.lut = lut_d;
                p.dst = dst->data;
                p.slot_offset = slot_offset;
                p.slot_stride = slot_stride;
                p.color_rgb = color_rgb;
                p.fill = fill;
            };
            auto tables = [&](auto& p) {
                common(p);
                p.ox = g0.ox;
                p.rw = g0.rw;
                p.xtab = xt_d;
                p.ytab = yt_d;
            };
            TParams& tp = h->sc_tparams;
            switch (k.family) {
            case EVAM_KERNEL_STRIP: common(tp); tp.prio = kn.prio; break;
            case EVAM_KERNEL_BAND: common(tp); tp.prio = kn.prio; tp.ahead = std::max(0, kn.band_ahead); break;
            case EVAM_KERNEL_WAVE: tables(up.w); break;
            case EVAM_KERNEL_STAGED: tables(up.s); break;
            default: tables(up.r); break;
            }
            for (int m0 = mfirst[f]; m0 < mfirst[f + 1]; m0 += kArgItems) {
                const int n = std::min(kArgItems, mfirst[f + 1] - m0);
                fill_args(k.items, m0, n);
                const int64_t grid = (int64_t)n * k.tiles_per_item;
                if (grid > 0x7FFFFFFF) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: too many tiles");
                if (k.family == EVAM_KERNEL_BAND) tp.units = (int)grid;
                // XCD-contiguous tiles: C2 -1.4 %, C4 -3 % kernel time; a grid of one workgroup round or
                // less (C5) gains nothing (profiles/r01ae_sweep_xcd.txt). EVAM_PP_XCD=0/1 forces it.
                if (k.family == EVAM_KERNEL_STAGED) up.s.xcd_remap = kn.xcd >= 0 ? kn.xcd : (int)(grid >= 8 * (int64_t)h->n_cu);
                const dim3 gr = k.gy ? dim3((unsigned)k.gx, (unsigned)k.gy, (unsigned)n) : dim3((unsigned)grid);
                if (int rc = launch_kernel(k.fn, gr, dim3((unsigned)k.block), k.lds, h->stream, k.params,
                                           k.family == EVAM_KERNEL_STAGED))
                    return rc;
                launches++; kmask |= k.family;
            }
            continue;
        }
        const ItemDesc* items_d = reinterpret_cast<const ItemDesc*>(d_block + desc_off) + first[f];
        const TileCfg t = choose_tiles(DW, DH, cfg->out_dtype, kn);
        KParams p{};
        p.items = items_d;
        p.lut = lut_d;
        p.dst = dst->data;
        p.slot_offset = slot_offset;
        p.slot_stride = slot_stride;
        p.DW = DW; p.DH = DH;
        p.TW = t.TW; p.TH = t.TH;
        p.tiles_x = (DW + t.TW - 1) / t.TW;
        const int tiles_y = (DH + t.TH - 1) / t.TH;
        p.tiles_per_item = p.tiles_x * tiles_y;
        const int64_t n_tiles = (int64_t)count[f] * p.tiles_per_item;
        if (n_tiles > 0x7FFFFFFF) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run: too many tiles");
        p.n_tiles = (int)n_tiles;
        p.tw_magic = t.TW > 1 ? (uint32_t)(0xFFFFFFFFu / (uint32_t)t.TW) + 1u : 0u;
        p.offCol = t.offCol; p.offRow = t.offRow;
        p.color_rgb = color_rgb;
        p.fill = fill;
        if (int rc = launch_kernel(generic_kernel(f, cfg->out_dtype, nhwc), dim3((unsigned)n_tiles), dim3(kThreads), t.lds,
                                   h->stream, &p, true))
            return rc;
        launches++; kmask |= EVAM_KERNEL_GENERIC;
    }
    if (any_roi) {
        HipRings b;
        if (int rc = h->pin.fence(b, h->stream)) return rc;
        pin_guard.armed = false;
    }
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = h->opt_timing != 0;
#ifdef EVAM_PP_HOST_PROF
    HP(10);
    static long hp_calls = 0;
    if (++hp_calls > 200) {  // steady state: past warm-up, allocations and code-object loading
        for (int i = 0; i < 12; i++) g_hp[i] += hp_t[i];
        g_hp_n++;
    }
#endif

    h->stats.n_items = n_items;
    h->stats.n_launches = launches;
    h->stats.kernels = kmask;
    h->stats.src_bytes = h->opt_stats ? src_bytes : 0;
    h->stats.dst_bytes = (int64_t)n_items * plane * 3 * esz;
    return EVAM_PP_OK;
}

}  // namespace

extern "C" {

int evam_pp_run(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi* items, int n_items,
                const evam_preproc* cfg, const evam_tensor* dst, evam_transform* out_xform) {
    return run_impl(h, srcs, n_srcs, items, n_items, cfg, dst, nullptr, out_xform);
}

int evam_pp_run_slots(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi* items, int n_items,
                      const evam_preproc* cfg, const evam_tensor* dst, const int32_t* slots, evam_transform* out_xform) {
    if (!slots) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_run_slots: slots is NULL");
    return run_impl(h, srcs, n_srcs, items, n_items, cfg, dst, slots, out_xform);
}

}  // extern "C"

#include "evam_rois_api.h"
#include "evam_jpeg_api.h"
#include "evam_jpeg_dec_api.h"
#include "evam_track_api.h"
#include "evam_detout_api.h"
