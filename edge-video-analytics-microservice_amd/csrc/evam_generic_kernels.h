// evam_pp_kernel, the generic kernel (any geometry per item, every format, dtype and layout: whatever no other family
// plans), and the helpers only it uses: yuv_to_bgr, load_tap, to_bgr. Source bytes: every lane gathers its pixels' four
// taps straight from the frame through L1, nothing is staged. LDS: the LUT, then the tile's column and row tables,
// built on the device. Waits: one __syncthreads() after the tables; the tap loads are pipelined one pixel deep.
// Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

namespace {

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

}  // namespace
