// evam_pp_roi, the ROI kernel (per-item geometry: gvaclassify crops, mixed crops), and wait_vmcnt_stores, which only
// it uses. Not evam_rois_kernels.h (plural): that header holds the kernels that build and consume device-resident
// ROI lists and feed this kernel its records. Source bytes: a group of R output rows' segments, packed back to back
// per plane, arrive in LDS by LDS-DMA while the previous group is converted. LDS: the LUT (itself by LDS-DMA), the
// device-built column and row tables, two staging buffers. Waits: per group one vmcnt that leaves the previous
// group's stores in flight (3 per store step), then one s_barrier. EVAM_PP_TRACE stamps and kAblate stops are inline.
// Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

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
