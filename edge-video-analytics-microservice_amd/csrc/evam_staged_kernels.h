// evam_pp_staged, the staged kernel (uniform geometry, workgroup-wide staging), and the helpers only it uses: xcd_tile,
// vmcnt_at_most. Source bytes: the row segments of a group of R output rows arrive in LDS by LDS-DMA, one group ahead,
// and taps are LDS byte reads. LDS: the LUT, then NBUF staging buffers of 2 R slots per plane. Waits: each wave counts
// the VMEM operations it issued after a group's DMA and waits vmcnt on that count, then one s_barrier per group.
// Included by evam_pp.hip after evam_kernel_common.h; reopens its anonymous namespace.
#pragma once

namespace {

// Workgroups are dispatched round-robin over the 8 XCDs (block b runs on XCD b % 8). Remap so each
// XCD walks a contiguous run of tiles: neighbouring tiles of one frame share source rows at their
// edges, and those rows then hit the same L2. Bijective for any grid size.
__device__ inline int xcd_tile(int b, int grid) {
    const int q = grid >> 3, r = grid & 7, x = b & 7, i = b >> 3;
    return x < r ? x * (q + 1) + i : r * (q + 1) + (x - r) * q + i;
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

}  // namespace
