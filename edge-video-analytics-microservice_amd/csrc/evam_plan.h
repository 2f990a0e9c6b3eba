// evam_plan.h — the host planner of libevam_pp.so: from a format group's geometry, item count and CU count to the
// kernel variant, tile height, wave count, LDS carve, grid shape and per-strip footprint table of its launches,
// plus the tuning knobs and the host's coefficient-table cache. Plain C++ on evam_geom.h and evam_params.h: the
// kernel pointers and the occupancy query come through a backend (below), so tests/native/planner_check.cpp runs the
// planner on the CPU under AddressSanitizer / UBSan with a fake one and checks every bound the kernels rely on.
// Compile with -ffp-contract=off (evam_geom.h).
#ifndef EVAM_PLAN_H
#define EVAM_PLAN_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "evam_geom.h"
#include "evam_params.h"

namespace {
using namespace evam;

struct TileCfg {
    int TW, TH, offCol, offRow, lds;
};

inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

// Tuning and diagnostic knobs. Read from the environment once, when a handle is
// created (evam_pp_create), never on the per-call path. -1 = the measured heuristic default.
struct Knobs {
    int staged = 1, wave = 1, rows = 1, roi = 1;   // kernel families allowed (wave 2 = force)
    int th = -1, tw = -1, xcd = -1;                // staged / generic tiles, XCD-contiguous order
    int nsegx = 0;                                 // staged tile width in 64-column segments (0: widest that fits)
    int stage_r = -1;                              // staged pipeline: rows per group
    int wth = -1, px = 0, reuse = 1, wave_lds = 40 * 1024;
    int roi_th = -1, roi_buf = -1, roi_px = 2;     // roi_buf -1: sized for one round; pixels per lane (1 for odd DW)
    int roi_sort = 1;  // 1: largest estimated bytes first before the stable sort by row groups (alone: equal or
                       // slower, profiles/r04k_ab_lines.txt; with the snake deal below C3 +1.5-2 %,
                       // profiles/r05zf_c3_snake_ab.txt)
    int roi_tail = 4;                              // row tiles per ROI of the uneven tail over the CUs (1: no split)
    int roi_snake = 1;                             // snake deal of the sorted units over the CUs (0: bands in one direction)
    int roi_xcd = 0;                               // 1: each frame's ROIs on one XCD, snake-dealt over its CUs (experiment)
    int strip = 1, strip_th = -1, strip_nw = -1, strip_px = 0;  // strip kernel: allowed (2: forced), rows per
                                                                // tile, waves, px
    int strip_pair = 1;                            // strip kernel: paired-tap DMA where the footprints allow it
    int strip_waves = 16;                          // strip / band kernels: resident waves per CU the tiles are sized for
    int band = 1, band_px = 0;                     // band kernel: allowed (2: forced), pixels per lane
    int band_dd = 1;                               // band kernel: six-column lanes where the column table allows
    int rec_device = 1;                            // ROI records in host-written device memory where mapped (0: pinned host)
    int prio = 1;                                  // progress-based wave priority (strip, band, ROI kernels): C2 +3 %,
                                                   // C4 +3 %, C5 +3-5 %, C1 +9 % (profiles/r04k_ab_lines.txt)
    int band_ahead = 2;                            // band kernel: source rows issued ahead of the current output row's
                                                   // (64: the whole band at once; 2 measured +2 % on C1)
    int host_simd = 1;                             // ROI calls: pass 1 on AVX2 (0: scalar)
    void read() {
        host_simd = env_int("EVAM_PP_HOST_SIMD", host_simd);
        prio = env_int("EVAM_PP_PRIO", prio);
        band_ahead = env_int("EVAM_PP_BAND_AHEAD", band_ahead);
        band = env_int("EVAM_PP_BAND", band); band_px = env_int("EVAM_PP_BAND_PX", band_px);
        band_dd = env_int("EVAM_PP_BAND_DD", band_dd);
        rec_device = env_int("EVAM_PP_REC_DEVICE", rec_device);
        strip = env_int("EVAM_PP_STRIP", strip); strip_th = env_int("EVAM_PP_STRIP_TH", strip_th);
        strip_waves = env_int("EVAM_PP_STRIP_WAVES", strip_waves);
        strip_pair = env_int("EVAM_PP_STRIP_PAIR", strip_pair); strip_nw = env_int("EVAM_PP_STRIP_NW", strip_nw);
        strip_px = env_int("EVAM_PP_STRIP_PX", strip_px);
        staged = env_int("EVAM_PP_STAGED", staged); wave = env_int("EVAM_PP_WAVE", wave);
        rows = env_int("EVAM_PP_ROWS", rows); roi = env_int("EVAM_PP_ROI", roi);
        th = env_int("EVAM_PP_TH", th); tw = env_int("EVAM_PP_TW", tw); xcd = env_int("EVAM_PP_XCD", xcd);
        nsegx = env_int("EVAM_PP_NSEGX", nsegx);
        stage_r = env_int("EVAM_PP_STAGE_R", stage_r);
        wth = env_int("EVAM_PP_WTH", wth); px = env_int("EVAM_PP_PX", px);
        reuse = env_int("EVAM_PP_REUSE", reuse); wave_lds = env_int("EVAM_PP_WAVE_LDS", wave_lds);
        roi_th = env_int("EVAM_PP_ROI_TH", roi_th); roi_buf = env_int("EVAM_PP_ROI_BUF", roi_buf);
        roi_px = env_int("EVAM_PP_ROI_PX", roi_px); roi_sort = env_int("EVAM_PP_ROI_SORT", roi_sort);
        roi_tail = env_int("EVAM_PP_ROI_TAIL", roi_tail); roi_snake = env_int("EVAM_PP_ROI_SNAKE", roi_snake);
        roi_xcd = env_int("EVAM_PP_ROI_XCD", roi_xcd);
    }
};

// Tile shape: up to 512 columns (a whole model-input row when it fits) x enough rows for ~4096 output
// pixels per 256-thread workgroup, so the per-tile table setup is amortised over ~16 pixels per lane.
// EVAM_PP_TW / EVAM_PP_TH override (tuning).
inline TileCfg choose_tiles(int DW, int DH, int out_dtype, const Knobs& k) {
    TileCfg t{};
    t.TW = std::min(DW, 512);
    t.TH = std::max(1, std::min(DH, 4096 / t.TW));
    if (k.tw > 0) t.TW = std::max(1, std::min(DW, k.tw));
    if (k.th > 0) t.TH = std::max(1, std::min(DH, k.th));
    t.offCol = out_dtype != EVAM_DTYPE_U8 ? kLutBytes : 0;
    t.offRow = t.offCol + (int)sizeof(ColEntry) * t.TW;
    t.lds = t.offRow + (int)sizeof(RowEntry) * t.TH;
    return t;
}

struct TabCache {
    int key[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    std::vector<XTab> x;
    std::vector<YTab> y;
};

// OpenCV coefficient tables for the uniform-geometry kernel, indexed by output column / row of the
// DW x DH plane (padding columns / rows get zero weights). Cached: rebuilt only when the geometry changes.
inline void build_tables(const Geom& g, int DW, int DH, TabCache& c, XTab* xt, YTab* yt) {
    const int key[8] = {g.cw, g.ch, g.rw, g.rh, g.ox, g.oy, DW, DH};
    if (memcmp(key, c.key, sizeof(key)) != 0) {
        c.x.assign(DW, XTab{});
        c.y.assign(DH, YTab{});
        build_tables_into(g, DW, DH, c.x.data(), c.y.data());
        memcpy(c.key, key, sizeof(key));
    }
    memcpy(xt, c.x.data(), sizeof(XTab) * DW);
    memcpy(yt, c.y.data(), sizeof(YTab) * DH);
}

struct RowCfg {
    int TW, TH;
};

// Row-kernel tile: TW in {512, 256, 128, 64} (whole 64-pixel segments; 4 waves split them) chosen for
// the least padding lanes, and enough rows for ~4096 pixels per 256-thread workgroup.
inline RowCfg choose_row_tiles(int DW, int DH, const Knobs& k) {
    RowCfg r{512, 8};
    int best = 1 << 30;
    for (int tw : {512, 256, 128, 64}) {
        const int waste = ((DW + tw - 1) / tw) * tw - DW;
        if (waste < best) { best = waste; r.TW = tw; }
    }
    if (k.tw > 0) r.TW = k.tw;
    if (r.TW != 64 && r.TW != 128 && r.TW != 256 && r.TW != 512) r.TW = 512;
    r.TH = std::max(1, std::min(DH, k.th > 0 ? k.th : 4096 / r.TW));
    return r;
}

// ---- kernel variants: the pure half of evam_pp.hip's kernel tables ----
// Per family: the size of each digit of its table (kDims), where a combination of template arguments sits in it
// (index, -1 when a digit is out of range) and which combinations are instantiated (built). evam_pp.hip's
// *Kernels derive from these and add the instantiations; the planner's CPU check builds its fake lookups on the
// same definitions, so both agree on which variants exist.
constexpr int px_digit(int px) { return px == 1 ? 0 : (px == 2 ? 1 : (px == 4 ? 2 : -1)); }

template <int N>
constexpr int table_size(const int (&dims)[N]) {
    int n = 1;
    for (int d : dims) n *= d;
    return n;
}
// Mixed-radix position of the digits v (v[k] in [0, dims[k])), or -1 when one is out of range.
template <int N>
constexpr int table_index(const int (&dims)[N], const int (&v)[N]) {
    int i = 0;
    for (int k = 0; k < N; k++) {
        if (v[k] < 0 || v[k] >= dims[k]) return -1;
        i = i * dims[k] + v[k];
    }
    return i;
}

struct GenericVariants {
    static constexpr int kDims[] = {4, 3, 2};  // format, output kind, NHWC
    static constexpr int index(int f, int o, int nhwc) { return table_index(kDims, {f, o, nhwc}); }
};
struct RowsVariants {
    static constexpr int kDims[] = {4, 2};  // format, output kind (u8 / fp32)
    static constexpr int index(int f, int o) { return table_index(kDims, {f, o}); }
};
struct StagedVariants {
    static constexpr int kDims[] = {4, 2, 2, 3, 1};  // format, output kind (u8 / fp32), R 1 / 2, NSEGX 1 / 2 / 4, NBUF 2
    static constexpr int index(int f, int o, int R, int nsegx, int nbuf) {
        return table_index(kDims, {f, o, R - 1, px_digit(nsegx), nbuf - 2});
    }
    static constexpr bool built(int R, int nsegx, int nbuf) { return staged_shape(R, nbuf) && staged_valid(nsegx, R); }
};
// Interleaved (NHWC) output: PX = 4 only, u8 or fp32 (the planner takes nothing else), see evam_pp_wave.
struct WaveVariants {
    static constexpr int kDims[] = {4, 3, 3, 2, 2};  // format, output kind, PX 1 / 2 / 4, REUSE, NHWC
    static constexpr int index(int f, int o, int px, int reuse, int nhwc) {
        return table_index(kDims, {f, o, px_digit(px), reuse, nhwc});
    }
    static constexpr bool built(int o, int px, int nhwc) { return !nhwc || (px == 4 && o < 2); }
};
// No BGR strip kernel; the interleaved (NHWC) instantiations are fp32 only.
struct StripVariants {
    static constexpr int kDims[] = {3, 3, 2, 2, 2};  // format (NV12 / I420 / BGRx), output kind, PX 1 / 2, paired taps, NHWC
    static constexpr int index(int f, int o, int px, int pr, int nhwc) { return table_index(kDims, {f, o, px - 1, pr, nhwc}); }
    static constexpr bool built(int o, int nhwc) { return !nhwc || o == 1; }
};
// NV12 / I420, u8 / fp32; six-column lanes (DD) with PX = 4 only; the interleaved (NHWC) instantiations are u8, PX = 4.
struct BandVariants {
    static constexpr int kDims[] = {2, 2, 3, 2, 2};  // format (NV12 / I420), output kind (u8 / fp32), PX 1 / 2 / 4, DD, NHWC
    static constexpr int index(int f, int o, int px, int dd, int nhwc) {
        return table_index(kDims, {f, o, px_digit(px), dd, nhwc});
    }
    static constexpr bool built(int o, int px, int dd, int nhwc) { return (!dd || px == 4) && (!nhwc || (o == 0 && px == 4)); }
};

// PX = 2 adjacent pixels per lane by default (round 5; 1 for odd output widths): one dwordx2 store per channel and
// one row setup per 2 pixels, C3 +3.7 % over PX = 1 on one box (profiles/r05p_c3_roi_px_rmax_ab.txt; PX = 4 equals
// PX = 1 there, round 2 measured it 8 % slower: lanes 4 pixels apart spread their LDS tap reads over more dwords).
// (Three staging buffers, EVAM_PP_ROI_NBUF=3, measured neutral or slower for two rounds: retired in round 5.)
// The device-list siblings (DEV): PX = 2, or 1 for odd output widths (EVAM_PP_ROI_PX = 4 is not built for them).
constexpr int roi_px(int px, int DW, bool dev) {
    if (dev) return (px == 2 || px == 4) && DW % 2 == 0 ? 2 : 1;
    return (px == 4 || px == 2) && DW % px == 0 ? px : 1;
}
struct RoiVariants {
    static constexpr int kDims[] = {4, 3, 3, 2};  // format, output kind, PX 1 / 2 / 4, DEV (two staging buffers each)
    static constexpr int index(int f, int o, int px, int dev) { return table_index(kDims, {f, o, px_digit(px), dev}); }
    static constexpr bool built(int px, int dev) { return !dev || px != 4; }
};

// The two facts the planner takes from the GPU runtime come through a backend B, a template parameter as in
// evam_rings.h (evam_pp.hip: HipKernels; tests/native/planner_check.cpp: a fake on the variants above):
//   rows / staged / wave / strip / band / roi (the family's template arguments as runtime values) -> the kernel's
//       opaque host pointer, nullptr where the combination is not built
//   resident(fn, lds) -> workgroups of fn (256 threads, lds bytes of dynamic LDS) resident per CU, >= 1

// What the launches of one uniform-geometry format group share. A plan_* function fills the kernel its plan was
// sized for (from the family's table), the workgroup size, the dynamic LDS and the grid of a launch of n items:
// (gx, gy, n) where gy > 0, else n * tiles_per_item workgroups. plan_uniform adds the family and the parameter
// struct that plan filled.
struct LaunchPlan {
    uint32_t family = 0;     // the family's EVAM_KERNEL_* bit (0: no uniform-geometry kernel serves the group)
    const void* fn = nullptr;
    int block = kThreads, lds = 0;
    int gx = 0, gy = 0, tiles_per_item = 0;
    void* params = nullptr;  // TParams (strip, band), WParams, SParams or RParams
    ItemArg* items = nullptr;  // its items[kArgItems]
};

// One uniform-geometry format group as the plan_* functions see it: the shared geometry `g` (of any item: only x0
// differs), the output plane, the items of the call, the host coefficient tables of the geometry, and how the
// caller wants the result stored.
struct UniformGroup {
    int f;                // FmtId
    const Geom& g;
    int DW, DH, count, out_dtype, n_cu;
    const XTab* xt;       // [DW]
    const YTab* yt;       // [DH]
    uint32_t x0_mask;     // bit r: some item's crop origin x0 has x0 mod 32 == r (0: g.x0's alone)
    const Knobs& kn;
    bool pair_ok;         // strip kernel: the frames' planes allow paired-tap DMA
    bool nhwc;            // interleaved output
    bool nhwc_wave_ok;    // ... and the band / wave kernels' four-pixel stores are aligned
    uint32_t origins() const { return x0_mask ? x0_mask : 1u << (g.x0 & 31); }
};

// Pairs of consecutive visible (non-letterbox) output rows, and how many of them share a source row: the second
// row's first tap is at or above the first row's second tap (vertical upscales).
struct RowSharing { int shared, visible; };
inline RowSharing shared_rows(const YTab* yt, int DH) {
    RowSharing s{0, 0};
    for (int Y = 0; Y + 1 < DH; Y++) {
        const bool pad0 = (yt[Y].b0 | yt[Y].b1) == 0, pad1 = (yt[Y + 1].b0 | yt[Y + 1].b1) == 0;
        if (pad0 || pad1) continue;
        s.visible++;
        s.shared += yt[Y + 1].r0 <= yt[Y].r1;
    }
    return s;
}

// The geometry fields of a strip / band launch: the output plane, the crop and resized sizes, the placement and
// OpenCV's two scale factors.
inline void fill_geometry(TParams& p, const UniformGroup& u) {
    const Geom& g = u.g;
    p.DW = u.DW; p.DH = u.DH;
    p.cw = g.cw; p.ch = g.ch; p.rw = g.rw; p.rh = g.rh; p.ox = g.ox; p.oy = g.oy;
    p.scale_x = 1. / ((double)g.rw / g.cw);
    p.scale_y = 1. / ((double)g.rh / g.ch);
}

// The per-strip footprint table of a strip / band launch: entry (strip group x 8 + wave) names strip
// s = group x nw + wave of `sw` columns (nw <= 8, at most 8 groups: the callers check kSfoot).
inline void fill_sfoot(TParams& p, const UniformGroup& u, int nw, int nstrips, int sw) {
    for (int k = 0; k < kSfoot; k++) {
        const int w = k & 7, s = (k >> 3) * nw + w;
        const int Xv0 = std::max(s * sw, u.g.ox), Xv1 = std::min(std::min(s * sw + sw, u.DW), u.g.ox + u.g.rw) - 1;
        p.sfoot[k] = w < nw && s < nstrips && Xv0 <= Xv1 ? ColSpan{u.xt[Xv0].s0, u.xt[Xv1].s1} : ColSpan{-1, -1};
    }
}

// Wave-row kernel plan for a uniform-geometry group: pixels per lane PX (the widest whose staging
// fits the LDS budget and divides DW), the exact per-tile footprint from the host tables, REUSE when
// consecutive output rows share source rows, and a tile height that gives every CU enough workgroups.
// The kernel stages each item's footprint from that item's own crop origin x0, and the number of
// 16-byte chunks a footprint spans depends on x0's alignment: the segments are sized for the worst
// case over every residue x0 mod 32 present in the group (x0_mask bit r), which covers the 16-byte
// phase of every plane (luma / packed at bpp 1, 3, 4; NV12 chroma 2 (x >> 1); I420 chroma x >> 1).
template <class B>
bool plan_wave(const B& be, const UniformGroup& u, WParams& w, bool& reuse, LaunchPlan& k) {
    const int f = u.f, DW = u.DW, DH = u.DH, count = u.count, out_dtype = u.out_dtype, n_cu = u.n_cu;
    const Geom& g = u.g;
    const Knobs& kn = u.kn;
    const int npc = f == kI420 ? 2 : (f == kNV12 ? 1 : 0);
    const int lut = out_dtype != EVAM_DTYPE_U8 ? kLutBytes : 0;
    const int budget = kn.wave_lds;
    const int want_px = u.nhwc ? 4 : kn.px;  // the interleaved variant exists for PX = 4 alone
    int px = 0, lds = 0;
    w = WParams{};
    const uint32_t x0_mask = u.origins();
    reuse = kn.reuse != 0 && shared_rows(u.yt, DH).shared > 0;
    for (int cand : {4, 2, 1}) {
        if (want_px && cand != want_px) continue;
        if (cand > 1 && DW % cand) continue;
        const int tw = 64 * cand;
        int mY = 0, mC = 0;
        wave_segments(f, g.ox, g.rw, DW, u.xt, x0_mask, tw, mY, mC);
        const int segY = std::max(16, 16 * mY), segC = npc ? std::max(16, 16 * mC) : 0;
        const int wave_bytes = 2 * (2 * segY + 2 * npc * segC);
        const int need = lut + 4 * wave_bytes;
        if (need > budget && !(want_px && need <= 64 * 1024)) continue;
        px = cand;
        w.segY = segY;
        w.segC = segC;
        w.wave_bytes = wave_bytes;
        w.offBuf = lut;
        lds = need;
        break;
    }
    if (!px) return false;
    w.DW = DW; w.DH = DH;
    w.tiles_x = (DW + 64 * px - 1) / (64 * px);
    // Rows per wave: enough that the whole grid is resident at once (one round: a second round repeats
    // every workgroup's prologue latency at the tail), counting at most 4 resident workgroups per CU —
    // longer per-wave row runs amortise the prologue better than more waves hide latency. C1: 16-row
    // tiles at the 5 workgroups per CU its registers allow ran 1.6 rounds, 31.9 us; 28-row tiles (one
    // round at 5 per CU) 31.6 us; 32-row tiles (one round at 4 per CU) 29.6 us (profiles/r02r_c1_sweep.txt).
    k.fn = be.wave(f, out_dtype, px, reuse, u.nhwc);
    const int per_cu = std::min(4, be.resident(k.fn, lds));
    const int64_t slots = (int64_t)n_cu * per_cu;
    int64_t rpw = ((int64_t)count * w.tiles_x * DH + 4 * slots - 1) / (4 * slots);
    rpw = std::max<int64_t>(2, std::min<int64_t>(32, rpw));
    w.TH = std::max(1, std::min(std::min(DH, 4 * 64), kn.wth > 0 ? kn.wth : (int)(4 * rpw)));  // <= 64 rows per wave
    w.tiles_per_item = w.tiles_x * ((DH + w.TH - 1) / w.TH);
    if ((int64_t)count * w.tiles_per_item > 0x7FFFFFFF) return false;
    k.block = kThreads;
    k.lds = lds;
    k.gy = 0;
    k.tiles_per_item = w.tiles_per_item;
    return true;
}

// Strip-kernel plan for a uniform 4:2:0 group (fills everything in TParams but the items, LUT, output
// and colour fields).
//  * Pixels per lane PX: 2 (128-column strips: one ~480-byte DMA segment per source row at 3.75x) where
//    the output has at least 4 such strips per row and a strip's footprint fits one 1 KB DMA instruction;
//    the strip pattern's data movement alone is 3 us faster at 128 columns than at 64
//    (profiles/r03c_strip_bw.txt).
//  * Waves per workgroup: 4..8 strips with the fewest idle waves.
//  * Tile height: about EVAM_PP_STRIP_WAVES (16) waves per CU over the whole launch (the data-movement
//    microbenchmark's best: fewer, longer-lived waves beat a full 32), at most 64 rows (the lane-held row
//    table).
//  * Ring depth: kStripD = 2.
//  * Paired taps (pr): both source rows of a plane in one LDS-DMA instruction when every strip's footprint is at
//    most 32 chunks (512 B) per row (I420 chroma: 16, four segments per instruction): 2 instructions per row
//    instead of 4 (NV12) or 6 (I420), 1 instead of 2 (BGRx). EVAM_PP_STRIP_PAIR=0 keeps one row per instruction.
// Returns false when the geometry does not suit it: outputs wider than kMaxStrips strips, footprints over
// 1 KB per strip, or consecutive output rows that share source rows (vertical upscales: the wave kernel's
// REUSE path).
template <class B>
bool plan_strip(const B& be, const UniformGroup& u, TParams& p, LaunchPlan& k) {
    const int f = u.f, DW = u.DW, DH = u.DH, count = u.count, out_dtype = u.out_dtype;
    const Geom& g = u.g;
    const Knobs& kn = u.kn;
    if (f != kNV12 && f != kI420 && f != kBGRX) return false;
    const RowSharing rs = shared_rows(u.yt, DH);
    if (kn.strip != 2 && rs.shared * 8 > rs.visible) return false;  // more than 1 in 8 rows re-stages a row
    const uint32_t x0_mask = u.origins();
    const int npc = f == kI420 ? 2 : (f == kBGRX ? 0 : 1);
    int mY = 0, mC = 0;
    int px = 0;
    for (int cand : {2, 1}) {
        if (kn.strip_px > 0 && cand != kn.strip_px) continue;
        // 128-column strips only where they still give a workgroup 4 strips per row: C5 (224 columns: two
        // 128-column strips, the second 3/4 full) runs 13.0 us in four 64-column strips and 15.6 us in
        // two 128-column ones (profiles/r03g_c5_px.txt)
        if (cand == 2 && (DW + 127) / 128 < 4 && kn.strip_px != 2) continue;
        wave_segments(f, g.ox, g.rw, DW, u.xt, x0_mask, 64 * cand, mY, mC);
        const int cap = strip_slot(f, cand) / 16;  // chunks of one slot
        if (mY <= cap && mC <= cap) { px = cand; break; }
    }
    if (!px) return false;
    const int nstrips = (DW + 64 * px - 1) / (64 * px);
    if (nstrips > kMaxStrips) return false;
    const int pr = kn.strip_pair && u.pair_ok && mY <= 32 && (npc == 0 || (npc == 1 && mC <= 32) || (npc == 2 && mC <= 16)) ? 1 : 0;
    // one ring entry: 2 luma + 2 x npc chroma segments (paired: 1 KB per plane group)
    const int grp_bytes = pr ? (npc ? 2048 : 1024) : (2 + 2 * npc) * strip_slot(f, px);
    int nw = 4, best = 1 << 30;
    for (int c = 4; c <= 8; c++) {
        const int idle = (nstrips + c - 1) / c * c - nstrips;
        if (idle < best) { best = idle; nw = c; }
    }
    if (nstrips < 4) nw = nstrips;
    if (kn.strip_nw > 0) nw = std::min(8, kn.strip_nw);
    p.nw = nw;
    p.tiles_x = (nstrips + nw - 1) / nw;
    const int lut_static = out_dtype != EVAM_DTYPE_U8 ? kLutBytes : 16;  // the kernel's static LDS
    const int wg_target = std::max(1, std::min(32, kn.strip_waves) / nw);
    p.wave_bytes = kStripD * grp_bytes;
    const int lds = nw * p.wave_bytes + 16;  // dynamic LDS; + 16: a right-edge tap reads past its footprint (weight 0)
    if (lds + lut_static > 64 * 1024) return false;
    k.fn = be.strip(f, out_dtype, px, pr, u.nhwc);
    // (resident() counts 256-thread workgroups; this one has 64 * nw threads. Kept: it decides measured plans.)
    const int res = std::max(1, std::min(wg_target, be.resident(k.fn, lds)));
    const int64_t slots = (int64_t)u.n_cu * res;
    const int64_t work = (int64_t)std::min(count, kArgItems) * p.tiles_x * DH;
    int th = (int)std::max<int64_t>(1, (work + slots - 1) / slots);
    th = std::max(th, std::min(DH, kStripD));
    if (kn.strip_th > 0) th = kn.strip_th;
    p.TH = std::max(1, std::min(std::min(DH, 64), th));
    p.tiles_per_item = p.tiles_x * ((DH + p.TH - 1) / p.TH);
    fill_geometry(p, u);
    fill_sfoot(p, u, nw, nstrips, 64 * px);
    if ((p.tiles_x - 1) * 8 + nw > kSfoot) return false;
    if ((int64_t)std::min(count, kArgItems) * p.tiles_per_item > 0x7FFFFFFF) return false;
    // grid (tile column, tile row, item), dispatched in that order (the C2 data movement in the strip pattern takes
    // 1.7 us longer with each XCD on its own run of tiles, profiles/r03c_strip_bw.txt)
    k.block = 64 * nw;
    k.lds = lds;
    k.gx = p.tiles_x;
    k.gy = (DH + p.TH - 1) / p.TH;
    k.tiles_per_item = p.tiles_per_item;
    return true;
}


// Band-kernel plan for a uniform 4:2:0 group whose consecutive output rows share source rows (vertical
// upscales, C1). Fills the geometry, strips, bands and LDS fields of TParams (not items, LUT, output,
// colour).
//  * PX: the widest of 4 / 2 / 1 adjacent columns per lane that divides DW and whose strip footprint fits
//    one DMA instruction (64 chunks) per row.
//  * Band height TH: about EVAM_PP_STRIP_WAVES (16) waves per CU over the launch (one round), at most 64
//    (the lane-held row table), lowered until the band's staged rows fit the LDS.
//  * LDS per wave: the most luma rows any band reads (nrY, from the host's row table) and the chroma rows
//    they can span at either crop-origin parity (nrY / 2 + 1).
// Returns false for geometries it does not suit (fewer than 1 in 8 rows sharing source rows, footprints
// over 1 KB, outputs wider than kMaxStrips strips).
template <class B>
bool plan_band(const B& be, const UniformGroup& u, TParams& p, LaunchPlan& k) {
    const int f = u.f, DW = u.DW, DH = u.DH, count = u.count, out_dtype = u.out_dtype, n_cu = u.n_cu;
    const Geom& g = u.g;
    const Knobs& kn = u.kn;
    const YTab* yt = u.yt;
    if (f != kNV12 && f != kI420) return false;
    const RowSharing rs = shared_rows(yt, DH);
    if (kn.band != 2 && rs.shared * 8 <= rs.visible) return false;
    const uint32_t x0_mask = u.origins();
    const int npc = f == kI420 ? 2 : 1;
    int mY = 0, mC = 0;
    int px = 0, nw = 0, lds = 0;
    for (int cand : {4, 2, 1}) {
        if (kn.band_px > 0 && cand != kn.band_px) continue;
        if (u.nhwc && cand != 4) continue;  // the interleaved variant exists for PX = 4 alone
        if (DW % cand) continue;
        wave_segments(f, g.ox, g.rw, DW, u.xt, x0_mask, 64 * cand, mY, mC);
        if (mY <= 64 && mC <= 64) { px = cand; break; }
    }
    if (!px) return false;
    const int nstrips = (DW + 64 * px - 1) / (64 * px);
    if (nstrips > kMaxStrips) return false;
    p.segY = 16 * std::max(1, mY);
    p.segC = 16 * std::max(1, mC) * npc;  // I420: the U and V rows side by side
    const int lut_static = out_dtype == EVAM_DTYPE_F32 ? kLutBytes : 16;
    const int per_launch = std::min(count, kArgItems);
    const int64_t want = (int64_t)std::max(1, std::min(64, kn.strip_waves)) * n_cu;
    const int64_t band_rows = (int64_t)per_launch * nstrips * DH;
    // Small batches (fewer band rows than the waves the chip is sized for: C1 at 1-4 frames) run faster on the wave
    // kernel: 7.4 vs 8.1 us per launch at 1, 2 and 4 frames, while at 8 frames the band kernel is 19 % ahead
    // (profiles/r04i_c1_small_batch_ab.txt)
    if (band_rows <= want && kn.band != 2 && kn.strip_th <= 0) return false;
    int th = (int)std::max<int64_t>(2, (band_rows + want - 1) / want);
    if (kn.strip_th > 0) th = kn.strip_th;
    th = std::max(1, std::min(std::min(DH, 64), th));
    for (;; th--) {
        int nrY = 1;
        for (int Y0 = 0; Y0 < DH; Y0 += th) {
            int lo = -1, hi = -1;
            for (int Y = Y0; Y < std::min(DH, Y0 + th); Y++) {
                if ((yt[Y].b0 | yt[Y].b1) == 0) continue;  // letterbox row
                if (lo < 0) lo = yt[Y].r0;
                hi = yt[Y].r1;
            }
            if (lo >= 0) nrY = std::max(nrY, hi - lo + 1);
        }
        p.nrY = nrY;
        p.wave_bytes = nrY * p.segY + (nrY / 2 + 1) * p.segC;
        nw = std::min(4, nstrips);  // a workgroup: up to four strips of one band
        lds = nw * p.wave_bytes + 16;  // + 16: a right-edge tap reads past its footprint (weight 0)
        if (lds + lut_static <= 64 * 1024 && nrY <= 64) break;  // <= 64 rows: one lane of the wait table per row
        if (th == 1) return false;
    }
    p.TH = th;
    p.nstrips = nstrips;
    p.tiles_per_item = nstrips * ((DH + th - 1) / th);  // wave units per item
    fill_geometry(p, u);
    p.nw = nw;
    p.tiles_x = (nstrips + nw - 1) / nw;  // strip groups
    if ((p.tiles_x - 1) * 8 + nw > kSfoot) return false;
    fill_sfoot(p, u, nw, nstrips, 64 * px);
    const bool dd = px == 4 && kn.band_dd && band_six_columns(u.xt, DW, x0_mask);
    k.fn = be.band(f, out_dtype, px, dd, u.nhwc);
    k.block = 64 * nw;
    k.lds = lds;
    k.gx = p.tiles_x;
    k.gy = (DH + th - 1) / th;
    k.tiles_per_item = p.tiles_per_item;
    return (int64_t)per_launch * p.tiles_per_item <= 0x7FFFFFFF;
}

// Staged-kernel plan for a uniform group (u8 / fp32, planar): fills the geometry, tile and LDS fields of SParams.
// Returns false where no tile width fits (the row kernel serves those) or EVAM_PP_STAGED=0.
template <class B>
bool plan_staged(const B& be, const UniformGroup& u, SParams& sp, LaunchPlan& k) {
    const int f = u.f, DW = u.DW, DH = u.DH, count = u.count, out_dtype = u.out_dtype, n_cu = u.n_cu;
    const Geom& g = u.g;
    const Knobs& kn = u.kn;
    // Tile width: the widest of 256 / 128 columns whose staged row segment (the exact widest footprint of
    // any tile and crop origin of this group) fits the kernel's 1 KB slot.
    auto seg_bytes = [&](int tw) {
        int mY = 0, mC = 0;
        wave_segments(f, g.ox, g.rw, DW, u.xt, u.x0_mask, tw, mY, mC);
        return 16 * std::max(1, std::max(mY, mC));
    };
    int nsegx = 0;
    if (kn.staged)
        for (int n : {4, 2}) {  // (64 columns would need R % 4 == 0: the row kernel serves those)
            if (seg_bytes(64 * n) <= kSlot) { nsegx = n; break; }
        }
    if (nsegx && kn.nsegx > 0 && kn.nsegx < nsegx && 2 % (4 / kn.nsegx) == 0) nsegx = kn.nsegx;
    if (!nsegx) return false;
    // Pipeline shape: R output rows per group, NBUF staging buffers (NBUF - 1 groups of DMA in
    // flight).
    int R = kn.stage_r > 0 ? kn.stage_r : 2, nbuf = 2;
    if (!staged_shape(R, nbuf) || !staged_valid(nsegx, R)) { R = 2; nbuf = 2; }
    sp = SParams{};
    sp.DW = DW; sp.DH = DH;
    const int tw = 64 * nsegx;
    sp.tiles_x = (DW + tw - 1) / tw;
    // ~4096 pixels per workgroup, but short enough tiles that small batches still put
    // 8 workgroups on every CU (a whole clip-ring step is only 32 x 224 x 224 pixels).
    // At most 16 rows: C4 (tw 128) runs 3-7 % faster at 16 than at 32 (profiles/r01ad_sweep_th*.txt).
    int th = std::max(2, std::min(16, 4096 / tw));
    const int64_t cols = (int64_t)std::min(count, kArgItems) * sp.tiles_x;
    const int64_t want = 8 * (int64_t)n_cu;
    if (cols * ((DH + th - 1) / th) < want) th = (int)std::max<int64_t>(2, cols * DH / want);
    sp.TH = std::max(1, std::min(std::min(DH, 64), kn.th > 0 ? kn.th : th));  // <= 64: lane-held rows
    sp.TH = std::min(64, (sp.TH + R - 1) / R * R);
    sp.tiles_per_item = sp.tiles_x * ((DH + sp.TH - 1) / sp.TH);
    const int np = f == kI420 ? 3 : (f == kNV12 ? 2 : 1);
    sp.offBuf = out_dtype == EVAM_DTYPE_F32 ? kLutBytes : 0;
    sp.slot_bytes = seg_bytes(tw);  // <= the kernel's SLOT_MAX (tile choice above)
    sp.buf_bytes = 2 * R * np * sp.slot_bytes;
    sp.ntcol = sp.tiles_x <= kTCols ? sp.tiles_x : 0;
    for (int c = 0; c < sp.ntcol; c++) {
        const int Xv0 = std::max(c * tw, g.ox), Xv1 = std::min(std::min(c * tw + tw, DW), g.ox + g.rw) - 1;
        sp.tcol[c] = Xv0 <= Xv1 ? ColSpan{u.xt[Xv0].s0, u.xt[Xv1].s1} : ColSpan{-1, -1};
    }
    k.fn = be.staged(f, out_dtype, R, nsegx, nbuf);
    k.block = kThreads;
    k.lds = sp.offBuf + nbuf * sp.buf_bytes;
    k.gy = 0;
    k.tiles_per_item = sp.tiles_per_item;
    return true;
}

// Row-kernel plan for a uniform group (u8 / fp32, planar): the tiles of choose_row_tiles. Serves every geometry.
template <class B>
bool plan_rows(const B& be, const UniformGroup& u, RParams& r, LaunchPlan& k) {
    const int DW = u.DW, DH = u.DH;
    const RowCfg rc = choose_row_tiles(DW, DH, u.kn);
    r = RParams{};
    r.DW = DW; r.DH = DH;
    r.TW = rc.TW; r.TH = rc.TH;
    r.tiles_x = (DW + rc.TW - 1) / rc.TW;
    r.tiles_per_item = r.tiles_x * ((DH + rc.TH - 1) / rc.TH);
    r.nsegx = rc.TW / 64;
    k.fn = be.rows(u.f, u.out_dtype);
    k.block = kThreads;
    k.lds = u.out_dtype == EVAM_DTYPE_F32 ? kLutBytes : 0;
    k.gy = 0;
    k.tiles_per_item = r.tiles_per_item;
    return true;
}

// The parameter structs of a uniform group's plan that are not kept on the handle (TParams is: 3.5 KB).
struct UniformParams {
    WParams w;
    SParams s;
    RParams r;
};

// The kernel choice for a uniform-geometry format group, in the one place that holds its order and guards:
// strip, then band, then wave, then staged, then rows; the first family that is allowed (the EVAM_PP_STRIP / _BAND /
// _WAVE / _STAGED knobs; 2 forces strip, band or wave past the others), instantiated for the output (layout,
// element size) and whose plan takes the geometry serves the group. run_impl asks twice with the same arguments:
// ahead of the descriptor block for interleaved and 16-bit groups (family 0: the generic kernel serves the group,
// which needs its descriptors in the block), and at the launch for every uniform group.
//  * strip: planar in every element type; interleaved in fp32 (12-byte stores, dword-aligned as the elements are).
//  * band: u8 / fp32 planar; interleaved u8 with four-pixel stores where they are aligned (nhwc_wave_ok).
//  * wave: where consecutive output rows share source rows (vertical upscale: REUSE), forced, or interleaved (four-
//    pixel stores, nhwc_wave_ok); for downscales the staged kernel's deeper shared staging is faster.
//  * staged, rows: planar u8 / fp32 only (not instantiated for 2-byte elements or interleaved stores).
template <class B>
LaunchPlan plan_uniform(const B& be, const UniformGroup& u, TParams& t, UniformParams& up) {
    const Knobs& kn = u.kn;
    const bool nhwc = u.nhwc, half = out_kind(u.out_dtype) == 2;
    LaunchPlan k;
    bool reuse = false;
    if (kn.strip && kn.wave != 2 && (!nhwc || u.out_dtype == EVAM_DTYPE_F32) && plan_strip(be, u, t, k)) {
        k.family = EVAM_KERNEL_STRIP; k.params = &t; k.items = t.items;
    } else if (kn.band && kn.wave != 2 && kn.strip != 2 && !half &&
               (!nhwc || (u.out_dtype == EVAM_DTYPE_U8 && u.nhwc_wave_ok)) && plan_band(be, u, t, k)) {
        k.family = EVAM_KERNEL_BAND; k.params = &t; k.items = t.items;
    } else if (kn.wave && (!nhwc || u.nhwc_wave_ok) && plan_wave(be, u, up.w, reuse, k) &&
               (reuse || kn.wave == 2 || nhwc)) {
        k.family = EVAM_KERNEL_WAVE; k.params = &up.w; k.items = up.w.items;
    } else if (nhwc || half) {
        k = LaunchPlan{};
    } else if (plan_staged(be, u, up.s, k)) {
        k.family = EVAM_KERNEL_STAGED; k.params = &up.s; k.items = up.s.items;
    } else {
        plan_rows(be, u, up.r, k);
        k.family = EVAM_KERNEL_ROWS; k.params = &up.r; k.items = up.r.items;
    }
    return k;
}

// ROI-kernel plan for one format group with per-item geometry: the tile height, the LDS carve and the
// staging buffer size, sized for the widest crop of the group (max_row_bytes = row_bytes_bound of it).
// Returns false when the group needs the generic kernel (outputs wider than kRoiK x 256 pixels, taller
// than 65535 rows, or a crop so wide that one output row's segments overflow the LDS budget).
// The staging buffers are sized so that the whole grid fits on the chip in one round when it can: a ROI
// batch is about one workgroup per CU slot (C3: 1,600 ROIs), and a second round starts its workgroups
// only when first-round ones finish, paying record, geometry and setup latency again at the tail
// (C3 with 6 instead of 7 resident per CU: the 64 smallest ROIs started at ~32 us and ended the launch,
// profiles/r02r_c3_roi_timeline_before.json). Occupancy is capped by the kernel's registers
// (kRoiWavesPerSimd); the buffers take what that occupancy leaves of the LDS (allocated in 1 KB
// granules, checked against the runtime's occupancy calculator), between the widest crop's row and
// 12 KB (EVAM_PP_ROI_BUF fixes it). `slots`: workgroups resident at once with that carve.
constexpr int kRoiWavesPerSimd = 7;  // evam_pp_roi<*, *, 1> at kRoiK = 6: <= 72 VGPRs
template <class B>
bool plan_roi(const B& be, int f, int DW, int DH, int out_dtype, int px, int max_row_bytes, int count, int n_cu,
              const Knobs& kn, QParams& q, int& base_tiles, int& lds, int64_t& slots, const void*& fn, bool dev = false) {
    if (DW > kRoiK * kThreads || DH > 65535) return false;
    q.DW = DW; q.DH = DH;
    q.TH = (int64_t)DW * DH <= 32768 ? DH : std::max(8, std::min(DH, 16384 / DW));
    if (kn.roi_th > 0) q.TH = std::max(1, std::min(DH, kn.roi_th));
    base_tiles = (DH + q.TH - 1) / q.TH;
    q.offXT = out_dtype != EVAM_DTYPE_U8 ? kLutBytes : 0;
    q.offYT = q.offXT + (int)sizeof(XTab) * DW;
    q.offBuf = q.offYT + (int)sizeof(YTab) * q.TH;
    const int64_t grid = (int64_t)count * base_tiles;
    const int per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(kRoiWavesPerSimd, (grid + n_cu - 1) / n_cu));
    const int pxv = roi_px(px, DW, dev);
    const uint32_t qw = (uint32_t)(DW / pxv);
    q.mqw = qw > 1 ? (uint32_t)((0x100000000ull + qw - 1) / qw) : 0u;
    const int nb = 2;
    int buf = kn.roi_buf;
    if (buf <= 0) buf = std::min(12 * 1024, ((((160 * 1024) / per_cu) & ~1023) - q.offBuf) / nb & ~15);
    q.buf_bytes = (std::max(buf, max_row_bytes) + 15) & ~15;
    lds = q.offBuf + nb * q.buf_bytes;
    if (q.buf_bytes > 32 * 1024 || lds > 160 * 1024) return false;
    fn = be.roi(f, out_dtype, pxv, dev);
    int res = be.resident(fn, lds);
    while (kn.roi_buf <= 0 && res < per_cu && q.buf_bytes - 512 >= max_row_bytes) {
        q.buf_bytes -= 512;
        lds -= 512 * nb;
        res = be.resident(fn, lds);
    }
    slots = (int64_t)n_cu * res;
    return true;
}

}  // namespace

#endif  // EVAM_PLAN_H
