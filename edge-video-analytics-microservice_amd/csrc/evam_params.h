// evam_params.h — what the kernels, the host planner (evam_plan.h) and the host path of libevam_pp.so share: the
// sizes the kernels are written for, the kernel-argument structs and the device-side descriptors. Plain C++ with no
// HIP type, so tests/native/planner_check.cpp compiles it for the host alone (tests/test_native_asan.py).
//
// Everything sits in an anonymous namespace, as the rest of evam_pp.hip's internals do: the kernels take these
// structs by value, so their namespace is part of every kernel's symbol.
#ifndef EVAM_PARAMS_H
#define EVAM_PARAMS_H

#include <stddef.h>
#include <stdint.h>

#include "evam_geom.h"

namespace {
using namespace evam;

// A pair of source columns in a kernel-argument table (SParams::tcol, TParams::sfoot): HIP's int2 in layout
// (8 bytes, 8-byte aligned), spelled out so that a host compiler knows it.
struct alignas(8) ColSpan {
    int x, y;
};
static_assert(sizeof(ColSpan) == 8, "ColSpan layout");

// ------------------------------------------------------------------------------------------------
// constants
// ------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;

constexpr int kLutBytes = 3 * 256 * 4;
// Output kind of a kernel instantiation (the OUT template parameter): 0 = u8, 1 = fp32 from the table, 2 = a 2-byte
// element (fp16 or bf16: the same kernels, only the table's contents differ). The table section keeps 4-byte
// entries for OUT = 2 with the 16-bit pattern in the low half, so vfinal's byte offsets, the LDS carve and
// every kLutBytes term of the planners are those of fp32; the kernels read the low u16 of an entry.
constexpr int out_kind(int out_dtype) {
    return out_dtype == EVAM_DTYPE_U8 ? 0 : (out_dtype == EVAM_DTYPE_F32 ? 1 : 2);
}
constexpr int out_esz(int out) { return out == 1 ? 4 : (out == 2 ? 2 : 1); }

// ------------------------------------------------------------------------------------------------
// device-side descriptors
// ------------------------------------------------------------------------------------------------
struct alignas(16) ItemDesc {
    const uint8_t* plane[3];
    int32_t pitch[3];
    int32_t x0, y0, cw, ch;  // effective crop in source pixels
    int32_t rw, rh, ox, oy;  // resized size, placement in the DW x DH plane
    int32_t index;    // item index in the call: output slot = slot_offset + index * slot_stride
    int32_t pad_;
    double scale_x, scale_y; // OpenCV: 1. / ((double)rw / cw)
};
static_assert(sizeof(ItemDesc) == 96, "ItemDesc layout");

struct KParams {
    const ItemDesc* items;
    const float* lut;  // [3][256]
    void* dst;
    int slot_offset, slot_stride;  // output slot of item i = slot_offset + i * slot_stride
    int DW, DH;
    int TW, TH, tiles_x, tiles_per_item, n_tiles;
    uint32_t tw_magic;  // ceil(2^32 / TW) (TW > 1)
    int offCol, offRow; // LDS carve: LUT at 0 (fp32 out), column table, row table
    int color_rgb;
    uint32_t fill;      // packed u8 fill, output channel order
};

// Per output column of a tile: absolute byte offsets of the two horizontal taps inside a source row.
struct alignas(16) ColEntry {  // 16 B
    int32_t oY0, oY1;  // luma / packed-pixel byte offsets of tap 0 / tap 1 (always valid addresses)
    int32_t oC0;       // chroma byte offset of tap 0 (NV12: U of the UV pair; I420: U/V plane column)
    uint16_t a0, a1;   // 11-bit horizontal weights << 4 (see vresize); both 0: the column shows padding
};
// Per output row of a tile: byte offsets of the two vertical taps' rows inside the planes.
struct alignas(16) RowEntry {  // 32 B
    int32_t y0, y1;   // row offsets in the luma / packed plane (always valid addresses)
    int32_t c0, c1;   // row offsets in the chroma plane (NV12: UV; I420: U)
    int32_t b0, b1;   // 11-bit vertical weights << 8 (see vresize); both 0: the row shows padding
    int32_t v0, v1;   // I420: row offsets in the V plane, which has its own pitch; else 0
};

// Per-item arguments of the uniform-geometry kernels (staged / wave / rows), carried in the launch's
// kernel arguments: every item of such a launch shares crop size, resized size and placement, so an
// item differs only in its frame (planes, pitches), its crop origin and its output slot. Passing them
// in the kernarg segment means a new set of frames (a decoder's next surfaces, a rotating frame pool)
// costs no descriptor upload and no cross-stream wait; launches take up to kArgItems items each.
struct ItemArg {  // 48 B
    const uint8_t* plane[3];
    int32_t pitch[3];
    int32_t x0, y0;   // crop origin in source pixels
    int32_t index;    // item index in the call: output slot = slot_offset + index * slot_stride
};
static_assert(sizeof(ItemArg) == 48, "ItemArg layout");
constexpr int kArgItems = 64;  // 3 KB of items per launch; the whole parameter block stays < 4 KB


struct RParams {
    ItemArg items[kArgItems];
    int ox, rw;          // uniform placement / resized width
    const float* lut;    // [3][256]
    const XTab* xtab;    // [DW]
    const YTab* ytab;    // [DH]
    void* dst;
    int slot_offset, slot_stride;  // output slot of item i = slot_offset + i * slot_stride
    int DW, DH;
    int TW, TH, tiles_x, tiles_per_item;
    int nsegx;           // TW / 64 column segments per tile row
    int color_rgb;
    uint32_t fill;
};

constexpr int kSlot = 1024;  // bytes of one staged source-row segment = one wave-wide 16 B/lane LDS-DMA

struct SParams {
    ItemArg items[kArgItems];
    int ox, rw;          // uniform placement / resized width
    const float* lut;    // [3][256]
    const XTab* xtab;    // [DW]
    const YTab* ytab;    // [DH]
    void* dst;
    int slot_offset, slot_stride;  // output slot of item i = slot_offset + i * slot_stride
    int DW, DH;
    int TH, tiles_x, tiles_per_item;
    int offBuf;          // LDS offset of staging buffer 0 (after the LUT)
    int buf_bytes;       // one staging buffer: 2 R planes x slot_bytes
    int slot_bytes;      // one staged row segment: the widest 16-byte-aligned footprint of the launch
    int color_rgb;
    uint32_t fill;
    int xcd_remap;       // 1: consecutive tiles land on one XCD (shared halo rows stay in one L2)
    int ntcol;           // tiles_x when <= kTCols (tcol valid), else 0 (the kernel reads xtab)
    ColSpan tcol[16];    // per tile column: crop-relative source columns of its first / last visible
                         // output column's taps, or (-1, -1) for a tile of padding columns only
};
constexpr int kTCols = 16;

struct WParams {
    ItemArg items[kArgItems];
    int ox, rw;          // uniform placement / resized width
    const float* lut;    // [3][256]
    const XTab* xtab;    // [DW]
    const YTab* ytab;    // [DH]
    void* dst;
    int slot_offset, slot_stride;  // output slot of item i = slot_offset + i * slot_stride
    int DW, DH;
    int TH, tiles_x, tiles_per_item;
    int offBuf;          // LDS offset of the per-wave staging areas (after the LUT)
    int segY, segC;      // bytes of one staged luma / chroma row segment (multiples of 16)
    int wave_bytes;      // one wave's staging area (two buffers)
    int color_rgb;
    uint32_t fill;
};

static_assert(sizeof(evam_roi) == 20, "evam_roi layout");

// One ROI tile in launch order, self-contained: its source frame's planes and size next to the caller's
// rect, the item index (output slot) and the output rows the tile covers, so a workgroup needs one
// 64-byte scalar load (one round trip over PCIe from the pinned descriptor slot) before it can resolve
// the geometry. (A 16-byte record with the frames in the kernel arguments measured slower: the frame
// lookup is a second dependent load, profiles/r02r_c3_records.txt.)
struct alignas(64) RoiRec {  // 64 B
    const uint8_t* plane[3];
    int32_t pitch[3];
    uint16_t width, height;   // source frame (<= 32768, validated)
    int32_t x, y, w, h;       // the caller's rect
    int32_t item;
    uint16_t row0, row1;      // output rows [row0, row1) of this tile (DH <= 65535 for split tiles)
};
static_assert(sizeof(RoiRec) == 64, "RoiRec layout");
// The host builds a record as four 16-byte lines: the frame's first 40 bytes (planes, pitches, size; prepared once per
// source and call), the caller's rect (evam_roi x, y, w, h: 16 contiguous bytes), then the output index and rows.
static_assert(offsetof(RoiRec, x) == 40 && offsetof(RoiRec, item) == 56 && offsetof(RoiRec, row0) == 60, "RoiRec lines");
static_assert(offsetof(evam_roi, h) == offsetof(evam_roi, x) + 12, "evam_roi rect");

constexpr int kMaxStrips = 32;  // per-strip footprints in the kernel arguments: DW <= 2048
constexpr int kSfoot = 64;      // footprint entries: strip kernel tile column x 8 + wave (<= 8 columns)
// One staged row segment of the strip kernel: a strip's footprint is at most one DMA instruction's 64
// 16-byte chunks, so every LDS offset of the ring is a compile-time immediate. 64-column 4:2:0 strips (PX = 1)
// use half-size slots (footprints <= 512 B, downscales <= ~7.7x): half the LDS per wave; BGRx rows are four
// bytes a pixel and always take whole 1 KB slots.
constexpr int strip_slot(int fmt, int px) { return px == 1 && fmt != kBGRX ? 512 : 1024; }

struct TParams {
    ItemArg items[kArgItems];
    double scale_x, scale_y;     // OpenCV: 1. / ((double)rw / cw), 1. / ((double)rh / ch)
    const float* lut;            // [3][256]
    void* dst;
    int slot_offset, slot_stride;  // output slot of item i = slot_offset + i * slot_stride
    int DW, DH;
    int cw, ch, rw, rh, ox, oy;  // the launch's crop size, resized size and placement (uniform)
    int nw;                      // waves (strips) per workgroup
    int TH, tiles_x, tiles_per_item;  // tile = nw strips x TH rows
    int wave_bytes;              // one wave's ring: D entries of strip_slot(PX)-byte segments
    int color_rgb;
    uint32_t fill;
    ColSpan sfoot[kSfoot];       // per strip: crop-relative source columns of the first visible column's
                                 // first tap and the last visible column's last tap; (-1, -1): padding only
                                 // (band kernel: per strip; strip kernel: per tile column x 8 + wave)
    // band kernel only: one wave per (item, band of TH rows, strip); LDS rows of one band
    int nstrips, units;          // strips per row; waves of work in the launch
    int segY, segC;              // bytes of one staged luma / chroma row (multiples of 16)
    int nrY;                     // most luma rows of one band (the chroma rows follow at nrY * segY)
    int prio;                    // 1: progress-based wave priority (s_setprio 3 -> 0 over the quarters of a wave's rows)
    int ahead;                   // band kernel: source rows issued ahead of the rows the current output row reads
};
static_assert(sizeof(TParams) <= 4000, "strip / band kernel arguments must fit the 4 KB kernarg segment");

#ifndef EVAM_PP_ROI_K
#define EVAM_PP_ROI_K 6
#endif
constexpr int kRoiK = EVAM_PP_ROI_K;  // max pixels per lane per row group in the ROI kernel

struct QParams {
    const RoiRec* recs;       // this launch's ROI tiles in launch order (largest work first)
    const float* lut;         // [3][256]
    void* dst;
    int DW, DH;
    int TH;                   // most output rows of one tile (the LDS row table's size)
    int mode, placement;      // evam_resize_mode, evam_placement
    int slot_offset, slot_stride;
    int offXT, offYT, offBuf; // LDS carve: [LUT][XTab x DW][YTab x TH][buf0][buf1]
    int buf_bytes;            // one staging buffer
    int color_rgb;
    uint32_t fill;
    int prio;                 // progress-based priority (as the strip kernel's), over the quarters of the row groups
    uint32_t mqw;             // q / QW as mulhi(q, mqw) for the lane quads (QW = DW / PX > 1): ceil(2^32 / QW)
};

// Staged-kernel pipeline shapes: (output rows per group R, staging buffers NBUF). One variant per
// (format, dtype, column segments) is instantiated for each shape listed here.
struct StagedShape { int R, nbuf; };
// (Three staging buffers, 512-column tiles and 2 KB row slots measured neutral or slower for two rounds and were
// retired in round 5.)
constexpr StagedShape kStagedShapes[] = {{2, 2}, {1, 2}};

// Valid (column segments, rows per group): four waves split NSEGX x R evenly.
constexpr bool staged_valid(int nsegx, int R) { return nsegx > 4 ? R == 1 : (nsegx == 4 ? true : R % (4 / nsegx) == 0); }

constexpr bool staged_shape(int R, int nbuf) {
    for (const StagedShape& ss : kStagedShapes)
        if (ss.R == R && ss.nbuf == nbuf) return true;
    return false;
}

// Ring depth: D = 2 (D 1 / 3 / 4 measured slower on C2 and C5, rounds 2-3: profiles/r03f_bench_lines.txt, C2 D 3
// +2.7 us; the other depths were retired in round 5).
#ifndef EVAM_PP_STRIP_DEPTH
#define EVAM_PP_STRIP_DEPTH 2  // A/B builds only (tools/build_variant.sh -DEVAM_PP_STRIP_DEPTH=3)
#endif
constexpr int kStripD = EVAM_PP_STRIP_DEPTH;

}  // namespace

#endif  // EVAM_PARAMS_H
