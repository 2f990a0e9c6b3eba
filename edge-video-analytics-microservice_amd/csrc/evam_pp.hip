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
// One translation unit. This file is the host path: the kernel tables, launch_kernel and resident_per_cu (HipKernels,
// the planner's HIP backend), HipRings, struct evam_pp, run_impl and the evam_pp_run entry points. It holds no kernel
// and no device helper. Included:
//  * evam_params.h (kernel-argument structs) and evam_plan.h (the host planner), both HIP-free;
//  * evam_kernel_common.h (device helpers that two or more families share), then the seven pre-processing families,
//    one header each with the helpers only that family uses, in definition order:
//    evam_{generic,rows,staged,wave,strip,band,roi}_kernels.h;
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
#include "evam_generic_kernels.h"
#include "evam_rows_kernels.h"
#include "evam_staged_kernels.h"
#include "evam_wave_kernels.h"
#include "evam_strip_kernels.h"
#include "evam_band_kernels.h"
#include "evam_roi_kernels.h"
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
