// Device helpers that two or more kernel families use: the diagnostic and cache-policy macros, the exact OpenCV
// arithmetic, the saturating BT.601 form, the store helpers, LaneRows, lds_barrier, ProgressPrio and the trace macros.
// Included by evam_pp.hip before the kernel families' headers (evam_{generic,rows,staged,wave,strip,band,roi}_kernels.h);
// reopens its anonymous namespace (evam:: names).
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// constants
// ------------------------------------------------------------------------------------------------
// Stage-removal diagnostics (bits: 2 no pixel math, 4 no stores, 8 loads only, 16 no loads, 32/64/128 stop
// early). Compile-time only: a product build is 0, every diagnostic branch folds away, and no environment
// setting can change results. A build with -DEVAM_PP_ABLATE=bits computes INVALID tensors; evam_pp_create
// refuses it unless EVAM_PP_DIAGNOSTIC_BUILD_OK=1 (tools/prof_ablate.sh).
#ifndef EVAM_PP_ABLATE
#define EVAM_PP_ABLATE 0
#endif
constexpr int kAblate = EVAM_PP_ABLATE;
// Cache-policy bits of the output stores: 2 = nt (non-temporal). The outputs are written once and
// read by nobody in the launch; streaming them past the caches measured 1.5-3 % faster on C2/C3/C4
// and 10 % on C5 (profiles/r02r_store_policy.txt). EVAM_PP_LOAD_AUX: the same bits for the LDS-DMA
// source reads (A/B builds).
#ifndef EVAM_PP_STORE_AUX
#define EVAM_PP_STORE_AUX 2
#endif
#ifndef EVAM_PP_LOAD_AUX
#define EVAM_PP_LOAD_AUX 0
#endif

// OpenCV color_yuv.simd.hpp ITUR_BT_601_*; the -128 chroma bias is folded into the constants.
constexpr int kCY = 1220542, kCUB = 2116026, kCUG = -409993, kCVG = -852492, kCVR = 1673527;
constexpr int kHalf = 1 << 19;
constexpr int kKR = kHalf - 128 * kCVR - 16 * kCY;  // the luma term is max(Y,16)*CY (see yuv_to_bgr)
constexpr int kKG = kHalf - 128 * kCVG - 128 * kCUG - 16 * kCY;
constexpr int kKB = kHalf - 128 * kCUB - 16 * kCY;

// ------------------------------------------------------------------------------------------------
// exact OpenCV arithmetic (shared host/device)
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// VResizeLinear<uchar,int,short,FixedPtCast<int,uchar,22>,VResizeLinearVec_32s8u>:
//   dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
// evaluated on the full-rate 24-bit multiplier. The column table holds a' = a << 4 and the row table
// b' = b << 8, so the horizontal pass yields D' = D << 4 (< 2^23) and
//   (b * (D >> 4)) >> 16 == mulhi_u24(b', D' & ~0xFF)
// exactly (b' * ((D >> 4) << 8) = b * (D >> 4) * 2^16).
__device__ __forceinline__ uint32_t mulhi_u24(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)) >> 32);
}
__device__ __forceinline__ int vresize(uint32_t D0s, uint32_t D1s, uint32_t b0s, uint32_t b1s) {
    return (int)((mulhi_u24(b0s, D0s & 0xFFFF00u) + mulhi_u24(b1s, D1s & 0xFFFF00u) + 2u) >> 2);
}
// Same, for OUT != 0 returned as 4 * result (the byte offset into a LUT section of 4-byte entries).
template <int OUT>
__device__ __forceinline__ uint32_t vfinal(uint32_t D0s, uint32_t D1s, uint32_t b0s, uint32_t b1s) {
    const uint32_t x = mulhi_u24(b0s, D0s & 0xFFFF00u) + mulhi_u24(b1s, D1s & 0xFFFF00u) + 2u;
    return OUT != 0 ? (x & ~3u) : (x >> 2);
}

template <int FMT>
struct FmtTraits {
    static constexpr int bpp = FMT == kBGRX ? 4 : (FMT == kBGR ? 3 : 1);
    static constexpr int nchroma = FMT == kNV12 ? 1 : (FMT == kI420 ? 2 : 0);
};

// Planar stores of one pixel. Plane bases are wave-uniform (SGPR) and the offset is a 32-bit byte
// offset, so every store is one saddr-form instruction with no 64-bit address arithmetic.
// NHWC (interleaved output): d0 is the slot base and the pixel's three elements are adjacent at 3 * o
// (d1, d2 unused); element stores only, so a slot may start at any element-aligned address.
// OUT == 2: the 16-bit pattern in the low half of table entry i (fp16 / bf16 bits, no conversion on the device).
__device__ __forceinline__ uint16_t lut_u16(const float* __restrict__ lut, int i) {
    return *reinterpret_cast<const uint16_t*>(lut + i);
}
template <int OUT, bool NHWC = false>
__device__ __forceinline__ void store_px(uint8_t* d0, uint8_t* d1, uint8_t* d2, const float* __restrict__ lut,
                                         uint32_t o, int v0, int v1, int v2) {
    if constexpr (NHWC) {
        const uint32_t o3 = o * 3u;
        if constexpr (OUT == 0) {
            d0[o3] = (uint8_t)v0;
            d0[o3 + 1] = (uint8_t)v1;
            d0[o3 + 2] = (uint8_t)v2;
        } else if constexpr (OUT == 2) {
            uint16_t* const q = reinterpret_cast<uint16_t*>(d0 + (o3 << 1));
            q[0] = lut_u16(lut, v0);
            q[1] = lut_u16(lut, 256 + v1);
            q[2] = lut_u16(lut, 512 + v2);
        } else {
            float* const q = reinterpret_cast<float*>(d0 + (o3 << 2));
            q[0] = lut[v0];
            q[1] = lut[256 + v1];
            q[2] = lut[512 + v2];
        }
    } else if constexpr (OUT == 0) {
        d0[o] = (uint8_t)v0;
        d1[o] = (uint8_t)v1;
        d2[o] = (uint8_t)v2;
    } else if constexpr (OUT == 2) {
        const uint32_t ob = o << 1;
        *reinterpret_cast<uint16_t*>(d0 + ob) = lut_u16(lut, v0);
        *reinterpret_cast<uint16_t*>(d1 + ob) = lut_u16(lut, 256 + v1);
        *reinterpret_cast<uint16_t*>(d2 + ob) = lut_u16(lut, 512 + v2);
    } else {
        const uint32_t ob = o << 2;
        *reinterpret_cast<float*>(d0 + ob) = lut[v0];
        *reinterpret_cast<float*>(d1 + ob) = lut[256 + v1];
        *reinterpret_cast<float*>(d2 + ob) = lut[512 + v2];
    }
}

// Saturating form of the BT.601 integers, two taps per register. The chroma terms carry the bias
// 2^32 - 2^28 on top of kK*, so for S = y + term (the BT.601 sum before >> 20) the unsigned
// saturating add y + term' is S + 2^32 - 2^28 when S < 2^28 and 0xFFFFFFFF otherwise; every term'
// lies in [0, 2^32) (no wrap). Its high half is then floor(S / 2^16) + 61440, and one u16
// saturating subtract of 61440 clamps it to [0, 4095], i.e. to 16 * clamp255(S >> 20) plus four
// low bits that a mask drops. Two taps' high halves share one register (v_perm), so the clamp costs
// a packed subtract and a mask per tap pair, and the horizontal pass D = c0*a0 + c1*a1 is one
// v_dot2_u32_u16 that yields 16 * D, the D' vresize takes. tools/check_sat_clamp.py checks the
// clamp against clamp255((y + term) >> 20) over all 2^24 (Y, U, V).
typedef unsigned short evam_u16x2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kSatBias = 0xF0000000u;  // 2^32 - 2^28
constexpr uint32_t kKBs = (uint32_t)kKB + kSatBias, kKGs = (uint32_t)kKG + kSatBias, kKRs = (uint32_t)kKR + kSatBias;
struct UVs { uint32_t b, g, r; };
__device__ __forceinline__ UVs uv_terms_sat(uint32_t U, uint32_t V) {
    // G as two chained v_mad_i32_i24 (the opaque middle value keeps the compiler from re-forming two products and
    // an add3): 4 VALU per chroma sample instead of 5
    int gu = __mul24((int)U, kCUG) + (int)kKGs;
    asm("" : "+v"(gu));
    return UVs{__umul24(U, (uint32_t)kCUB) + kKBs, (uint32_t)(__mul24((int)V, kCVG) + gu), __umul24(V, (uint32_t)kCVR) + kKRs};
}
__device__ __forceinline__ uint32_t luma_term(uint32_t Y) { return __umul24(max(Y, 16u), (uint32_t)kCY); }
// One source row, one channel: taps' sums s0 (column x0) and s1 (column x1), packed weights w = a0 | a1 << 16
// (plain 11-bit) -> 16 * (c0 * a0 + c1 * a1).
// hpass_sums: the same from the taps' saturated sums (pixels whose taps meet at one column share a sum).
__device__ __forceinline__ uint32_t hpass_sums(uint32_t s0, uint32_t s1, uint32_t w) {
    const evam_u16x2 h = __builtin_bit_cast(evam_u16x2, __builtin_amdgcn_perm(s1, s0, 0x07060302u));
    const evam_u16x2 c = __builtin_elementwise_sub_sat(h, (evam_u16x2){61440, 61440});
    const uint32_t c16 = __builtin_bit_cast(uint32_t, c) & 0xFFF0FFF0u;
    return __builtin_amdgcn_udot2(__builtin_bit_cast(evam_u16x2, c16), __builtin_bit_cast(evam_u16x2, w), 0u, false);
}
__device__ __forceinline__ uint32_t hpass_sat(uint32_t y0, uint32_t t0, uint32_t y1, uint32_t t1, uint32_t w) {
    return hpass_sums(__builtin_elementwise_add_sat(y0, t0), __builtin_elementwise_add_sat(y1, t1), w);
}

// Horizontal pass of one source row, three channels, from the two taps' luma bytes and chroma terms.
__device__ __forceinline__ void hrow_sat(uint32_t Y0, uint32_t Y1, const UVs& tA, const UVs& tB, uint32_t w,
                                         uint32_t (&H)[3]) {
    const uint32_t yA = luma_term(Y0), yB = luma_term(Y1);
    H[0] = hpass_sat(yA, tA.b, yB, tB.b, w);
    H[1] = hpass_sat(yA, tA.g, yB, tB.g, w);
    H[2] = hpass_sat(yA, tA.r, yB, tB.r, w);
}

// Row table of up to 64 consecutive output rows held one row per lane (r0, r1, b0, b1 in four VGPRs),
// read back as wave-uniform values with v_readlane: the per-row lookups of the staging loops then cost
// no scalar-memory round trip (a dependent s_load per row serialised the DMA issue).
struct LaneRows {
    int r0, r1, b0, b1;
    __device__ __forceinline__ void load(const YTab* ytab, int Ybase, int n, int lane) {
        const int Y = Ybase + (lane < n ? lane : 0);
        const YTab e = ytab[Y];
        r0 = e.r0; r1 = e.r1; b0 = e.b0; b1 = e.b1;
    }
    __device__ __forceinline__ int R0(int i) const { return __builtin_amdgcn_readlane(r0, i); }
    __device__ __forceinline__ int R1(int i) const { return __builtin_amdgcn_readlane(r1, i); }
    __device__ __forceinline__ int B0(int i) const { return __builtin_amdgcn_readlane(b0, i); }
    __device__ __forceinline__ int B1(int i) const { return __builtin_amdgcn_readlane(b1, i); }
};

// Workgroup barrier for data written to LDS by ds_write only: lgkmcnt(0) and a raw s_barrier. __syncthreads()
// also waits vmcnt(0), which drains every LDS-DMA in flight (cdna_hip_programming.md, Pipelining across barriers).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

typedef int evam_v2i __attribute__((ext_vector_type(2)));
typedef int evam_v3i __attribute__((ext_vector_type(3)));
typedef int evam_v4i __attribute__((ext_vector_type(4)));

// PX adjacent output pixels of one channel from one lane as a single buffer store (as the wave kernel's store_vec),
// with the fp32 values given as byte offsets into an LDS LUT section `lb` (vfinal<1>): the LUT
// read needs no address arithmetic (section base 0, 1024, 2048 is the instruction's immediate offset).
template <int OUT, int PX>
__device__ __forceinline__ void store_off(const __amdgpu_buffer_rsrc_t rs, uint32_t vo, const uint8_t* lb,
                                          const uint32_t (&v)[PX]) {
    if constexpr (OUT == 1) {
        auto L = [&](uint32_t o) { return (int)*reinterpret_cast<const uint32_t*>(lb + o); };
        if constexpr (PX == 4) {
            evam_v4i q = {L(v[0]), L(v[1]), L(v[2]), L(v[3])};
            __builtin_amdgcn_raw_buffer_store_b128(q, rs, vo, 0, EVAM_PP_STORE_AUX);
        } else if constexpr (PX == 2) {
            evam_v2i q = {L(v[0]), L(v[1])};
            __builtin_amdgcn_raw_buffer_store_b64(q, rs, vo, 0, EVAM_PP_STORE_AUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32((uint32_t)L(v[0]), rs, vo, 0, EVAM_PP_STORE_AUX);
        }
    } else if constexpr (OUT == 2) {
        // the low u16 of each 4-byte entry, two per dword (see store_vec)
        auto H = [&](uint32_t o) { return (uint32_t)*reinterpret_cast<const uint16_t*>(lb + o); };
        if constexpr (PX == 4) {
            evam_v2i q = {(int)(H(v[0]) | (H(v[1]) << 16)), (int)(H(v[2]) | (H(v[3]) << 16))};
            __builtin_amdgcn_raw_buffer_store_b64(q, rs, vo, 0, EVAM_PP_STORE_AUX);
        } else if constexpr (PX == 2) {
            __builtin_amdgcn_raw_buffer_store_b32(H(v[0]) | (H(v[1]) << 16), rs, vo, 0, EVAM_PP_STORE_AUX);
        } else {
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)H(v[0]), rs, vo, 0, EVAM_PP_STORE_AUX);
        }
    } else {
        if constexpr (PX == 4)
            __builtin_amdgcn_raw_buffer_store_b32(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24), rs, vo, 0,
                                                  EVAM_PP_STORE_AUX);
        else if constexpr (PX == 2)
            __builtin_amdgcn_raw_buffer_store_b16((uint16_t)(v[0] | (v[1] << 8)), rs, vo, 0, EVAM_PP_STORE_AUX);
        else
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v[0], rs, vo, 0, EVAM_PP_STORE_AUX);
    }
}

// Progress-based priority (EVAM_PP_PRIO): s_setprio 3 at the start, one level lower at each quarter of a wave's n
// steps (rows or row groups), so the waves behind get the issue slot when several are ready. One scalar compare per
// step against the next threshold; the level change sits in the rarely taken branch (the three-way compare chain it
// replaces cost six scalar instructions per step).
struct ProgressPrio {
    int next, q2, q3, level;
    __device__ __forceinline__ ProgressPrio(bool on, int n) : next(on ? n / 4 : -1), q2(n / 2), q3((3 * n) / 4), level(3) {
        if (on) __builtin_amdgcn_s_setprio(3);
    }
    __device__ __forceinline__ void step(int i) {
        if (__builtin_expect(i != next, 1)) return;
        if (level == 3) {
            __builtin_amdgcn_s_setprio(2);
            level = 2;
            next = q2;
        } else if (level == 2) {
            __builtin_amdgcn_s_setprio(1);
            level = 1;
            next = q3;
        } else {
            __builtin_amdgcn_s_setprio(0);
            level = 0;
            next = -1;
        }
    }
};

// Diagnostic builds only (-DEVAM_PP_TRACE): timestamps of the 100 MHz constant clock written by lane 0
// with a vector store, per workgroup (EVAM_STAMP: the ROI kernel, tools/roi_timeline.py) or per wave
// (EVAM_WSTAMP: the strip kernel, tools/wave_timeline.py). Product builds compile no stamp. In the strip
// kernel a stamp is one more VMEM operation than its counted waits assume, which only makes them wait
// longer (still exact data, slightly perturbed timing).
#ifdef EVAM_PP_TRACE
constexpr int kTraceWGs = 16384, kTraceSlots = 12;
__device__ unsigned long long g_evam_trace[kTraceWGs * kTraceSlots];
#define EVAM_STAMP(k)                                                                                  \
    do {                                                                                               \
        unsigned long long t_;                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        if (threadIdx.x == 0 && blockIdx.x < kTraceWGs) g_evam_trace[blockIdx.x * kTraceSlots + (k)] = t_; \
    } while (0)
#define EVAM_TRACE_VAL(k, v)                                                                           \
    do {                                                                                               \
        if (threadIdx.x == 0 && blockIdx.x < kTraceWGs) g_evam_trace[blockIdx.x * kTraceSlots + (k)] = (v); \
    } while (0)
#define EVAM_WSTAMP(k)                                                                                 \
    do {                                                                                               \
        unsigned long long t_;                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        const unsigned w_ = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); \
        if ((threadIdx.x & 63) == 0 && w_ < (unsigned)kTraceWGs) g_evam_trace[w_ * kTraceSlots + (k)] = t_; \
    } while (0)
#define EVAM_WTRACE_VAL(k, v)                                                                          \
    do {                                                                                               \
        const unsigned w_ = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); \
        if ((threadIdx.x & 63) == 0 && w_ < (unsigned)kTraceWGs) g_evam_trace[w_ * kTraceSlots + (k)] = (v); \
    } while (0)
#else
#define EVAM_STAMP(k) do { } while (0)
#define EVAM_TRACE_VAL(k, v) do { } while (0)
#define EVAM_WSTAMP(k) do { } while (0)
#define EVAM_WTRACE_VAL(k, v) do { } while (0)
#endif

}  // namespace
