// evam_pp_jpeg_info / evam_pp_decode_jpeg / evam_pp_decode_jpeg_planes and their _host twins: the host side of the
// JPEG decoder.
// Included at the end of evam_pp.hip (needs struct evam_pp); kernels in evam_jpeg_dec_kernels.h, arithmetic in
// evam_jpeg_dec.h.
#pragma once

namespace {

int jdec_reserve(const char* who, evam_pp* h, int which, size_t need) {
    JdecScratch& s = h->jdec;
    if (need <= s.cap[which]) return EVAM_PP_OK;
    if (s.buf[which]) {  // hipFree waits for the kernels that may still use it
        (void)hipFree(s.buf[which]);
        s.buf[which] = nullptr;
        s.cap[which] = 0;
    }
    void* p = nullptr;
    if (hipMalloc(&p, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(EVAM_PP_ERR_OOM, "%s: cannot allocate %zu bytes of device scratch", who, need);
    }
    s.buf[which] = p;
    s.cap[which] = need;
    return EVAM_PP_OK;
}

enum JdecOutKind { kJdOutPacked = 0, kJdOutPlanes };  // BGR / BGRX pixels, or raw NV12 / I420 planes

// What the planes entry points ask of out[i] (fourcc NV12 or I420, every used plane on its own).
int jdec_validate_planes_out(const char* who, const evam_image* out, int n, const JdecGeom& g) {
    for (int i = 0; i < n; i++) {
        const evam_image& o = out[i];
        if (o.fourcc != EVAM_FOURCC_NV12 && o.fourcc != EVAM_FOURCC_I420)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] fourcc 0x%08X: NV12 or I420 planes are written", who, i,
                        o.fourcc);
        if (o.fourcc != out[0].fourcc)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] and out[0] differ in fourcc", who, i);
        if (o.width != g.W || o.height != g.H)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] is %dx%d, the files are %dx%d", who, i, o.width, o.height,
                        g.W, g.H);
        const int np = o.fourcc == EVAM_FOURCC_NV12 ? 2 : 3;
        for (int p = 0; p < np; p++) {
            const int row = p == 0 || np == 2 ? g.W : g.W / 2, rows = p == 0 ? g.H : g.H / 2;
            if (!o.planes[p]) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] has a NULL plane %d", who, i, p);
            if (((uintptr_t)o.planes[p] & 15) || (o.pitch[p] & 15) || o.pitch[p] < row)
                return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] plane %d at %p pitch %d: both must be multiples of 16 "
                            "and the pitch at least %d", who, i, p, (const void*)o.planes[p], o.pitch[p], row);
            if ((int64_t)o.pitch[p] * rows >= ((int64_t)1 << 31))
                return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] plane %d spans 2 GiB or more", who, i, p);
        }
    }
    return EVAM_PP_OK;
}

// Everything the entry points check before any work: the arguments, every file's header, one geometry, the outputs.
int jdec_validate(const char* who, JdecOutKind kind, const uint8_t* const* files, const size_t* lens, int n,
                  const evam_image* out, const int32_t* status, std::vector<JdecFile>& parsed, JdecGeom& g) {
    if (!files || !lens || !out || !status) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (n <= 0 || n > 65535) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: n %d outside 1..65535", who, n);
    parsed.resize((size_t)n);
    evam_jpeg_info first{};
    char msg[320];
    for (int i = 0; i < n; i++) {
        if (!files[i]) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: files[%d] is NULL", who, i);
        evam_jpeg_info info{};
        if (int rc = jdec_parse(files[i], lens[i], &info, &parsed[(size_t)i], msg, sizeof(msg)))
            return fail(rc, "%s: files[%d]: %s", who, i, msg);
        if (kind == kJdOutPlanes && !jdec_planes_ok(info)) {
            if (info.components != 3 || info.h_samp != 2 || info.v_samp != 2)
                return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: files[%d]: %d components, luma sampling %dx%d: raw planes are "
                            "written for 4:2:0 files only (such a file decodes to BGR / BGRX)", who, i, info.components,
                            info.h_samp, info.v_samp);
            return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: files[%d]: odd size %dx%d: raw planes are written for even sizes "
                        "only (such a file decodes to BGR / BGRX)", who, i, info.width, info.height);
        }
        if (i == 0) first = info;
        else if (info.width != first.width || info.height != first.height || info.components != first.components ||
                 info.h_samp != first.h_samp || info.v_samp != first.v_samp ||
                 info.restart_interval != first.restart_interval)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: the files of one call must share a geometry: files[0] is %dx%d, "
                        "%d components, sampling %dx%d, restart %d and files[%d] %dx%d, %d, %dx%d, %d", who, first.width,
                        first.height, first.components, first.h_samp, first.v_samp, first.restart_interval, i,
                        info.width, info.height, info.components, info.h_samp, info.v_samp, info.restart_interval);
    }
    if (!jdec_geom(first, g)) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: bad size %dx%d", who, first.width, first.height);
    if (kind == kJdOutPlanes) return jdec_validate_planes_out(who, out, n, g);
    for (int i = 0; i < n; i++) {
        const evam_image& o = out[i];
        if (o.fourcc != EVAM_FOURCC_BGR && o.fourcc != EVAM_FOURCC_BGRX)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] fourcc 0x%08X: BGR or BGRX is written", who, i, o.fourcc);
        const int bpp = o.fourcc == EVAM_FOURCC_BGR ? 3 : 4;
        if (o.width != g.W || o.height != g.H)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] is %dx%d, the files are %dx%d", who, i, o.width, o.height,
                        g.W, g.H);
        if (!o.planes[0]) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] has a NULL plane", who, i);
        if (((uintptr_t)o.planes[0] & 15) || (o.pitch[0] & 15) || o.pitch[0] < g.W * bpp)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] plane %p pitch %d: both must be multiples of 16 and the "
                        "pitch at least %d", who, i, (const void*)o.planes[0], o.pitch[0], g.W * bpp);
        if ((int64_t)o.pitch[0] * g.H >= ((int64_t)1 << 31))
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] spans 2 GiB or more", who, i);
    }
    return EVAM_PP_OK;
}

int decode_jpeg_impl(const char* who, JdecOutKind kind, evam_pp* h, const uint8_t* const* files, const size_t* lens,
                     int n, const evam_image* out, int32_t* status) {
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL argument", who);
    JdecGeom g;
    std::vector<JdecFile>& parsed = h->jdec.parsed;
    if (int rc = jdec_validate(who, kind, files, lens, n, out, status, parsed, g)) return rc;
    const bool planes = kind == kJdOutPlanes;
    for (int i = 1; i < n && !planes; i++)
        if (out[i].fourcc != out[0].fourcc)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out[%d] and out[0] differ in fourcc", who, i);
    HIP_TRY(hipSetDevice(h->device));

    // ---- layout of the upload: JdecFile[n], JdecOut[n] or JdecPlanesOut[n], then every file's entropy-coded bytes ----
    static_assert(sizeof(JdecFile) % 16 == 0 && sizeof(JdecOut) % 16 == 0 && sizeof(JdecPlanesOut) % 16 == 0,
                  "the entropy-coded bytes start at a multiple of 16");
    const size_t nf = (size_t)n;
    size_t up = nf * sizeof(JdecFile) + nf * (planes ? sizeof(JdecPlanesOut) : sizeof(JdecOut));
    const size_t raw0 = up;
    uint32_t max_scan = 0;
    for (size_t i = 0; i < nf; i++) {
        parsed[i].raw_off = (uint32_t)(up - raw0);
        up += ((size_t)parsed[i].scan_len + 15) & ~(size_t)15;
        max_scan = std::max(max_scan, parsed[i].scan_len);
        if (up - raw0 >= ((size_t)1 << 32))
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: the files of one call hold 4 GiB or more", who);
    }
    up += 16;
    const size_t stream_stride = (((size_t)max_scan + 15) & ~(size_t)15) + 2 * kJdecStreamPad;
    const size_t n_slots = (size_t)max_scan / kJdecSubBytes + (size_t)g.n_int + 1;

    JdecScratch& s = h->jdec;
    if (s.pin_busy) {  // the previous call's copy may still read the staging
        HIP_TRY(hipEventSynchronize(s.pin_ev));
        s.pin_busy = false;
    }
    if (!s.pin_ev) HIP_TRY(hipEventCreateWithFlags(&s.pin_ev, hipEventDisableTiming));
    if (up > s.pin_cap) {
        if (s.pin) (void)hipHostFree(s.pin);
        s.pin = nullptr; s.pin_cap = 0;
        void* p = nullptr;
        if (hipHostMalloc(&p, up, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(EVAM_PP_ERR_OOM, "%s: cannot allocate %zu bytes of pinned staging", who, up);
        }
        s.pin = (uint8_t*)p; s.pin_cap = up;
    }
    if (int rc = jdec_reserve(who, h, kJdUp, up)) return rc;
    if (int rc = jdec_reserve(who, h, kJdStream, nf * stream_stride)) return rc;
    if (int rc = jdec_reserve(who, h, kJdFirst, nf * ((size_t)g.n_int + 1) * sizeof(uint32_t))) return rc;
    if (int rc = jdec_reserve(who, h, kJdSlots, nf * n_slots * sizeof(uint4))) return rc;
    if (int rc = jdec_reserve(who, h, kJdCoef, nf * (size_t)g.n_blk * 64 * sizeof(int16_t))) return rc;
    if (!planes)  // the planes path writes the caller's planes: no component planes in scratch
        if (int rc = jdec_reserve(who, h, kJdPlanes, nf * (size_t)g.plane_bytes)) return rc;

    memcpy(s.pin, parsed.data(), nf * sizeof(JdecFile));
    JdecOut* outs = reinterpret_cast<JdecOut*>(s.pin + nf * sizeof(JdecFile));
    JdecPlanesOut* pouts = reinterpret_cast<JdecPlanesOut*>(s.pin + nf * sizeof(JdecFile));
    for (size_t i = 0; i < nf; i++) {
        if (planes) {
            pouts[i] = JdecPlanesOut{};
            for (int p = 0; p < (out[i].fourcc == EVAM_FOURCC_NV12 ? 2 : 3); p++) {
                pouts[i].p[p] = const_cast<uint8_t*>(out[i].planes[p]);
                pouts[i].pitch[p] = out[i].pitch[p];
            }
        } else {
            outs[i].p = const_cast<uint8_t*>(out[i].planes[0]);
            outs[i].pitch = out[i].pitch[0];
            outs[i].pad = 0;
        }
        memcpy(s.pin + raw0 + parsed[i].raw_off, files[i] + (lens[i] - parsed[i].scan_len), parsed[i].scan_len);
    }
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev0, h->stream));
    HIP_TRY(hipMemcpyAsync(s.buf[kJdUp], s.pin, up, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(s.pin_ev, h->stream));
    s.pin_busy = true;
    HIP_TRY(hipMemsetAsync(status, 0, nf * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(s.buf[kJdSlots], 0, nf * n_slots * sizeof(uint4), h->stream));
    HIP_TRY(hipMemsetAsync(s.buf[kJdCoef], 0, nf * (size_t)g.n_blk * 64 * sizeof(int16_t), h->stream));

    JdecParams p{};
    p.g = g;
    p.files = (const JdecFile*)s.buf[kJdUp];
    p.outs = (const JdecOut*)((const uint8_t*)s.buf[kJdUp] + nf * sizeof(JdecFile));
    p.pouts = (const JdecPlanesOut*)((const uint8_t*)s.buf[kJdUp] + nf * sizeof(JdecFile));
    p.raw = (const uint8_t*)s.buf[kJdUp] + raw0;
    p.stream = (uint8_t*)s.buf[kJdStream];
    p.stream_stride = (uint32_t)stream_stride;
    p.first = (uint32_t*)s.buf[kJdFirst];
    p.slots = (uint4*)s.buf[kJdSlots];
    p.n_slots = (uint32_t)n_slots;
    p.coef = (int16_t*)s.buf[kJdCoef];
    p.planes = planes ? nullptr : (uint8_t*)s.buf[kJdPlanes];
    p.status = status;
    hipLaunchKernelGGL(evam_jdec_unstuff, dim3(n), dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jdec_sync, dim3(g.n_int, n), dim3(kJdecChunk), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jdec_write, dim3((unsigned)((n_slots + 255) / 256), n), dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jdec_dc, dim3(g.n_int, n), dim3(kJdecDcThreads), 0, h->stream, p);
    if (planes) {
        const dim3 pgrid((g.n_mcu + kJdecPlaneMcus - 1) / kJdecPlaneMcus, n);
        if (out[0].fourcc == EVAM_FOURCC_NV12)
            hipLaunchKernelGGL(evam_jdec_idct_planes<true>, pgrid, dim3(256), 0, h->stream, p);
        else
            hipLaunchKernelGGL(evam_jdec_idct_planes<false>, pgrid, dim3(256), 0, h->stream, p);
    } else {
        hipLaunchKernelGGL(evam_jdec_idct, dim3((g.n_blk + 31) / 32, n), dim3(256), 0, h->stream, p);
        constexpr int kVec = 4;
        const dim3 cgrid((g.W + 256 * kVec - 1) / (256 * kVec), g.H, n);
        if (out[0].fourcc == EVAM_FOURCC_BGR)
            hipLaunchKernelGGL((evam_jdec_colour<3, kVec>), cgrid, dim3(256), 0, h->stream, p);
        else
            hipLaunchKernelGGL((evam_jdec_colour<4, kVec>), cgrid, dim3(256), 0, h->stream, p);
    }
    HIP_TRY(hipGetLastError());
    if (h->opt_timing) {
        HIP_TRY(hipEventRecord(h->ev1, h->stream));
        h->timed = true;
    }
    h->stats = evam_pp_stats{};
    h->stats.n_items = n;
    h->stats.n_launches = planes ? 5 : 6;
    h->stats.kernels = EVAM_KERNEL_JPEG_DEC;
    return EVAM_PP_OK;
}

int decode_jpeg_host_impl(const char* who, JdecOutKind kind, const uint8_t* const* files, const size_t* lens, int n,
                          const evam_image* out, int32_t* status) {
    JdecGeom g;
    std::vector<JdecFile> parsed;
    if (int rc = jdec_validate(who, kind, files, lens, n, out, status, parsed, g)) return rc;
    std::vector<int16_t> coef((size_t)g.n_blk * 64);
    std::vector<uint8_t> planes(kind == kJdOutPlanes ? 0 : g.plane_bytes), stream;
    std::vector<uint32_t> first((size_t)g.n_int + 1);
    for (int i = 0; i < n; i++) {
        const JdecFile& f = parsed[(size_t)i];
        std::fill(coef.begin(), coef.end(), (int16_t)0);
        stream.assign((size_t)f.scan_len + kJdecStreamPad, 0);
        int err = jdec_unstuff_host(files[i] + (lens[i] - f.scan_len), f.scan_len, g.n_int, stream.data(), first.data());
        JdecScan sc{stream.data(), &f, g.nluma, g.bpm};
        for (int k = 0; k < g.n_int; k++) {
            const uint32_t m0 = g.ri > 0 ? (uint32_t)k * g.ri : 0u;
            const uint32_t m1 = g.ri > 0 ? std::min<uint32_t>(m0 + g.ri, g.n_mcu) : (uint32_t)g.n_mcu;
            uint32_t p = first[k] * 8, bz = 0;
            const uint32_t end = first[k + 1] * 8, blk0 = m0 * g.bpm, limit = m1 * g.bpm;
            const uint32_t done = jdec_run(sc, p, bz, end, end, coef.data(), blk0, limit, err);
            if (blk0 + done < limit) err = 1;
        }
        if (kind == kJdOutPlanes) {
            JdecPlanesOut o{};
            for (int p = 0; p < (out[i].fourcc == EVAM_FOURCC_NV12 ? 2 : 3); p++) {
                o.p[p] = const_cast<uint8_t*>(out[i].planes[p]);
                o.pitch[p] = out[i].pitch[p];
            }
            if (out[i].fourcc == EVAM_FOURCC_NV12) jdec_planes_host<true>(g, f, coef.data(), o, err);
            else jdec_planes_host<false>(g, f, coef.data(), o, err);
        } else {
            jdec_dc_and_idct_host(g, f, coef.data(), planes.data(), err);
            jdec_colour_host(g, planes.data(), const_cast<uint8_t*>(out[i].planes[0]), out[i].pitch[0],
                             out[i].fourcc == EVAM_FOURCC_BGR ? 3 : 4);
        }
        status[i] = err ? EVAM_PP_ERR_INVALID_ARG : 0;
    }
    return EVAM_PP_OK;
}

}  // namespace

extern "C" {

int evam_pp_jpeg_info(const uint8_t* file, size_t len, evam_jpeg_info* out) {
    char msg[320];
    if (!file || !out) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_jpeg_info: NULL argument");
    evam_jpeg_info info{};
    try {  // the parse allocates its table scratch
        if (int rc = jdec_parse(file, len, &info, nullptr, msg, sizeof(msg)))
            return fail(rc, "evam_pp_jpeg_info: %s", msg);
    } catch (const std::bad_alloc&) {
        return fail(EVAM_PP_ERR_OOM, "evam_pp_jpeg_info: out of host memory");
    } catch (...) {
        return fail(EVAM_PP_ERR_HIP, "evam_pp_jpeg_info: unexpected exception");
    }
    *out = info;
    return EVAM_PP_OK;
}

int evam_pp_decode_jpeg(evam_pp* h, const uint8_t* const* files, const size_t* lens, int n, const evam_image* out,
                        int32_t* status) {
    try {
        return decode_jpeg_impl("evam_pp_decode_jpeg", kJdOutPacked, h, files, lens, n, out, status);
    } catch (const std::bad_alloc&) {
        return fail(EVAM_PP_ERR_OOM, "evam_pp_decode_jpeg: out of host memory");
    } catch (...) {
        return fail(EVAM_PP_ERR_HIP, "evam_pp_decode_jpeg: unexpected exception");
    }
}

int evam_pp_decode_jpeg_host(const uint8_t* const* files, const size_t* lens, int n, const evam_image* out,
                             int32_t* status) {
    try {
        return decode_jpeg_host_impl("evam_pp_decode_jpeg_host", kJdOutPacked, files, lens, n, out, status);
    } catch (const std::bad_alloc&) {
        return fail(EVAM_PP_ERR_OOM, "evam_pp_decode_jpeg_host: out of host memory");
    } catch (...) {
        return fail(EVAM_PP_ERR_HIP, "evam_pp_decode_jpeg_host: unexpected exception");
    }
}

int evam_pp_decode_jpeg_planes(evam_pp* h, const uint8_t* const* files, const size_t* lens, int n,
                               const evam_image* out, int32_t* status) {
    try {
        return decode_jpeg_impl("evam_pp_decode_jpeg_planes", kJdOutPlanes, h, files, lens, n, out, status);
    } catch (const std::bad_alloc&) {
        return fail(EVAM_PP_ERR_OOM, "evam_pp_decode_jpeg_planes: out of host memory");
    } catch (...) {
        return fail(EVAM_PP_ERR_HIP, "evam_pp_decode_jpeg_planes: unexpected exception");
    }
}

int evam_pp_decode_jpeg_planes_host(const uint8_t* const* files, const size_t* lens, int n, const evam_image* out,
                                    int32_t* status) {
    try {
        return decode_jpeg_host_impl("evam_pp_decode_jpeg_planes_host", kJdOutPlanes, files, lens, n, out, status);
    } catch (const std::bad_alloc&) {
        return fail(EVAM_PP_ERR_OOM, "evam_pp_decode_jpeg_planes_host: out of host memory");
    } catch (...) {
        return fail(EVAM_PP_ERR_HIP, "evam_pp_decode_jpeg_planes_host: unexpected exception");
    }
}

}  // extern "C"
