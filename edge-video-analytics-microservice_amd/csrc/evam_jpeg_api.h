// evam_pp_jpeg_header / evam_pp_jpeg_bound / evam_pp_encode_jpeg: the host side of the JPEG encoder.
// Included at the end of evam_pp.hip (needs run_impl and struct evam_pp); kernels in evam_jpeg_kernels.h.
#pragma once

namespace {

bool jpeg_geom(int width, int height, JpegGeom& g) {
    if (width <= 0 || height <= 0 || width > 32768 || height > 32768) return false;
    g.W = width; g.H = height;
    g.mx = (width + 15) / 16; g.my = (height + 15) / 16;
    g.n_mcu = g.mx * g.my;
    g.n_blk = g.n_mcu * 6;
    g.n_grp = (g.n_blk + kJpegGroup - 1) / kJpegGroup;
    g.yb_x = (width + 7) / 8; g.yb_y = (height + 7) / 8;
    g.cq_y = (height + 1) / 2;
    return true;
}

int jpeg_reserve(evam_pp* h, int which, size_t need) {
    JpegScratch& s = h->jpeg;
    if (need <= s.cap[which]) return EVAM_PP_OK;
    if (s.buf[which]) {  // hipFree waits for the kernels that may still read it
        (void)hipFree(s.buf[which]);
        s.buf[which] = nullptr;
        s.cap[which] = 0;
        if (which == kJsTab) s.key[2] = -1;
    }
    void* p = nullptr;
    if (hipMalloc(&p, need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(EVAM_PP_ERR_OOM, "evam_pp_encode_jpeg: cannot allocate %zu bytes of device scratch", need);
    }
    s.buf[which] = p;
    s.cap[which] = need;
    return EVAM_PP_OK;
}

int encode_jpeg_impl(evam_pp* h, const evam_image* srcs, int n_srcs, int quality, void* dst, size_t dst_stride,
                     uint32_t* sizes) {
    if (!h || !srcs || !dst || !sizes) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: NULL argument");
    if (n_srcs <= 0 || n_srcs > 65535)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: n_srcs %d outside 1..65535", n_srcs);
    if (quality < 0 || quality > 100)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: quality %d outside 0..100", quality);
    if (dst_stride < (size_t)kJpegHeaderLen + 2)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: dst_stride %zu is smaller than the header and EOI (%d)",
                    dst_stride, kJpegHeaderLen + 2);
    for (int i = 1; i < n_srcs; i++)
        if (srcs[i].width != srcs[0].width || srcs[i].height != srcs[0].height)
            return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: frames of one call must share a size, got %dx%d "
                        "and srcs[%d] %dx%d", srcs[0].width, srcs[0].height, i, srcs[i].width, srcs[i].height);
    JpegGeom g;
    if (!jpeg_geom(srcs[0].width, srcs[0].height, g))
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: srcs[0] bad size %dx%d", srcs[0].width, srcs[0].height);
    // the scan's bit offsets are 32-bit
    if ((uint64_t)g.n_blk * kJpegBlockBits >= ((uint64_t)1 << 32))
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_encode_jpeg: frame %dx%d is too large", g.W, g.H);
    HIP_TRY(hipSetDevice(h->device));

    // ---- the published BGR frame: the identity export of evam_pp_run into scratch (it validates the sources) ----
    const size_t n = (size_t)n_srcs;
    if (int rc = jpeg_reserve(h, kJsBgr, n * g.H * g.W * 3)) return rc;
    evam_preproc cfg{};
    cfg.resize_mode = EVAM_RESIZE_NO_ASPECT;
    cfg.color_order = EVAM_COLOR_BGR;
    cfg.out_dtype = EVAM_DTYPE_U8;
    evam_tensor t{};
    t.data = h->jpeg.buf[kJsBgr];
    t.n = n_srcs; t.c = 3; t.h = g.H; t.w = g.W;
    t.slot_stride = 1;
    t.layout = EVAM_LAYOUT_NHWC;
    if (int rc = run_impl(h, srcs, n_srcs, nullptr, n_srcs, &cfg, &t, nullptr, nullptr)) return rc;

    // ---- scratch and tables ----
    const size_t stream_words = (((size_t)g.n_blk * kJpegBlockBits / 32 + 1) + 3 + 4) & ~(size_t)3;
    if (int rc = jpeg_reserve(h, kJsTab, sizeof(JpegTables))) return rc;
    if (int rc = jpeg_reserve(h, kJsCoef, n * g.n_blk * 64 * sizeof(int16_t))) return rc;
    if (int rc = jpeg_reserve(h, kJsMeta, n * g.n_blk * sizeof(uint32_t))) return rc;
    if (int rc = jpeg_reserve(h, kJsOff, n * g.n_blk * sizeof(uint32_t))) return rc;
    if (int rc = jpeg_reserve(h, kJsGsum, n * g.n_grp * sizeof(uint32_t))) return rc;
    if (int rc = jpeg_reserve(h, kJsTotal, n * sizeof(uint32_t))) return rc;
    if (int rc = jpeg_reserve(h, kJsStream, n * stream_words * sizeof(uint32_t))) return rc;
    JpegScratch& s = h->jpeg;
    if (s.key[0] != g.W || s.key[1] != g.H || s.key[2] != quality) {
        // stream-ordered behind the kernels of earlier calls that read the old tables; the source is pageable, so
        // the runtime has staged it when the call returns
        JpegTables tab;
        jpeg_build_tables(g.W, g.H, quality, tab);
        s.key[2] = -1;
        HIP_TRY(hipMemcpyAsync(s.buf[kJsTab], &tab, sizeof(tab), hipMemcpyHostToDevice, h->stream));
        s.key[0] = g.W; s.key[1] = g.H; s.key[2] = quality;
    }

    JpegParams p{};
    p.g = g;
    p.bgr = (const uint8_t*)s.buf[kJsBgr];
    p.tab = (const JpegTables*)s.buf[kJsTab];
    p.coef = (int16_t*)s.buf[kJsCoef];
    p.meta = (uint32_t*)s.buf[kJsMeta];
    p.off = (uint32_t*)s.buf[kJsOff];
    p.gsum = (uint32_t*)s.buf[kJsGsum];
    p.total = (uint32_t*)s.buf[kJsTotal];
    p.stream = (uint32_t*)s.buf[kJsStream];
    p.stream_words = (uint32_t)stream_words;
    p.dst = (uint8_t*)dst;
    p.dst_stride = dst_stride;
    p.sizes = sizes;
    hipLaunchKernelGGL(evam_jpeg_coef, dim3((g.n_mcu + 3) / 4, n_srcs), dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jpeg_scan1, dim3(g.n_grp, n_srcs), dim3(kJpegGroup), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jpeg_scan2, dim3(n_srcs), dim3(256), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jpeg_pack, dim3(g.n_grp, n_srcs), dim3(kJpegGroup), 0, h->stream, p);
    hipLaunchKernelGGL(evam_jpeg_finish, dim3(n_srcs), dim3(kJpegFinishThreads), 0, h->stream, p);
    HIP_TRY(hipGetLastError());
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev1, h->stream));  // the export's ev0 .. the last JPEG kernel
    h->stats.n_launches += 5;
    h->stats.kernels |= EVAM_KERNEL_JPEG;
    return EVAM_PP_OK;
}

}  // namespace

extern "C" {

int evam_pp_jpeg_header(int width, int height, int quality, uint8_t* out, size_t cap, size_t* len) {
    JpegGeom g;
    if (!len) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_jpeg_header: len is NULL");
    *len = kJpegHeaderLen;
    if (!jpeg_geom(width, height, g))
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_jpeg_header: bad frame size %dx%d", width, height);
    if (quality < 0 || quality > 100)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_jpeg_header: quality %d outside 0..100", quality);
    if (!out || cap < (size_t)kJpegHeaderLen)
        return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_jpeg_header: out holds %zu bytes, the header needs %d", out ? cap : 0,
                    kJpegHeaderLen);
    JpegTables* t = new (std::nothrow) JpegTables;
    if (!t) return fail(EVAM_PP_ERR_OOM, "evam_pp_jpeg_header: out of host memory");
    jpeg_build_tables(width, height, quality, *t);
    memcpy(out, t->header, kJpegHeaderLen);
    delete t;
    return EVAM_PP_OK;
}

size_t evam_pp_jpeg_bound(int width, int height) {
    JpegGeom g;
    if (!jpeg_geom(width, height, g)) return 0;
    // per block kJpegBlockBits bits, doubled for byte stuffing: 415 bytes
    return (size_t)kJpegHeaderLen + 2 + (size_t)g.n_blk * (2 * kJpegBlockBits / 8);
}

int evam_pp_encode_jpeg(evam_pp* h, const evam_image* srcs, int n_srcs, int quality, void* dst, size_t dst_stride,
                        uint32_t* sizes) {
    try {
        return encode_jpeg_impl(h, srcs, n_srcs, quality, dst, dst_stride, sizes);
    } catch (const std::bad_alloc&) {
        return fail(EVAM_PP_ERR_OOM, "evam_pp_encode_jpeg: out of host memory");
    } catch (...) {
        return fail(EVAM_PP_ERR_HIP, "evam_pp_encode_jpeg: unexpected exception");
    }
}

}  // extern "C"
