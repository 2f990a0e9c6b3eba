// Device-resident ROI lists: evam_pp_ssd_rois_host, evam_pp_ssd_rois(_ex), evam_pp_run_device_rois and their argument
// checks; grow_device, which the DetectionOutput entry point uses too. Included at the end of evam_pp.hip, before the other
// evam_*_api.h (needs struct evam_pp, fail, HIP_TRY, run_impl's helpers); kernels in evam_rois_kernels.h.
#pragma once

namespace {

int grow_device(void** p, size_t* cap, size_t n, const char* who) {
    if (*cap >= n) return 0;
    if (*p) {
        HIP_TRY(hipFree(*p));  // waits for the kernels that still use it
        *p = nullptr;
        *cap = 0;
    }
    const size_t c = std::max<size_t>(n * 2, 64 * 1024);
    if (hipMalloc(p, c) != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        return fail(EVAM_PP_ERR_OOM, "%s: hipMalloc(%zu) failed", who, c);
    }
    *cap = c;
    return 0;
}

int check_roi_list(const evam_roi_list* list, const char* who) {
    if (!list || !list->rois || !list->count) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL ROI list pointer", who);
    if (list->cap <= 0) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: list cap %d must be > 0", who, list->cap);
    return 0;
}

int check_ssd_args(const char* who, const float* det, int n_items, int k, const evam_image* srcs, int tensor_w,
                   int tensor_h, const int32_t* labels, int n_labels, const evam_roi_list* list) {
    if (!det || !srcs) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = check_roi_list(list, who)) return rc;
    if (n_items <= 0 || k <= 0 || n_items > 65535 || k > 65535)
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: n_items %d / k %d outside 1..65535", who, n_items, k);
    if (tensor_w <= 0 || tensor_h <= 0) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: bad tensor size %dx%d", who, tensor_w, tensor_h);
    if (n_labels < 0 || (!labels && n_labels > 0)) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: bad label list", who);
    for (int i = 0; i < n_items; i++)
        if (srcs[i].width <= 0 || srcs[i].height <= 0 || srcs[i].width > 32768 || srcs[i].height > 32768)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: srcs[%d] bad size %dx%d", who, i, srcs[i].width, srcs[i].height);
    return 0;
}

}  // namespace

extern "C" {

int evam_pp_ssd_rois_host(const float* det, int n_items, int k, const evam_image* srcs, const evam_transform* xf,
                          int tensor_w, int tensor_h, float threshold, const int32_t* labels, int n_labels,
                          const evam_roi_list* list) {
    if (int rc = check_ssd_args("evam_pp_ssd_rois_host", det, n_items, k, srcs, tensor_w, tensor_h, labels, n_labels, list))
        return rc;
    static const int32_t none = 0;
    const int32_t* lab = labels ? (n_labels ? labels : &none) : nullptr;
    uint32_t total = 0;
    for (int i = 0; i < n_items; i++) {
        const float* d = det + (size_t)i * (size_t)k * 7;
        for (int r = 0; r < k; r++) {
            const float* row = d + (size_t)r * 7;
            if (row[0] < 0.f) break;
            int x, y, w, h;
            if (!ssd_row_rect(row, xf ? xf + i : nullptr, srcs[i].width, srcs[i].height, tensor_w, tensor_h, threshold, lab,
                              n_labels, x, y, w, h))
                continue;
            if (total < (uint32_t)list->cap) list->rois[total] = evam_roi{i, x, y, w, h};
            total++;
        }
    }
    *list->count = total;
    return EVAM_PP_OK;
}

int evam_pp_ssd_rois(evam_pp* h, const float* det, int n_items, int k, const evam_image* srcs, const evam_transform* xf,
                     int tensor_w, int tensor_h, float threshold, const int32_t* labels, int n_labels,
                     const evam_roi_list* list) {
    return evam_pp_ssd_rois_ex(h, det, n_items, k, srcs, xf, tensor_w, tensor_h, threshold, labels, n_labels, list, nullptr);
}

int evam_pp_ssd_rois_ex(evam_pp* h, const float* det, int n_items, int k, const evam_image* srcs, const evam_transform* xf,
                        int tensor_w, int tensor_h, float threshold, const int32_t* labels, int n_labels,
                        const evam_roi_list* list, int32_t* out_labels) {
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "evam_pp_ssd_rois: NULL handle");
    if (int rc = check_ssd_args("evam_pp_ssd_rois", det, n_items, k, srcs, tensor_w, tensor_h, labels, n_labels, list))
        return rc;
    // host block: [int2 x n_items: frame sizes][evam_transform x n_items, with xf][int32 x n_labels] (never empty)
    const size_t off_xf = sizeof(int2) * (size_t)n_items;
    const size_t off_lab = off_xf + (xf ? sizeof(evam_transform) * (size_t)n_items : 0);
    std::vector<uint8_t>& blk = h->h_aux;
    blk.assign(off_lab + sizeof(int32_t) * (size_t)std::max(1, n_labels), 0);
    for (int i = 0; i < n_items; i++) {
        const int32_t wh[2] = {srcs[i].width, srcs[i].height};
        memcpy(blk.data() + sizeof(int2) * (size_t)i, wh, sizeof(wh));
    }
    if (xf) memcpy(blk.data() + off_xf, xf, sizeof(evam_transform) * (size_t)n_items);
    if (n_labels) memcpy(blk.data() + off_lab, labels, sizeof(int32_t) * (size_t)n_labels);
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = grow_device(&h->dev_cnt, &h->dev_cnt_cap, 2 * sizeof(uint32_t) * (size_t)n_items, "evam_pp_ssd_rois")) return rc;
    const uint8_t* d_blk = nullptr;
    {
        HipRings b;
        if (int rc = h->ring_ssd.upload(b, h->stream, blk.data(), blk.size(), &d_blk)) return rc;
    }
    SsdParams p{};
    p.det = det;
    p.sizes = reinterpret_cast<const int2*>(d_blk);
    p.xf = xf ? reinterpret_cast<const evam_transform*>(d_blk + off_xf) : nullptr;
    p.labels = labels ? reinterpret_cast<const int32_t*>(d_blk + off_lab) : nullptr;
    p.item_count = static_cast<uint32_t*>(h->dev_cnt);
    p.item_off = p.item_count + n_items;
    p.rois = list->rois;
    p.count = list->count;
    p.n_items = n_items; p.k = k; p.n_labels = n_labels;
    p.TW = tensor_w; p.TH = tensor_h; p.cap = list->cap;
    p.threshold = threshold;
    p.out_labels = out_labels;
    hipLaunchKernelGGL((evam_pp_ssd_rows<false>), dim3(n_items), dim3(kThreads), 0, h->stream, p);
    hipLaunchKernelGGL(evam_pp_ssd_scan, dim3(1), dim3(kThreads), 0, h->stream, p.item_count, p.item_off, n_items, p.count);
    if (out_labels) hipLaunchKernelGGL((evam_pp_ssd_rows<true, true>), dim3(n_items), dim3(kThreads), 0, h->stream, p);
    else hipLaunchKernelGGL((evam_pp_ssd_rows<true>), dim3(n_items), dim3(kThreads), 0, h->stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "evam_pp_ssd_rois: kernel launch failed: %s", hipGetErrorString(e));
    return EVAM_PP_OK;
}

int evam_pp_run_device_rois(evam_pp* h, const evam_image* srcs, int n_srcs, const evam_roi_list* list,
                            const evam_preproc* cfg, const evam_tensor* dst, int32_t* status) {
    const char* who = "evam_pp_run_device_rois";
    if (!h || !srcs || !cfg || !dst) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (int rc = check_roi_list(list, who)) return rc;
    if (n_srcs <= 0) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: n_srcs must be > 0", who);
    if (int rc = check_output(who, cfg, dst)) return rc;
    const int DW = dst->w, DH = dst->h, cap = list->cap;
    const int64_t plane = (int64_t)DW * DH;
    const int esz = out_esz(out_kind(cfg->out_dtype));
    if (dst->layout == EVAM_LAYOUT_NHWC)
        return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: interleaved (NHWC) output is not served from a device list", who);
    if (dst->layout != EVAM_LAYOUT_NCHW) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: unknown dst layout %d", who, dst->layout);
    for (int i : {0, cap - 1}) {  // slots are linear in the entry index: the first and the last bound them all
        const int64_t slot = (int64_t)dst->slot_offset + (int64_t)i * dst->slot_stride;
        if (slot < 0 || slot >= dst->n)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: entry %d -> slot %lld outside tensor batch %d", who, i, (long long)slot, dst->n);
    }
    if (int rc = validate_sources(srcs, n_srcs)) return rc;
    const int f = fmt_id(srcs[0].fourcc);
    int max_w = 0;
    for (int i = 0; i < n_srcs; i++) {
        if (fmt_id(srcs[i].fourcc) != f)
            return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: sources of more than one format in a call (srcs[%d])", who, i);
        max_w = std::max(max_w, srcs[i].width);
    }
    // Planned without the rects: staging for the widest source, occupancy from the list's capacity, units in list order.
    const Knobs& kn = h->knobs;
    QParams q{};
    int base = 1, lds = 0;
    int64_t slots = 0;
    const void* fn = nullptr;
    HIP_TRY(hipSetDevice(h->device));
    if (!plan_roi(HipKernels{}, f, DW, DH, cfg->out_dtype, kn.roi_px, row_bytes_bound(f, max_w), cap, h->n_cu, kn, q, base, lds,
                  slots, fn, true))
        return fail(EVAM_PP_ERR_UNSUPPORTED, "%s: %dx%d output from %d-wide sources is not planned by the ROI kernel", who, DW,
                    DH, max_w);
    const int64_t units = (int64_t)cap * base;
    if (units > 0x7FFFFFFF - kThreads) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: too many tiles", who);
    // host block: [LUT][RecFrame x n_srcs]
    std::vector<uint8_t>& blk = h->h_aux;
    blk.resize(kLutBytes + sizeof(RecFrame) * (size_t)n_srcs);
    block_lut(h, cfg, blk.data());
    for (int s = 0; s < n_srcs; s++) {
        const RecFrame f = rec_frame(srcs[s]);
        memcpy(blk.data() + kLutBytes + sizeof(RecFrame) * (size_t)s, &f, sizeof(f));
    }
    if (int rc = grow_device(&h->dev_recs, &h->dev_recs_cap, sizeof(RoiRec) * (size_t)units, who)) return rc;
    const uint8_t* d_blk = nullptr;
    {
        HipRings b;
        if (int rc = h->ring.upload(b, h->stream, blk.data(), blk.size(), &d_blk)) return rc;
    }
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev0, h->stream));
    DParams d{};
    d.rois = list->rois;
    d.count = list->count;
    d.srcs = reinterpret_cast<const uint4*>(d_blk + kLutBytes);
    d.recs = static_cast<RoiRec*>(h->dev_recs);
    d.status = status;
    d.cap = cap; d.n_srcs = n_srcs; d.tiles = base; d.TH = q.TH; d.DH = DH; d.fmt = f;
    hipLaunchKernelGGL(evam_pp_roi_records, dim3((unsigned)((units + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    roi_launch_fields(q, d.recs, reinterpret_cast<const float*>(d_blk), cfg, dst, dst->slot_offset, dst->slot_stride, kn.prio);
    if (int rc = launch_kernel(fn, dim3((unsigned)units), dim3(kThreads), lds, h->stream, &q, true)) return rc;
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = h->opt_timing != 0;
    h->stats.n_items = cap;
    h->stats.n_launches = 2;
    h->stats.kernels = EVAM_KERNEL_ROI;
    h->stats.src_bytes = 0;
    h->stats.dst_bytes = (int64_t)cap * plane * 3 * esz;
    return EVAM_PP_OK;
}

}  // extern "C"
