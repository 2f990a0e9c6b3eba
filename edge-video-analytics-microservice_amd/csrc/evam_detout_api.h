// evam_pp_detection_output / evam_pp_detection_output_host / evam_pp_expf: the host side of SSD DetectionOutput.
// Included at the end of evam_pp.hip (needs struct evam_pp, fail, and grow_device of evam_rois_api.h); kernels in evam_detout_kernels.h.
#pragma once

namespace {

int detout_check(const char* who, const float* loc, const float* conf, const float* priors, int n, int p,
                 const evam_detout_cfg* cfg, const float* out) {
    if (!loc) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: loc is NULL", who);
    if (!conf) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: conf is NULL", who);
    if (!priors) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: priors is NULL", who);
    if (!out) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out is NULL", who);
    char msg[256];
    if (int rc = detout_validate(n, p, cfg, msg, sizeof(msg))) return fail(rc, "%s: %s", who, msg);
    return 0;
}

}  // namespace

extern "C" {

float evam_pp_expf(float x) { return evam_expf(x); }

int evam_pp_detection_output_host(const float* loc, const float* conf, const float* priors, int n, int p,
                                  const evam_detout_cfg* cfg, float* out, uint32_t* counts) {
    if (int rc = detout_check("evam_pp_detection_output_host", loc, conf, priors, n, p, cfg, out)) return rc;
    const size_t P = (size_t)p, C = (size_t)cfg->num_classes, K = (size_t)cfg->keep_top_k;
    for (int i = 0; i < n; i++) {
        const uint32_t m = detout_image(i, loc + (size_t)i * P * 4, conf + (size_t)i * P * C, priors, p, *cfg,
                                        out + (size_t)i * K * 7);
        if (counts) counts[i] = m;
    }
    return EVAM_PP_OK;
}

int evam_pp_detection_output(evam_pp* h, const float* loc, const float* conf, const float* priors, int n, int p,
                             const evam_detout_cfg* cfg, float* out, uint32_t* counts) {
    const char* who = "evam_pp_detection_output";
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (int rc = detout_check(who, loc, conf, priors, n, p, cfg, out)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // scratch: [uint32 x n x C, rounded up to 256 bytes][uint64 x n x C x top_k]
    const size_t nc = (size_t)n * (size_t)cfg->num_classes;
    const size_t off_keys = (nc * sizeof(uint32_t) + 255) & ~(size_t)255;
    const size_t bytes = off_keys + nc * (size_t)cfg->top_k * sizeof(uint64_t);
    if (int rc = grow_device(&h->dev_detout, &h->dev_detout_cap, bytes, who)) return rc;
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev0, h->stream));
    DetoutParams q{};
    q.loc = loc;
    q.conf = conf;
    q.priors = priors;
    q.kcount = static_cast<uint32_t*>(h->dev_detout);
    q.keys = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(h->dev_detout) + off_keys);
    q.out = out;
    q.counts = counts;
    q.n = n; q.p = p; q.c = cfg->num_classes; q.bg = cfg->background_label;
    q.top_k = cfg->top_k; q.keep_top_k = cfg->keep_top_k;
    q.conf_thr = cfg->confidence_threshold; q.nms_thr = cfg->nms_threshold;
    hipLaunchKernelGGL(evam_pp_detout_class, dim3((unsigned)cfg->num_classes, (unsigned)n), dim3(kThreads), 0, h->stream, q);
    hipLaunchKernelGGL(evam_pp_detout_merge, dim3((unsigned)n), dim3(kThreads), 0, h->stream, q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    if (h->opt_timing) HIP_TRY(hipEventRecord(h->ev1, h->stream));
    h->timed = h->opt_timing != 0;
    h->stats = evam_pp_stats{};
    h->stats.n_items = n;
    h->stats.n_launches = 2;
    h->stats.kernels = EVAM_KERNEL_DETOUT;
    return EVAM_PP_OK;
}

}  // extern "C"
