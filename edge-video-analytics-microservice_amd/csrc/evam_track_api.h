// evam_pp_track_host / evam_pp_tracker_* / evam_pp_track_device_rois: the host side of the tracker.
// Included at the end of evam_pp.hip (needs struct evam_pp, fail, HipRings); kernels in evam_track_kernels.h.
#pragma once

// The states of a tracker's streams and the due flags of its last call, all device memory. Every call waits (on the
// device) for `ev`, recorded behind the call before it, so calls through handles on different HIP streams touch the
// states and the flags one after the other, in host issue order.
struct evam_pp_tracker {
    int device = 0;
    int n_streams = 0;
    evam_track_cfg cfg{};
    evam_track_state* states = nullptr;
    uint32_t* flags = nullptr;  // due flags of one call, [flags_cap]
    size_t flags_cap = 0;
    hipEvent_t ev = nullptr;
    bool ev_rec = false;
    std::vector<uint8_t> seen;  // per-call scratch: stream slots named by the item table
};

namespace {

int track_check_gate(const char* who, const int32_t* set, int n_set, int reclassify) {
    if (n_set > 0 && !set) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL classify label set of %d", who, n_set);
    if (n_set < 0 && set) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: a label set with n_classify_labels %d", who, n_set);
    if (reclassify < 1) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: reclassify %d must be >= 1", who, reclassify);
    return 0;
}

int track_check_cfg(const char* who, const evam_track_cfg* cfg) {
    if (!cfg) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL cfg", who);
    if (cfg->max_lost < 0) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: max_lost %d must be >= 0", who, cfg->max_lost);
    return 0;
}

// Order the handle's stream behind the tracker's last call / record this call behind its launches.
int tracker_enter(evam_pp* h, evam_pp_tracker* t) {
    HIP_TRY(hipSetDevice(h->device));
    if (t->ev_rec) HIP_TRY(hipStreamWaitEvent(h->stream, t->ev, 0));
    return 0;
}
int tracker_leave(evam_pp* h, evam_pp_tracker* t) {
    HIP_TRY(hipEventRecord(t->ev, h->stream));
    t->ev_rec = true;
    return 0;
}

int tracker_args(const char* who, evam_pp* h, evam_pp_tracker* t, int stream, bool with_stream) {
    if (!h || !t) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (t->device != h->device)
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: the tracker is on device %d, the handle on %d", who, t->device, h->device);
    if (with_stream && (stream < 0 || stream >= t->n_streams))
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: stream slot %d outside [0, %d)", who, stream, t->n_streams);
    return 0;
}

}  // namespace

extern "C" {

int evam_pp_track_host(evam_track_state* state, const evam_track_cfg* cfg, uint32_t frame, const evam_roi* dets,
                       const int32_t* labels, int n_dets, const int32_t* classify_labels, int n_classify_labels,
                       int reclassify, uint32_t* ids, uint8_t* due) {
    const char* who = "evam_pp_track_host";
    if (!state) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL state", who);
    if (int rc = track_check_cfg(who, cfg)) return rc;
    if (n_dets < 0 || (n_dets > 0 && (!dets || !labels || !ids)))
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: %d detections with a NULL array", who, n_dets);
    if (int rc = track_check_gate(who, classify_labels, n_classify_labels, reclassify)) return rc;
    if (frame == EVAM_TRACK_NONE) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: frame index 0x%x is reserved", who, frame);
    if (state->next_id == 0) track_state_init(state);
    const bool gate = classify_labels != nullptr || n_classify_labels < 0;
    track_step(state, track_thr_key(cfg->iou_threshold), cfg->max_lost, frame, dets, labels, n_dets, gate, classify_labels,
               n_classify_labels, (uint32_t)reclassify, ids, due);
    return EVAM_PP_OK;
}

int evam_pp_tracker_create(evam_pp* h, int n_streams, const evam_track_cfg* cfg, evam_pp_tracker** out) {
    const char* who = "evam_pp_tracker_create";
    if (!out) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!h) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (int rc = track_check_cfg(who, cfg)) return rc;
    if (n_streams <= 0 || n_streams > 65535)
        return fail(EVAM_PP_ERR_INVALID_ARG, "%s: n_streams %d outside 1..65535", who, n_streams);
    HIP_TRY(hipSetDevice(h->device));
    evam_pp_tracker* t = new (std::nothrow) evam_pp_tracker();
    if (!t) return fail(EVAM_PP_ERR_OOM, "%s: out of host memory", who);
    t->device = h->device;
    t->n_streams = n_streams;
    t->cfg = *cfg;
    if (hipMalloc((void**)&t->states, sizeof(evam_track_state) * (size_t)n_streams) != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return fail(EVAM_PP_ERR_OOM, "%s: hipMalloc of %d states failed", who, n_streams);
    }
    if (hipEventCreateWithFlags(&t->ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(t->states);
        delete t;
        return fail(EVAM_PP_ERR_HIP, "%s: hipEventCreate failed", who);
    }
    hipLaunchKernelGGL(evam_pp_track_reset, dim3((unsigned)n_streams), dim3(kThreads), 0, h->stream, t->states);
    hipError_t e = hipGetLastError();
    int rc = e == hipSuccess ? tracker_leave(h, t) : fail(EVAM_PP_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    if (rc) {
        evam_pp_tracker_destroy(t);
        return rc;
    }
    *out = t;
    return EVAM_PP_OK;
}

void evam_pp_tracker_destroy(evam_pp_tracker* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->ev_rec) (void)hipEventSynchronize(t->ev);
    if (t->states) (void)hipFree(t->states);
    if (t->flags) (void)hipFree(t->flags);
    if (t->ev) (void)hipEventDestroy(t->ev);
    delete t;
}

int evam_pp_tracker_reset(evam_pp* h, evam_pp_tracker* t, int stream) {
    const char* who = "evam_pp_tracker_reset";
    if (int rc = tracker_args(who, h, t, stream, true)) return rc;
    if (int rc = tracker_enter(h, t)) return rc;
    hipLaunchKernelGGL(evam_pp_track_reset, dim3(1), dim3(kThreads), 0, h->stream, t->states + stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return tracker_leave(h, t);
}

int evam_pp_tracker_read(evam_pp* h, evam_pp_tracker* t, int stream, evam_track_state* out) {
    const char* who = "evam_pp_tracker_read";
    if (int rc = tracker_args(who, h, t, stream, true)) return rc;
    if (!out) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (int rc = tracker_enter(h, t)) return rc;
    HIP_TRY(hipMemcpyAsync(out, t->states + stream, sizeof(evam_track_state), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EVAM_PP_OK;
}

int evam_pp_track_device_rois(evam_pp* h, evam_pp_tracker* t, const evam_roi_list* list, const int32_t* labels,
                              int n_items, const evam_track_item* items, const int32_t* classify_labels,
                              int n_classify_labels, int reclassify, uint32_t* ids, const evam_roi_list* due) {
    const char* who = "evam_pp_track_device_rois";
    if (int rc = tracker_args(who, h, t, 0, false)) return rc;
    if (int rc = check_roi_list(list, who)) return rc;
    if (due) {
        if (int rc = check_roi_list(due, who)) return rc;
        if (due->rois == list->rois || due->count == list->count)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: the due list must be other memory than the list", who);
    }
    if (!labels || !items || !ids) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: NULL argument", who);
    if (n_items <= 0 || n_items > 65535) return fail(EVAM_PP_ERR_INVALID_ARG, "%s: n_items %d outside 1..65535", who, n_items);
    if (int rc = track_check_gate(who, classify_labels, n_classify_labels, reclassify)) return rc;
    const bool gate = classify_labels != nullptr || n_classify_labels < 0;
    const int n_set = std::max(0, n_classify_labels);
    // the item table: every stream slot's items contiguous, its frame indices ascending
    t->seen.assign((size_t)t->n_streams, 0);
    std::vector<TrkStream> runs;
    for (int i = 0; i < n_items; i++) {
        const int s = items[i].stream;
        if (s < 0 || s >= t->n_streams)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: items[%d]: stream slot %d outside [0, %d)", who, i, s, t->n_streams);
        if (items[i].frame == EVAM_TRACK_NONE)
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: items[%d]: frame index 0x%x is reserved", who, i, items[i].frame);
        if (i > 0 && items[i - 1].stream == s) {
            if (items[i].frame <= items[i - 1].frame)
                return fail(EVAM_PP_ERR_INVALID_ARG, "%s: items[%d]: frame %u of stream slot %d does not ascend (after %u)", who,
                            i, items[i].frame, s, items[i - 1].frame);
            runs.back().n++;
            continue;
        }
        if (t->seen[(size_t)s])
            return fail(EVAM_PP_ERR_INVALID_ARG, "%s: items[%d]: the items of stream slot %d are not contiguous", who, i, s);
        t->seen[(size_t)s] = 1;
        runs.push_back(TrkStream{s, i, 1, 0});
    }
    // host block: [TrkStream x runs][evam_track_item x n_items][int32 x max(1, n_set)]
    const size_t off_items = sizeof(TrkStream) * runs.size();
    const size_t off_set = off_items + sizeof(evam_track_item) * (size_t)n_items;
    std::vector<uint8_t>& blk = h->h_aux;
    blk.assign(off_set + sizeof(int32_t) * (size_t)std::max(1, n_set), 0);
    memcpy(blk.data(), runs.data(), off_items);
    memcpy(blk.data() + off_items, items, sizeof(evam_track_item) * (size_t)n_items);
    if (n_set) memcpy(blk.data() + off_set, classify_labels, sizeof(int32_t) * (size_t)n_set);
    if (int rc = tracker_enter(h, t)) return rc;
    if (due && t->flags_cap < (size_t)list->cap) {
        // grows to the largest cap seen; hipFree waits for the kernels that still use the old buffer (stated in the
        // header: the one place where this call can wait on the device)
        if (t->flags) (void)hipFree(t->flags);
        t->flags = nullptr;
        t->flags_cap = 0;
        if (hipMalloc((void**)&t->flags, sizeof(uint32_t) * (size_t)list->cap) != hipSuccess) {
            (void)hipGetLastError();
            return fail(EVAM_PP_ERR_OOM, "%s: hipMalloc of %d due flags failed", who, list->cap);
        }
        t->flags_cap = (size_t)list->cap;
    }
    const uint8_t* d_blk = nullptr;
    {
        HipRings b;
        if (int rc = h->ring_trk.upload(b, h->stream, blk.data(), blk.size(), &d_blk)) return rc;
    }
    HIP_TRY(hipMemsetAsync(ids, 0, sizeof(uint32_t) * (size_t)list->cap, h->stream));
    if (due) HIP_TRY(hipMemsetAsync(t->flags, 0, sizeof(uint32_t) * (size_t)list->cap, h->stream));
    TrkParams p{};
    p.states = t->states;
    p.rois = list->rois;
    p.count = list->count;
    p.labels = labels;
    p.streams = reinterpret_cast<const TrkStream*>(d_blk);
    p.items = reinterpret_cast<const evam_track_item*>(d_blk + off_items);
    p.set = reinterpret_cast<const int32_t*>(d_blk + off_set);
    p.ids = ids;
    p.flags = due ? t->flags : nullptr;
    p.cap = list->cap;
    p.n_set = n_classify_labels < 0 ? -1 : n_set;
    p.gate = gate ? 1 : 0;
    p.max_lost = t->cfg.max_lost;
    p.thr_key = track_thr_key(t->cfg.iou_threshold);
    p.reclassify = (uint32_t)reclassify;
    hipLaunchKernelGGL(evam_pp_track, dim3((unsigned)runs.size()), dim3(kThreads), 0, h->stream, p);
    if (due)
        hipLaunchKernelGGL(evam_pp_track_emit, dim3(1), dim3(kThreads), 0, h->stream, list->rois, list->count, list->cap,
                           t->flags, due->rois, due->count, due->cap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EVAM_PP_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return tracker_leave(h, t);
}

}  // extern "C"
