// Device-resident ROI lists: evam_pp_roi_records (list -> ROI-kernel records) and evam_pp_ssd_rows / evam_pp_ssd_scan
// (SSD rows -> list). Included by evam_pp.hip after the kernel families; reopens its anonymous namespace. Entry points
// in evam_rois_api.h. Not evam_roi_kernels.h (singular): that header is evam_pp_roi, the kernel these records feed.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------
// device-resident ROI lists (evam_pp_ssd_rois, evam_pp_run_device_rois)
// ------------------------------------------------------------------------------------------------
// Records kernel: one thread per (list entry, row tile) of the list's capacity writes that unit's RoiRec, in list
// order, from the entry and the per-source table (RecFrame per source: the frame half of a record). An entry past
// min(*count, cap), with a src_index outside the sources, or whose rect clips to nothing (roi_clip, the host's own
// rule) gets the row range [0, 0): evam_pp_roi<.., DEV = true> returns on it. Ordinary vector stores: the ROI kernel
// launched next on the stream sees them through the kernel boundary.
struct DParams {
    const evam_roi* rois;
    const uint32_t* count;
    const uint4* srcs;  // [n_srcs][3]
    RoiRec* recs;       // [cap * tiles]
    int32_t* status;    // NULL or [cap]
    int cap, n_srcs, tiles, TH, DH, fmt;
};

__global__ __launch_bounds__(kThreads) void evam_pp_roi_records(const DParams P) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= P.cap * P.tiles) return;
    const int e = u / P.tiles, t = u - e * P.tiles;
    const uint32_t cnt = *P.count;
    bool live = (uint32_t)e < cnt;  // e < cap by the grid
    int st = 0;
    uint4 l0 = {0u, 0u, 0u, 0u}, l1 = l0, l2 = l0;
    int rx = 0, ry = 0, rw = 0, rh = 0;
    if (live) {
        const int32_t* r = reinterpret_cast<const int32_t*>(P.rois + e);
        const int si = r[0];
        rx = r[1]; ry = r[2]; rw = r[3]; rh = r[4];
        if ((unsigned)si >= (unsigned)P.n_srcs) {
            st = EVAM_PP_ERR_INVALID_ARG;
            live = false;
        } else {
            l0 = P.srcs[3 * si];
            l1 = P.srcs[3 * si + 1];
            l2 = P.srcs[3 * si + 2];  // pitch[2], width | height << 16, 0, 0
            Geom g;
            if (roi_clip(P.fmt, (int)(l2.y & 0xFFFF), (int)(l2.y >> 16), true, rx, ry, rw, rh, g)) {
                st = EVAM_PP_ERR_EMPTY_ROI;
                live = false;
            }
        }
    }
    const uint32_t row0 = live ? (uint32_t)(t * P.TH) : 0u;
    const uint32_t row1 = live ? (uint32_t)min(P.DH, (t + 1) * P.TH) : 0u;
    uint4* o = reinterpret_cast<uint4*>(P.recs + u);
    o[0] = l0;
    o[1] = l1;
    o[2] = make_uint4(l2.x, l2.y, (uint32_t)rx, (uint32_t)ry);
    o[3] = make_uint4((uint32_t)rw, (uint32_t)rh, (uint32_t)e, row0 | (row1 << 16));
    if (t == 0 && P.status) P.status[e] = st;
}

// SSD rows -> ROI list, an ordered compaction in three launches: evam_pp_ssd_rows<false> counts the accepted rows
// of every item (one workgroup per item), evam_pp_ssd_scan turns the counts into each item's first list position and
// the total, evam_pp_ssd_rows<true> evaluates the rows again and writes every accepted rect at its position: item
// order, then row order, as the host path lists them. ssd_row_rect (evam_geom.h) is the host's arithmetic.
struct SsdParams {
    const float* det;          // [n_items][k][7]
    const int2* sizes;         // per item: its frame's (width, height)
    const evam_transform* xf;  // per item, or NULL: identity
    const int32_t* labels;     // accepted label ids, or NULL: all
    uint32_t* item_count;      // [n_items]
    uint32_t* item_off;        // [n_items]
    evam_roi* rois;
    uint32_t* count;
    int n_items, k, n_labels, TW, TH, cap;
    float threshold;
    int32_t* out_labels;       // evam_pp_ssd_rois_ex (LAB): the label of each list entry, [cap]
};

template <bool EMIT, bool LAB = false>
__global__ __launch_bounds__(kThreads) void evam_pp_ssd_rows(const SsdParams P) {
    __shared__ int s_end;
    __shared__ uint32_t s_w[kThreads / 64];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* d = P.det + (size_t)i * (size_t)P.k * 7;
    if (tid == 0) s_end = P.k;
    __syncthreads();
    // the rows before the first image_id < 0
    for (int r = tid; r < P.k; r += kThreads)
        if (d[(size_t)r * 7] < 0.f) {
            atomicMin(&s_end, r);
            break;
        }
    __syncthreads();
    const int kend = s_end;
    const int2 wh = P.sizes[i];
    const evam_transform* xf = P.xf ? P.xf + i : nullptr;
    const uint32_t base = EMIT ? P.item_off[i] : 0u;
    uint32_t total = 0;
    for (int r0 = 0; r0 < kend; r0 += kThreads) {  // kend is uniform: every thread takes every barrier
        const int r = r0 + tid;
        int x = 0, y = 0, w = 0, h = 0;
        const bool acc = r < kend && ssd_row_rect(d + (size_t)r * 7, xf, wh.x, wh.y, P.TW, P.TH, P.threshold, P.labels,
                                                  P.n_labels, x, y, w, h);
        const unsigned long long m = __ballot(acc);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int v = 0; v < kThreads / 64; v++) {
            before += v < wave ? s_w[v] : 0u;
            all += s_w[v];
        }
        if (EMIT && acc) {
            const uint32_t pos = base + total + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < (uint32_t)P.cap) {
                int32_t* o = reinterpret_cast<int32_t*>(P.rois + pos);
                o[0] = i; o[1] = x; o[2] = y; o[3] = w; o[4] = h;
                if (LAB) {  // int(label), as the host path truncates it
                    const float lf = d[(size_t)r * 7 + 1];
                    P.out_labels[pos] = (lf - lf == 0.f) && lf < 2147483648.f && lf >= -2147483648.f ? (int32_t)lf : 0;
                }
            }
        }
        total += all;
        __syncthreads();  // s_w is rewritten by the next chunk
    }
    if (!EMIT && tid == 0) P.item_count[i] = total;
}

__global__ __launch_bounds__(kThreads) void evam_pp_ssd_scan(const uint32_t* cnt, uint32_t* off, int n, uint32_t* total) {
    __shared__ uint32_t s[kThreads];
    const int tid = threadIdx.x;
    uint32_t running = 0;
    for (int i0 = 0; i0 < n; i0 += kThreads) {
        const int i = i0 + tid;
        const uint32_t v = i < n ? cnt[i] : 0u;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < kThreads; d <<= 1) {  // inclusive scan of the chunk
            const uint32_t a = tid >= d ? s[tid - d] : 0u;
            __syncthreads();
            s[tid] += a;
            __syncthreads();
        }
        if (i < n) off[i] = running + s[tid] - v;
        running += s[kThreads - 1];
        __syncthreads();
    }
    if (tid == 0) *total = running;
}

}  // namespace
