// evam_pp_track and its helpers: the gvatrack rule (evam_track.h) over a device ROI list.
// Included by evam_pp.hip inside its anonymous namespace's reach (kThreads, evam:: names).
#pragma once

namespace {

constexpr int kTrkStride = kTrackDets + 1;  // words per candidate row: odd, so rows fall on different LDS banks

struct TrkStream {  // 16 B: one workgroup's work
    int32_t slot;   // the tracker's stream slot
    int32_t first;  // its first item of the call
    int32_t n;      // its items (contiguous)
    int32_t pad;
};

struct TrkParams {
    evam_track_state* states;       // the tracker's [n_streams]
    const evam_roi* rois;           // the list, in item order
    const uint32_t* count;
    const int32_t* labels;          // [cap]
    const TrkStream* streams;       // [gridDim.x]
    const evam_track_item* items;   // [n_items]
    const int32_t* set;             // the classify label set (n_set > 0)
    uint32_t* ids;                  // [cap], zeroed before the launch
    uint32_t* flags;                // [cap] due flags, zeroed before the launch; NULL without a due list
    int cap, n_set, gate, max_lost;
    uint32_t thr_key, reclassify;
};

// First list position in [0, n) whose src_index >= item (the list is in item order). Ends for any contents, and the
// result stays in [0, n].
__device__ inline int trk_lower_bound(const evam_roi* rois, int n, int item) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rois[mid].src_index < item) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One workgroup per stream slot of the call; it walks the slot's items in order. The slot's state (4 KB) and the
// frame's packed candidates (T rows of D words, padded to kTrkStride so that a row scan and a column scan are both free
// of bank conflicts; 0 = none) live in LDS.
//
// The rule matches the largest candidate among unmatched tracks and detections, again and again. The packed words are
// distinct (each holds its own slot and detection), so that order is strict, and a pair that is the maximum of both its
// row and its column is taken by the rule before any other pair of that row or column: all such pairs can be matched
// at once, and repeating this gives the rule's matching exactly. A round: 128 threads take a detection each and find
// its column's maximum over unmatched slots, the other 128 a slot each and its row's maximum over unmatched detections;
// after a barrier the detections whose column maximum is also its row's maximum match. The largest candidate left is
// always such a pair, so every round but the last matches something: at most min(T, D) + 1 rounds, two or three on
// frames whose objects moved a little.
//
// Every barrier sits in a loop whose trip count is the same for all threads: the item loop (P.streams[b].n), the round
// loop (bounded, and left by all threads together on the same LDS word).
__global__ __launch_bounds__(kThreads) void evam_pp_track(const TrkParams P) {
    __shared__ evam_track_state st;
    __shared__ uint32_t keys[kTrackSlots * kTrkStride];
    __shared__ uint32_t s_rowmax[kTrackSlots], s_colmax[kTrackDets];
    __shared__ int32_t s_any[2];            // a round matched something (double-buffered by round parity)
    __shared__ int32_t d_lab[kTrackDets];
    __shared__ int32_t d_box[kTrackDets][4];
    __shared__ int32_t d_slot[kTrackDets];  // detection -> its slot, or -1
    __shared__ int32_t s_hit[kTrackSlots];  // slot matched in this frame
    __shared__ int32_t s_lo, s_hi, s_top;
    static_assert(kTrackSlots == 128 && kTrackDets == 128 && kThreads == 256, "the index arithmetic below assumes them");
    static_assert(sizeof(evam_track_state) % 4 == 0, "copied as words");

    const int tid = threadIdx.x;
    const TrkStream ws = P.streams[blockIdx.x];
    uint32_t* gs = reinterpret_cast<uint32_t*>(P.states + ws.slot);
    uint32_t* ls = reinterpret_cast<uint32_t*>(&st);
    constexpr int kWords = (int)(sizeof(evam_track_state) / 4);
    for (int i = tid; i < kWords; i += kThreads) ls[i] = gs[i];
    const uint32_t cnt = *P.count;
    const int n_live = (int)(cnt < (uint32_t)P.cap ? cnt : (uint32_t)P.cap);
    __syncthreads();

    for (int it = 0; it < ws.n; it++) {
        const int item = ws.first + it;
        const uint32_t frame = P.items[item].frame;
        if (tid == 0) s_lo = trk_lower_bound(P.rois, n_live, item);
        if (tid == 64) s_hi = trk_lower_bound(P.rois, n_live, item + 1);
        if (tid == 128) s_top = 0;
        __syncthreads();
        const int lo = s_lo;
        const int n = s_hi > lo ? s_hi - lo : 0;  // lo + n <= n_live <= cap
        const int m = n < kTrackDets ? n : kTrackDets;
        if (tid < kTrackDets) {
            d_slot[tid] = -1;
            s_hit[tid] = 0;
            if (tid < m) {
                const int32_t* r = reinterpret_cast<const int32_t*>(P.rois + lo + tid);
                d_box[tid][0] = r[1]; d_box[tid][1] = r[2]; d_box[tid][2] = r[3]; d_box[tid][3] = r[4];
                d_lab[tid] = P.labels[lo + tid];
            }
        } else if (st.slots[tid - kTrackDets].id) {
            atomicMax(&s_top, tid - kTrackDets + 1);
        }
        __syncthreads();
        // rows of live slots only: [0, top) holds every live slot
        const int top = s_top;
        const int n_pairs = top * kTrackDets;
        const int det = tid & (kTrackDets - 1);
        for (int p = tid; p < n_pairs; p += kThreads) {
            const int slot = p >> 7;
            const evam_track_slot& k = st.slots[slot];
            uint32_t v = 0, key;
            if (det < m && k.id &&
                track_key(k.label, k.x, k.y, k.w, k.h, d_lab[det], d_box[det][0], d_box[det][1], d_box[det][2],
                          d_box[det][3], P.thr_key, key))
                v = track_pack(key, slot, det);
            keys[slot * kTrkStride + det] = v;
        }
        __syncthreads();
        const int max_rounds = (top < m ? top : m) + 1;  // uniform
        for (int round = 0; round < max_rounds; round++) {
            if (tid == 0) s_any[round & 1] = 0;
            if (tid < kTrackDets) {  // a column: this detection against the unmatched slots
                uint32_t best = 0;
                if (tid < m && d_slot[tid] < 0)
                    for (int t = 0; t < top; t++)
                        if (!s_hit[t]) best = max(best, keys[t * kTrkStride + tid]);
                s_colmax[tid] = best;
            } else {                 // a row: this slot against the unmatched detections
                const int t = tid - kTrackDets;
                uint32_t best = 0;
                if (t < top && !s_hit[t])
                    for (int d = 0; d < m; d++)
                        if (d_slot[d] < 0) best = max(best, keys[t * kTrkStride + d]);
                s_rowmax[t] = best;
            }
            __syncthreads();
            if (tid < m) {
                const uint32_t p = s_colmax[tid];
                if (p != 0 && s_rowmax[track_pack_slot(p)] == p) {  // the maximum of its row and of its column
                    const int t = track_pack_slot(p);                // t < top; track_pack_det(p) == tid
                    evam_track_slot& k = st.slots[t];
                    k.x = d_box[tid][0]; k.y = d_box[tid][1]; k.w = d_box[tid][2]; k.h = d_box[tid][3];
                    k.lost = 0;
                    s_hit[t] = 1;
                    d_slot[tid] = t;
                    s_any[round & 1] = 1;
                }
            }
            __syncthreads();  // the matches are in place for the next round's scans and for what follows the loop
            if (!s_any[round & 1]) break;  // the same word for every thread: all leave together
        }
        if (tid < kTrackSlots) {
            evam_track_slot& k = st.slots[tid];
            if (k.id && !s_hit[tid] && ++k.lost > P.max_lost) {
                k.id = 0; k.label = 0; k.x = 0; k.y = 0; k.w = 0; k.h = 0; k.lost = 0;
                k.classified_at = EVAM_TRACK_NONE;
            }
        }
        __syncthreads();
        if (tid == 0) {  // births, in detection order into the lowest free slots: at most T + D steps
            int free_from = 0;
            for (int d = 0; d < m; d++) {
                if (d_slot[d] >= 0) continue;
                while (free_from < kTrackSlots && st.slots[free_from].id) free_from++;
                if (free_from == kTrackSlots) break;
                evam_track_slot& k = st.slots[free_from];
                k.id = st.next_id++;
                k.label = d_lab[d];
                k.x = d_box[d][0]; k.y = d_box[d][1]; k.w = d_box[d][2]; k.h = d_box[d][3];
                k.lost = 0;
                k.classified_at = EVAM_TRACK_NONE;
                d_slot[d] = free_from;
            }
        }
        __syncthreads();
        // ids and the gate: a track is matched to one detection of the frame at most, so the detections are independent
        for (int d = tid; d < n; d += kThreads) {
            const int slot = d < m ? d_slot[d] : -1;
            evam_track_slot* k = slot >= 0 ? &st.slots[slot] : nullptr;
            const int e = lo + d;
            P.ids[e] = k ? k->id : 0u;
            if (P.gate) {
                const int32_t lab = d < m ? d_lab[d] : P.labels[e];
                const bool is_due = track_label_in(lab, P.set, P.n_set) && track_due(k, frame, P.reclassify);
                if (P.flags && is_due) P.flags[e] = 1u;
            }
        }
        __syncthreads();  // the next item rewrites the detection arrays
    }
    for (int i = tid; i < kWords; i += kThreads) gs[i] = ls[i];
}

// Fresh states: one workgroup per state of `states`.
__global__ __launch_bounds__(kThreads) void evam_pp_track_reset(evam_track_state* states) {
    uint32_t* g = reinterpret_cast<uint32_t*>(states + blockIdx.x);
    constexpr int kWords = (int)(sizeof(evam_track_state) / 4);
    constexpr int kHead = (int)(offsetof(evam_track_state, slots) / 4);
    for (int i = threadIdx.x; i < kWords; i += kThreads) {
        uint32_t v = 0;
        if (i == 0) v = 1u;                                        // next_id
        else if (i >= kHead && ((i - kHead) & 7) == 7) v = EVAM_TRACK_NONE;  // classified_at: word 7 of a 32-byte slot
        g[i] = v;
    }
}

// The due entries of the list, in list order: one workgroup walks the live entries in chunks of kThreads, ranks each
// chunk's flags with a ballot and a four-word scan (as evam_pp_ssd_rows ranks accepted rows), and copies each due entry
// to its position. *due_count is the true total.
__global__ __launch_bounds__(kThreads) void evam_pp_track_emit(const evam_roi* rois, const uint32_t* count, int cap,
                                                               const uint32_t* flags, evam_roi* due_rois,
                                                               uint32_t* due_count, int due_cap) {
    __shared__ uint32_t s_w[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t cnt = *count;
    const int n_live = (int)(cnt < (uint32_t)cap ? cnt : (uint32_t)cap);
    uint32_t total = 0;
    for (int e0 = 0; e0 < n_live; e0 += kThreads) {  // n_live is uniform: every thread takes every barrier
        const int e = e0 + tid;
        const bool acc = e < n_live && flags[e] != 0u;
        const unsigned long long m = __ballot(acc);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int v = 0; v < kThreads / 64; v++) {
            before += v < wave ? s_w[v] : 0u;
            all += s_w[v];
        }
        if (acc) {
            const uint32_t pos = total + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < (uint32_t)due_cap) {
                const int32_t* r = reinterpret_cast<const int32_t*>(rois + e);
                int32_t* o = reinterpret_cast<int32_t*>(due_rois + pos);
                o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4];
            }
        }
        total += all;
        __syncthreads();  // s_w is rewritten by the next chunk
    }
    if (tid == 0) *due_count = total;
}

}  // namespace
