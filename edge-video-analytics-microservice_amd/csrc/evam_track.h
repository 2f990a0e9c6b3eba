// evam_track.h — the gvatrack rule of libevam_pp.so: object ids by greedy IoU matching and the
// reclassify-interval gate, in integer arithmetic only, so the host (evam_pp_track_host, the pipeline's TrackStage)
// and the evam_pp_track kernel agree bit for bit. tests/native/track_check.cpp compiles this header for the host alone
// under AddressSanitizer / UBSan; tests/track_ref.py restates the rule in Python.
//
// EVAM_HD marks what the kernel calls too (evam_pp.hip defines it as __host__ __device__ first): track_key scores a
// (track, detection) pair, track_pack orders the candidates, track_due is the gate. track_step is the rule driven
// sequentially on the host; the kernel drives the same three functions with one workgroup per stream.
//
// The rule (DESIGN.md §3 ledger; DL Streamer's tracker is closed, this is the project's convention):
//   1. the first EVAM_TRACK_DETS detections of a frame take part, the rest get id 0;
//   2. key = (inter << 16) / union of a live track and a detection of the same label; a candidate when key >= thr_key;
//   3. repeatedly the candidate with the largest key among unmatched tracks and detections is matched (ties: lower
//      slot, then lower detection index);
//   4. a match copies the box into the track, lost = 0, the detection takes the track's id;
//   5. an unmatched live track: lost += 1, freed when lost > max_lost;
//   6. unmatched detections, in order, take the lowest free slot with id = next_id++ (no slot: id 0);
//   7. with a classify label set, a detection of such a label is due when its id is 0, its track was never classified,
//      or frame - classified_at >= reclassify; a due detection with an id sets classified_at = frame.
#ifndef EVAM_TRACK_H
#define EVAM_TRACK_H

#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../include/evam_pp.h"

#ifndef EVAM_HD
#define EVAM_HD
#endif

namespace evam {

constexpr int kTrackSlots = EVAM_TRACK_SLOTS;  // T
constexpr int kTrackDets = EVAM_TRACK_DETS;    // D
constexpr int64_t kTrackSideMax = 1 << 20;     // a box side counts as min(max(side, 0), 2^20): areas stay below 2^41

// floor(iou_threshold * 65536) in double, clamped to [0, 65536]; NaN gives 65536 (only identical boxes match).
inline uint32_t track_thr_key(float iou_threshold) {
    const double v = (double)iou_threshold * 65536.0;
    if (!(v < 65536.0)) return 65536u;
    return v <= 0.0 ? 0u : (uint32_t)v;
}

// The key of a pair: (inter << 16) / union, 0..65536. false when the pair is no candidate (labels differ, both boxes
// empty, or key < thr_key).
EVAM_HD inline bool track_key(int32_t tl, int32_t tx, int32_t ty, int32_t tw, int32_t th, int32_t dl, int32_t dx,
                              int32_t dy, int32_t dw, int32_t dh, uint32_t thr_key, uint32_t& key) {
    if (tl != dl) return false;
    const int64_t w0 = tw < 0 ? 0 : (tw > kTrackSideMax ? kTrackSideMax : tw);
    const int64_t h0 = th < 0 ? 0 : (th > kTrackSideMax ? kTrackSideMax : th);
    const int64_t w1 = dw < 0 ? 0 : (dw > kTrackSideMax ? kTrackSideMax : dw);
    const int64_t h1 = dh < 0 ? 0 : (dh > kTrackSideMax ? kTrackSideMax : dh);
    const int64_t xa = tx > dx ? tx : dx, ya = ty > dy ? ty : dy;
    const int64_t xb = (int64_t)tx + w0 < (int64_t)dx + w1 ? (int64_t)tx + w0 : (int64_t)dx + w1;
    const int64_t yb = (int64_t)ty + h0 < (int64_t)dy + h1 ? (int64_t)ty + h0 : (int64_t)dy + h1;
    const int64_t iw = xb > xa ? xb - xa : 0, ih = yb > ya ? yb - ya : 0;
    const uint64_t inter = (uint64_t)(iw * ih);
    const uint64_t uni = (uint64_t)(w0 * h0 + w1 * h1) - inter;
    if (uni == 0) return false;
    key = inter ? (uint32_t)((inter << 16) / uni) : 0u;  // most pairs are disjoint: no division for them
    return key >= thr_key;
}

// A candidate as one word whose maximum is the pair to match next: larger key, then lower slot, then lower detection
// index. Never 0, so 0 stands for "no candidate".
EVAM_HD inline uint32_t track_pack(uint32_t key, int slot, int det) {
    return ((key + 1u) << 14) | ((uint32_t)(kTrackSlots - 1 - slot) << 7) | (uint32_t)(kTrackDets - 1 - det);
}
EVAM_HD inline int track_pack_slot(uint32_t p) { return kTrackSlots - 1 - (int)((p >> 7) & 127u); }
EVAM_HD inline int track_pack_det(uint32_t p) { return kTrackDets - 1 - (int)(p & 127u); }

// The classify label set: NULL with n < 0 is every label.
EVAM_HD inline bool track_label_in(int32_t label, const int32_t* set, int n) {
    if (n < 0) return true;
    bool hit = false;
    for (int j = 0; j < n; j++) hit |= set[j] == label;
    return hit;
}

// Step 7 for a detection whose label is in the set: id 0 (slot == NULL) is always due.
EVAM_HD inline bool track_due(evam_track_slot* slot, uint32_t frame, uint32_t reclassify) {
    if (!slot) return true;
    if (slot->classified_at != EVAM_TRACK_NONE && frame - slot->classified_at < reclassify) return false;
    slot->classified_at = frame;
    return true;
}

inline void track_state_init(evam_track_state* s) {
    *s = evam_track_state{};
    s->next_id = 1;
    for (int t = 0; t < kTrackSlots; t++) s->slots[t].classified_at = EVAM_TRACK_NONE;
}

// One frame of one stream, sequentially. gate: run step 7 (n_set < 0: every label). ids: [n]; due: [n], or NULL when
// the caller wants no flags (the gate still runs).
inline void track_step(evam_track_state* s, uint32_t thr_key, int max_lost, uint32_t frame, const evam_roi* dets,
                       const int32_t* labels, int n, bool gate, const int32_t* set, int n_set, uint32_t reclassify,
                       uint32_t* ids, uint8_t* due) {
    const int m = n < kTrackDets ? n : kTrackDets;
    int det_slot[kTrackDets];    // the slot a participating detection was matched to / created in, or -1
    bool slot_hit[kTrackSlots];  // matched this frame
    for (int d = 0; d < m; d++) det_slot[d] = -1;
    for (int t = 0; t < kTrackSlots; t++) slot_hit[t] = false;
    // every candidate once, in the order the repeated arg-max takes them: a pair is matched when it is reached with
    // both its track and its detection still unmatched
    std::vector<uint32_t> cand;
    for (int t = 0; t < kTrackSlots; t++) {
        const evam_track_slot& k = s->slots[t];
        if (!k.id) continue;
        for (int d = 0; d < m; d++) {
            uint32_t key;
            if (track_key(k.label, k.x, k.y, k.w, k.h, labels[d], dets[d].x, dets[d].y, dets[d].w, dets[d].h, thr_key, key))
                cand.push_back(track_pack(key, t, d));
        }
    }
    std::sort(cand.begin(), cand.end(), std::greater<uint32_t>());
    for (const uint32_t p : cand) {
        const int t = track_pack_slot(p), d = track_pack_det(p);
        if (slot_hit[t] || det_slot[d] >= 0) continue;
        evam_track_slot& k = s->slots[t];
        k.x = dets[d].x; k.y = dets[d].y; k.w = dets[d].w; k.h = dets[d].h;
        k.lost = 0;
        slot_hit[t] = true;
        det_slot[d] = t;
    }
    for (int t = 0; t < kTrackSlots; t++) {
        evam_track_slot& k = s->slots[t];
        if (!k.id || slot_hit[t]) continue;
        if (++k.lost > max_lost) {
            k = evam_track_slot{};
            k.classified_at = EVAM_TRACK_NONE;
        }
    }
    int free_from = 0;
    for (int d = 0; d < m; d++) {
        if (det_slot[d] >= 0) continue;
        while (free_from < kTrackSlots && s->slots[free_from].id) free_from++;
        if (free_from == kTrackSlots) break;
        evam_track_slot& k = s->slots[free_from];
        k.id = s->next_id++;
        k.label = labels[d];
        k.x = dets[d].x; k.y = dets[d].y; k.w = dets[d].w; k.h = dets[d].h;
        k.lost = 0;
        k.classified_at = EVAM_TRACK_NONE;
        det_slot[d] = free_from;
    }
    for (int d = 0; d < n; d++) {
        evam_track_slot* k = d < m && det_slot[d] >= 0 ? &s->slots[det_slot[d]] : nullptr;
        ids[d] = k ? k->id : 0u;
        // the gate runs with or without a due array: classified_at is state, the flag only its report
        const bool is_due = gate && track_label_in(labels[d], set, n_set) && track_due(k, frame, reclassify);
        if (due) due[d] = is_due ? 1 : 0;
    }
}

}  // namespace evam

#endif  // EVAM_TRACK_H
