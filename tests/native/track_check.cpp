// The gvatrack rule of csrc/evam_track.h (track_step: what evam_pp_track_host runs) as a stand-alone program for
// AddressSanitizer / UBSan (tests/test_native_asan_track.py). It reads detection sequences from a file the test wrote
// (tests/track_ref.random_sequences), runs the rule with the state and every frame's arrays in exactly-sized heap
// allocations, and writes each detection's id and due flag and each stream's final state for the test to compare with
// the Python reference. The first stream is stepped a second time on a state of its own with a NULL due pointer: ids and
// state must equal the run with a due array (the gate runs either way). Last, the key of every pair of a grid of extreme
// boxes is written out for the test to compare with the reference's.
//
// Input (text): "n_streams max_lost iou_threshold n_set set... reclassify", then per stream "n_frames", per frame
// "frame_index n" and n rows "label x y w h". n_set = -2: no gate; -1: every label.
// Output (text): per frame "ids... | due...", per stream "state next_id" and 128 rows of a slot's 8 fields; then per
// extreme pair "key tx ty tw th dx dy dw dh k" (k = -1: no candidate at threshold 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../edge-video-analytics-microservice_amd/csrc/evam_track.h"

using namespace evam;

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: track_check IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    int n_streams, max_lost, n_set, reclassify;
    float iou;
    if (fscanf(in, "%d %d %f %d", &n_streams, &max_lost, &iou, &n_set) != 4) return 2;
    std::unique_ptr<int32_t[]> set(new int32_t[n_set > 0 ? n_set : 0]);
    for (int j = 0; j < n_set; j++)
        if (fscanf(in, "%d", &set[j]) != 1) return 2;
    if (fscanf(in, "%d", &reclassify) != 1) return 2;
    const bool gate = n_set != -2;
    const uint32_t thr = track_thr_key(iou);
    long steps = 0, dets_total = 0, null_steps = 0;
    for (int s = 0; s < n_streams; s++) {
        std::unique_ptr<evam_track_state> st(new evam_track_state);
        track_state_init(st.get());
        std::unique_ptr<evam_track_state> st_null(new evam_track_state);  // the same steps with due == NULL (stream 0)
        track_state_init(st_null.get());
        int n_frames;
        if (fscanf(in, "%d", &n_frames) != 1) return 2;
        for (int f = 0; f < n_frames; f++) {
            unsigned frame;
            int n;
            if (fscanf(in, "%u %d", &frame, &n) != 2 || n < 0) return 2;
            // exactly n elements each: a read or write past a frame's detections is a heap overflow
            std::unique_ptr<evam_roi[]> dets(new evam_roi[n]);
            std::unique_ptr<int32_t[]> labels(new int32_t[n]);
            std::unique_ptr<uint32_t[]> ids(new uint32_t[n]);
            std::unique_ptr<uint8_t[]> due(new uint8_t[n]);
            for (int d = 0; d < n; d++) {
                dets[d].src_index = 0;
                if (fscanf(in, "%d %d %d %d %d", &labels[d], &dets[d].x, &dets[d].y, &dets[d].w, &dets[d].h) != 5) return 2;
            }
            track_step(st.get(), thr, max_lost, frame, dets.get(), labels.get(), n, gate, n_set > 0 ? set.get() : nullptr,
                       n_set == -2 ? 0 : n_set, (uint32_t)reclassify, ids.get(), due.get());
            if (s == 0) {
                std::unique_ptr<uint32_t[]> ids_null(new uint32_t[n]);
                track_step(st_null.get(), thr, max_lost, frame, dets.get(), labels.get(), n, gate,
                           n_set > 0 ? set.get() : nullptr, n_set == -2 ? 0 : n_set, (uint32_t)reclassify, ids_null.get(),
                           nullptr);
                if ((n && memcmp(ids_null.get(), ids.get(), sizeof(uint32_t) * (size_t)n)) ||
                    memcmp(st_null.get(), st.get(), sizeof(evam_track_state))) {
                    fprintf(stderr, "frame %u: a NULL due pointer changed the ids or the state\n", frame);
                    return 1;
                }
                null_steps++;
            }
            for (int d = 0; d < n; d++) fprintf(out, "%u ", ids[d]);
            fprintf(out, "|");
            for (int d = 0; d < n; d++) fprintf(out, " %d", (int)due[d]);
            fprintf(out, "\n");
            steps++;
            dets_total += n;
        }
        fprintf(out, "state %u\n", st->next_id);
        for (int t = 0; t < kTrackSlots; t++) {
            const evam_track_slot& k = st->slots[t];
            fprintf(out, "%u %d %d %d %d %d %d %u\n", k.id, k.label, k.x, k.y, k.w, k.h, k.lost, k.classified_at);
        }
    }
    // extreme boxes: the key arithmetic stays inside 64 bits for any int32 input, and every key goes to the test
    const int32_t ext[] = {INT32_MIN, -(1 << 20), -1, 0, 1, 7, 100, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, INT32_MAX};
    long keys = 0;
    for (int32_t x : ext)
        for (int32_t w : ext)
            for (int32_t x2 : ext)
                for (int32_t w2 : ext) {
                    uint32_t key = 0;
                    const bool ok = track_key(0, x, x2, w, w2, 0, x2, x, w2, w, 0, key);
                    if (ok && key > 65536u) {
                        fprintf(stderr, "key %u out of range\n", key);
                        return 1;
                    }
                    fprintf(out, "key %d %d %d %d %d %d %d %d %ld\n", x, x2, w, w2, x2, x, w2, w, ok ? (long)key : -1L);
                    keys += ok;
                }
    fclose(in);
    fclose(out);
    printf("track_check: %ld steps, %ld detections, %ld steps with a NULL due pointer, %ld extreme keys: all checks passed\n",
           steps, dets_total, null_steps, keys);
    return 0;
}
