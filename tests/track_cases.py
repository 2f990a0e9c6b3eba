"""What the GPU tracker tests share (``test_gpu_track.py``, ``test_gpu_track_sweep.py``): the host twin of a
DeviceTracker, the upload of one call's list, and the byte comparisons of ids, due list and states."""
import ctypes

import numpy as np

import track_ref as R

SENTINEL = -3
# random_sequences seeds of test_gpu_track.py by stream count, 16 frames each: every one reaches the events
# track_ref.assert_events names (11 + n_streams, but for one stream: seed 12 has no frame past D detections)
SEQ_SEEDS = {1: 14, 3: 14, 8: 19}


class Host:
    """The host twin of a DeviceTracker: one HostTracker per stream slot."""

    def __init__(self, evam, n_slots, cfg):
        self.evam, self.cfg = evam, cfg
        self.trk = [evam.native.HostTracker(cfg=cfg) for _ in range(n_slots)]

    def call(self, items, classify, reclassify):
        """items: [(slot, frame, boxes, labels)] in table order -> (list rows [n, 5], labels, ids, due rows)."""
        rows, labs, ids, due = [], [], [], []
        for i, (slot, frame, boxes, labels) in enumerate(items):
            a, d = self.trk[slot].step(frame, boxes, labels, classify, reclassify)
            r = np.concatenate([np.full((len(boxes), 1), i, np.int32), np.asarray(boxes, np.int32).reshape(-1, 4)], axis=1)
            rows.append(r)
            labs.append(np.asarray(labels, np.int32).reshape(-1))
            ids.append(a)
            due.append(r[d])
        cat = lambda v, shape: np.concatenate(v) if v else np.zeros(shape, np.int32)  # noqa: E731
        return cat(rows, (0, 5)), cat(labs, (0,)), cat(ids, (0,)).astype(np.uint32), cat(due, (0, 5))

    def state_bytes(self, slot):
        st = self.trk[slot].state
        if st.next_id == 0:  # never stepped: the fresh state zeroed memory stands for
            st = self.evam.native.EvamTrackState()
            st.next_id = 1
            for s in st.slots:
                s.classified_at = self.evam.native.TRACK_NONE
        return bytes(st)


def upload_call(evam, torch, gpu, rows, labs, cap=None, due_cap=None):
    cap = max(len(rows), 1) if cap is None else cap
    lst = evam.DeviceRoiList(cap, device=gpu)
    lst.rois.fill_(SENTINEL)
    lst.set(rows)
    labels = torch.full((cap,), SENTINEL, dtype=torch.int32, device=gpu)
    if len(labs):
        labels[:len(labs)].copy_(torch.from_numpy(labs))
    ids = torch.full((cap,), SENTINEL, dtype=torch.int32, device=gpu)
    due = evam.DeviceRoiList(max(len(rows), 1) if due_cap is None else due_cap, device=gpu)
    due.rois.fill_(SENTINEL)
    due.count.fill_(-1)
    return lst, labels, ids, due


def check_call(what, n, want_ids, want_due, ids, due):
    got = ids.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n], want_ids), f"{what}: ids"
    assert (got[n:] == 0).all(), f"{what}: ids past the count are 0"
    count = int(due.count.cpu().numpy().view(np.uint32)[0])
    assert count == len(want_due), f"{what}: due count {count}, host {len(want_due)}"
    m = min(count, due.cap)
    rois = due.rois.cpu().numpy()
    assert np.array_equal(rois[:m], want_due[:m]), f"{what}: due entries"
    assert (rois[m:] == SENTINEL).all(), f"{what}: due entries past the count were written"
    return count


def check_states(evam, pp, tracker, host, what):
    for slot in range(tracker.n_streams):
        assert bytes(tracker.read_state(pp, slot)) == host.state_bytes(slot), f"{what}: state of slot {slot}"


def tracker_with_cfg(evam, pp, n_streams, cfg):
    """A DeviceTracker over ``evam_pp_tracker_create`` with any ``EvamTrackCfg``: the two ``tracking-type`` strings are
    the only public spellings, and they carry ``max_lost`` 0 and 8 alone."""
    lib = evam.load_library()
    t = ctypes.c_void_p()
    pp._bind_stream()
    evam.native.check(lib, lib.evam_pp_tracker_create(pp._h, int(n_streams), ctypes.byref(cfg), ctypes.byref(t)))
    tracker = object.__new__(evam.DeviceTracker)
    tracker.cfg, tracker._lib, tracker.n_streams, tracker.device, tracker._t = cfg, lib, int(n_streams), pp.device, t
    return tracker


def host_against_reference(evam, seqs, frame_indices, max_lost, iou, classify, reclassify):
    """``HostTracker`` against ``track_ref.Tracker`` step by step on ``seqs`` (per stream, per frame ``(boxes,
    labels)``): ids, due flags and final states. Returns the reference's ``(results, Events)``."""
    want, states, ev = R.run_reference(seqs, max_lost, iou, classify, reclassify, frame_indices=frame_indices)
    cfg = evam.native.EvamTrackCfg(max_lost, iou)
    for s, frames in enumerate(seqs):
        host = evam.native.HostTracker(cfg=cfg)
        for f, (boxes, labels) in enumerate(frames):
            ids, due = host.step(frame_indices[s][f], boxes, labels, classify, reclassify)
            assert ids.tolist() == want[s][f][0], (s, f)
            assert due.tolist() == want[s][f][1], (s, f)
        assert evam.native.track_state_tuple(host.state) == states[s], s
    return want, ev
