"""``evam_pp_track_device_rois`` (the ``evam_pp_track`` kernel, its due-list compaction, the tracker object) on the
GPU, byte for byte against ``evam_pp_track_host`` on the same inputs: the ids, the due list's entries, order and count,
and every stream's state after the last call. Frames hold 0..140 boxes; a call holds 1..16 frames of 1..8 streams."""
import numpy as np
import pytest

import device_rois_cases as C
import track_ref as R
from track_cases import SENTINEL, SEQ_SEEDS, Host, check_call, check_states, upload_call

pytestmark = pytest.mark.gpu


def grid(n, dx=0, step=40, size=30):
    a = np.asarray([((i % 40) * step + dx, (i // 40) * step, size, size) for i in range(n)], np.int32).reshape(-1, 4)
    return a, (np.arange(n, dtype=np.int32) % 3)


@pytest.mark.parametrize("n_streams,chunks,classify,reclassify,due_cap",
                         [(1, [16], "all", 4, None), (3, [1, 2, 5, 8], [0, 2], 3, 5), (8, [4, 4, 8], "all", 2, None),
                          (3, [3, 13], None, 1, None)])
def test_track_device_equals_host(evam, gpu, n_streams, chunks, classify, reclassify, due_cap):
    import torch

    seqs = R.random_sequences(SEQ_SEEDS[n_streams], n_streams, sum(chunks))
    R.assert_events(R.run_reference(seqs, 8, 0.3)[2], 8)  # on the reference alone: what these sequences reach
    n_slots = n_streams + 2
    slots = [(3 * s + 1) % n_slots for s in range(n_streams)]  # 8 streams: 1 4 7 0 3 6 9 2 — not monotone
    assert len(set(slots)) == n_streams
    pp = evam.HipPreProcessor(device=0)
    tracker = evam.DeviceTracker(pp, n_slots, "short-term-imageless")
    host = Host(evam, n_slots, tracker.cfg)
    try:
        f0, total_due, over_cap = 0, 0, 0
        for c, nf in enumerate(chunks):
            order = list(range(n_streams))[::-1] if c % 2 else list(range(n_streams))
            order = order[c % n_streams:] + order[:c % n_streams]
            items = [(slots[s], 2 * f, *seqs[s][f]) for s in order for f in range(f0, f0 + nf)]  # frame indices 0, 2, 4 ..
            f0 += nf
            rows, labs, want_ids, want_due = host.call(items, classify, reclassify)
            lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs, due_cap=due_cap)
            got = pp.track_rois(lst, labels, tracker, [(s, f) for s, f, _, _ in items], classify, reclassify, ids, due)
            assert got is ids
            count = check_call(f"call {c}", len(rows), want_ids, want_due, ids, due)
            total_due += count
            over_cap += count > due.cap
        check_states(evam, pp, tracker, host, "after the last call")  # classified_at of entries past the cap included
        if classify is not None:
            assert total_due > 0
        if due_cap is not None:
            assert over_cap, "the case was meant to overflow the due list"
    finally:
        tracker.close()
        pp.close()


def test_detection_counts_and_empty_frames(evam, gpu):
    """Frames of 0, 1, 127, 128, 129 and 140 detections, twice over, in one call each; max_lost 0."""
    import torch

    pp = evam.HipPreProcessor(device=0)
    tracker = evam.DeviceTracker(pp, 1, "zero-term-imageless")
    host = Host(evam, 1, tracker.cfg)
    try:
        counts = [0, 1, 127, 128, 129, 140, 140, 129, 0, 0, 128, 127, 1]
        for c in range(2):
            items = [(0, c * 100 + f, *grid(n, dx=2 * f)) for f, n in enumerate(counts)]
            rows, labs, want_ids, want_due = host.call(items, [0, 1], 3)
            assert (want_ids == 0).any() and (want_ids != 0).any()
            lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs)
            pp.track_rois(lst, labels, tracker, [(s, f) for s, f, _, _ in items], [0, 1], 3, ids, due)
            check_call(f"call {c}", len(rows), want_ids, want_due, ids, due)
        check_states(evam, pp, tracker, host, "counts")
        # a call whose list is empty: every item is a step with no detections
        rows, labs, want_ids, want_due = host.call([(0, 300, *grid(0)), (0, 301, *grid(0))], "all", 1)
        lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs)
        pp.track_rois(lst, labels, tracker, [(0, 300), (0, 301)], "all", 1, ids, due)
        check_call("empty", 0, want_ids, want_due, ids, due)
        check_states(evam, pp, tracker, host, "empty")
    finally:
        tracker.close()
        pp.close()


def test_slot_reset_in_mid_sequence(evam, gpu):
    import torch

    pp = evam.HipPreProcessor(device=0)
    tracker = evam.DeviceTracker(pp, 2)
    host = Host(evam, 2, tracker.cfg)
    try:
        for c in range(4):
            if c == 2:  # stream slot 1 ends: ids start again at 1 there, slot 0 goes on
                tracker.reset(pp, 1)
                host.trk[1].reset()
            items = [(s, c, *grid(20 + s, dx=3 * c)) for s in (1, 0)]
            rows, labs, want_ids, want_due = host.call(items, "all", 2)
            lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs)
            pp.track_rois(lst, labels, tracker, [(s, f) for s, f, _, _ in items], "all", 2, ids, due)
            check_call(f"call {c}", len(rows), want_ids, want_due, ids, due)
            if c == 2:
                assert want_ids[:21].tolist() == list(range(1, 22))
        check_states(evam, pp, tracker, host, "reset")
    finally:
        tracker.close()
        pp.close()


def test_forty_calls_two_handles_no_host_sync(evam, gpu):
    """40 calls on one tracker, alternating two handles on two streams, with no host synchronisation in between: the
    tracker's event orders them on the device."""
    import torch

    seqs = R.random_sequences(5, 3, 40, max_boxes=60)
    streams = [torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)]
    pps = [evam.HipPreProcessor(device=0, stream=s) for s in streams]
    tracker = evam.DeviceTracker(pps[0], 3)
    host = Host(evam, 3, tracker.cfg)
    try:
        calls = []
        for f in range(40):
            items = [(s, f, *seqs[s][f]) for s in (2, 0, 1)]
            rows, labs, want_ids, want_due = host.call(items, "all", 4)
            calls.append((items, len(rows), want_ids, want_due, upload_call(evam, torch, gpu, rows, labs)))
        torch.cuda.synchronize()  # the inputs are in place; from here on the host waits for nothing
        for f, (items, _, _, _, (lst, labels, ids, due)) in enumerate(calls):
            pps[f % 2].track_rois(lst, labels, tracker, [(s, fi) for s, fi, _, _ in items], "all", 4, ids, due)
        torch.cuda.synchronize()
        for f, (_, n, want_ids, want_due, (_, _, ids, due)) in enumerate(calls):
            check_call(f"call {f}", n, want_ids, want_due, ids, due)
        check_states(evam, pps[1], tracker, host, "40 calls")
    finally:
        tracker.close()
        for p in pps:
            p.close()


def test_refusals(evam, gpu):
    import torch

    N = evam.native
    pp = evam.HipPreProcessor(device=0)
    tracker = evam.DeviceTracker(pp, 3)
    try:
        rows, labs = np.zeros((0, 5), np.int32), np.zeros((0,), np.int32)
        lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs)
        for items in ([(0, 0), (1, 0), (0, 1)],     # the items of stream slot 0 are not contiguous
                      [(0, 5), (0, 5)],             # frame indices must ascend
                      [(0, 5), (0, 4)],
                      [(3, 0)], [(-1, 0)],          # a stream slot outside the tracker
                      []):
            with pytest.raises(N.PreProcError) as e:
                pp.track_rois(lst, labels, tracker, items, "all", 1, ids, due)
            assert e.value.status == N.ERR_INVALID_ARG, items
        with pytest.raises(N.PreProcError) as e:
            pp.track_rois(lst, labels, tracker, [(0, 0)], "all", 0, ids, due)
        assert e.value.status == N.ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert (ids.cpu().numpy() == SENTINEL).all(), "a refused call wrote ids"
        for kind in ("zero-term", "short-term"):
            with pytest.raises(N.PreProcError) as e:
                evam.DeviceTracker(pp, 1, kind)
            assert e.value.status == N.ERR_UNSUPPORTED and "image features" in str(e.value)
        # nothing above changed the tracker
        host = Host(evam, 3, tracker.cfg)
        check_states(evam, pp, tracker, host, "refusals")
    finally:
        tracker.close()
        pp.close()


def host_labels(evam, b):
    """The label id of every rect of the host path (device_rois_cases.python_rois), in its order."""
    P, roi_inside = evam.postproc, evam.pipeline_server.roi_inside
    from importlib import import_module

    xfs = None if b.xf is None else import_module(evam.__name__ + ".preproc").Transforms(b.xf)
    out = []
    for i, dets in enumerate(P.parse_ssd_batch(b.det, b.threshold)):
        W, H = b.sizes[i]
        for r in P.detections_to_regions(dets, None if xfs is None else xfs[i], W, H, b.tensor[0], b.tensor[1]):
            if (b.labels is None or r.label_id in b.labels) and roi_inside(r.x, r.y, r.w, r.h, W, H):
                out.append(r.label_id)
    return out


@pytest.mark.parametrize("case", [(3, 10, "mixed", None), (64, 200, "none", None), (5, 300, "mixed", (1, 2, 4))],
                         ids=C.case_id)
def test_out_labels(evam, gpu, case):
    import torch

    n, K, kind, labels = case
    b = C.make_batch(evam, 99 + n, n, K, kind, labels)
    want_rois, count = C.host_rois(evam, b)
    want_labels = host_labels(evam, b)
    assert len(want_labels) == count > 0
    frames = [evam.Image(evam.native.FOURCC_NV12, w, h, []) for w, h in b.sizes]
    det = torch.from_numpy(b.det).to(gpu)
    pp = evam.HipPreProcessor(device=0)
    try:
        outs = []
        for cap in (n * K, max(1, count // 2)):
            for with_labels in (False, True):
                lst = evam.DeviceRoiList(cap, device=gpu)
                lst.rois.fill_(SENTINEL)
                lab = torch.full((cap,), SENTINEL, dtype=torch.int32, device=gpu) if with_labels else None
                pp.detections_to_rois(det, frames, b.xf, b.tensor, b.threshold, b.labels, lst, out_labels=lab)
                torch.cuda.synchronize()
                rois, got = lst.rois.cpu().numpy(), int(lst.count.cpu().numpy().view(np.uint32)[0])
                outs.append((rois.tobytes(), got))
                m = min(count, cap)
                assert got == count and np.array_equal(rois[:m], want_rois[:m])
                if with_labels:
                    g = lab.cpu().numpy()
                    assert g[:m].tolist() == want_labels[:m]
                    assert (g[m:] == SENTINEL).all(), "labels past the count were written"
            assert outs[-1] == outs[-2], "the list bytes differ with out_labels"
    finally:
        pp.close()
