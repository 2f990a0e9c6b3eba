"""``evam_pp_track_host`` (the gvatrack rule on host arrays, no GPU) against ``tests/track_ref.py``: ids, due flags and
the state after every step are equal, on hand-written cases and on seeded random sequences whose preconditions (ties,
slot exhaustion, frames past D detections, long-lived ids, slots reborn) are asserted on the reference alone.

Two of the preconditions depend on ``max_lost`` and are asserted only where they can hold: slot exhaustion needs
``max_lost`` > 0 (with 0 every unmatched track is freed before the births, so D <= T detections always fit; that sweep
asserts a slot freed and refilled in one step instead), and an id that survives 10 frames is asserted for ``max_lost``
8 only: the sweeps with ``max_lost`` 0 and 2 (seeds 2 and 3) do not check longevity.

Further: the inputs that need as many matching rounds as there are tracks (``track_ref.chain_frames``,
``disjoint_frames`` at threshold 0.0), sequences of extreme boxes, labels and frame indices at thresholds 0.0, 0.3, 1.0,
NaN and 2.0 with ``max_lost`` 0, 1 and 8, and the gate with a NULL due array."""
import numpy as np
import pytest

import track_ref as R
from track_cases import host_against_reference as run_host_against_reference


def both(evam, max_lost=8, iou=0.3):
    cfg = evam.native.EvamTrackCfg(max_lost, iou)
    return evam.native.HostTracker(cfg=cfg), R.Tracker(max_lost, iou)


def step_both(evam, host, ref, fi, boxes, labels, classify=None, reclassify=1):
    """One step on both; asserts ids, due and state equal; returns (ids, due) of the reference."""
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    ids, due = host.step(fi, boxes, labels, classify, reclassify)
    rids, rdue = ref.step(fi, boxes, labels, classify, reclassify)
    assert ids.tolist() == rids, (fi, ids.tolist(), rids)
    assert due.tolist() == rdue, (fi, due.tolist(), rdue)
    assert evam.native.track_state_tuple(host.state) == ref.state(), fi
    return rids, rdue


def test_two_boxes_crossing(evam):
    host, ref = both(evam)
    seen = []
    for f in range(12):
        a = (100 + 20 * f, 100, 80, 80)   # moves right
        b = (320 - 20 * f, 110, 80, 80)   # moves left, through a
        seen.append(step_both(evam, host, ref, f, [a, b], [1, 1])[0])
    assert seen[0] == [1, 2]
    assert all(sorted(s) == [1, 2] for s in seen)  # no id is lost or born while they cross


def test_equal_keys_slot_then_detection(evam):
    host, ref = both(evam)
    box = (10, 10, 50, 50)
    assert step_both(evam, host, ref, 0, [box, box], [0, 0])[0] == [1, 2]      # two tracks on one box
    # one detection, two tracks with key 65536: the lower slot (id 1) takes it; the other ages
    assert step_both(evam, host, ref, 1, [box], [0])[0] == [1]
    # two equal detections, both tracks: (slot 0, det 0) first, then (slot 1, det 1)
    assert step_both(evam, host, ref, 2, [box, box], [0, 0])[0] == [1, 2]
    # equal keys across detections for one track: the lower detection index wins
    host, ref = both(evam)
    step_both(evam, host, ref, 0, [(100, 100, 40, 40)], [0])
    left, right = (90, 100, 40, 40), (110, 100, 40, 40)
    assert R.pair_key((100, 100, 40, 40), left) == R.pair_key((100, 100, 40, 40), right)
    assert step_both(evam, host, ref, 1, [left, right], [0, 0])[0] == [1, 2]
    assert step_both(evam, host, ref, 2, [(100, 100, 40, 40), left], [0, 0])[0] == [2, 1]


def test_duplicate_boxes(evam):
    host, ref = both(evam)
    box = (5, 5, 30, 30)
    assert step_both(evam, host, ref, 0, [box] * 4, [2] * 4)[0] == [1, 2, 3, 4]
    assert step_both(evam, host, ref, 1, [box] * 4, [2] * 4)[0] == [1, 2, 3, 4]
    assert step_both(evam, host, ref, 2, [box] * 5, [2] * 5)[0] == [1, 2, 3, 4, 5]


def test_label_change_breaks_track(evam):
    host, ref = both(evam, max_lost=0)
    box = (40, 40, 60, 60)
    assert step_both(evam, host, ref, 0, [box], [1])[0] == [1]
    assert step_both(evam, host, ref, 1, [box], [2])[0] == [2]   # same box, other label: a new object
    assert step_both(evam, host, ref, 2, [box], [2])[0] == [2]


@pytest.mark.parametrize("max_lost", [0, 8])
def test_max_lost(evam, max_lost):
    host, ref = both(evam, max_lost=max_lost)
    box = (40, 40, 60, 60)
    assert step_both(evam, host, ref, 0, [box], [0])[0] == [1]
    for f in range(1, max_lost + 1):   # missed max_lost frames: still alive
        step_both(evam, host, ref, f, [], [])
    assert step_both(evam, host, ref, max_lost + 1, [box], [0])[0] == [1]
    for f in range(max_lost + 2, 2 * max_lost + 3):   # missed max_lost + 1 frames: gone
        step_both(evam, host, ref, f, [], [])
    assert step_both(evam, host, ref, 2 * max_lost + 3, [box], [0])[0] == [2]


def grid(n, step=40, size=30):
    return [((i % 40) * step, (i // 40) * step, size, size) for i in range(n)]


def test_more_detections_than_d(evam):
    host, ref = both(evam)
    for f in range(3):
        ids, due = step_both(evam, host, ref, f, grid(140), [0] * 140, "all", 2)
        assert ids[:128] == list(range(1, 129)) and ids[128:] == [0] * 12
        assert due[128:] == [True] * 12              # untracked: classified on every frame
        assert due[:128] == [f != 1] * 128


def test_more_live_tracks_than_t(evam):
    host, ref = both(evam)
    step_both(evam, host, ref, 0, grid(100), [0] * 100)
    # 100 tracks age (max_lost 8), 60 other boxes arrive: 28 find a slot, 32 find none
    far = [(x, y + 2000, w, h) for x, y, w, h in grid(60)]
    ids, _ = step_both(evam, host, ref, 1, far, [0] * 60)
    assert ids == list(range(101, 129)) + [0] * 32
    ids, _ = step_both(evam, host, ref, 2, far, [0] * 60)
    assert ids == list(range(101, 129)) + [0] * 32   # every slot is still taken
    assert host.state.next_id == 129


def test_slot_freed_and_refilled_in_one_step(evam):
    host, ref = both(evam, max_lost=0)
    assert step_both(evam, host, ref, 0, [(0, 0, 20, 20), (100, 0, 20, 20)], [0, 0])[0] == [1, 2]
    # track 1 (slot 0) is not matched: freed in step 5, and the new box takes slot 0 in step 6 of the same step
    assert step_both(evam, host, ref, 1, [(500, 500, 20, 20), (100, 0, 20, 20)], [0, 0])[0] == [3, 2]
    assert host.state.slots[0].id == 3 and host.state.slots[1].id == 2


@pytest.mark.parametrize("reclassify", [1, 3, 7])
def test_reclassify_interval(evam, reclassify):
    host, ref = both(evam)
    box, other = (40, 40, 60, 60), (400, 40, 60, 60)
    for f in range(16):
        _, due = step_both(evam, host, ref, f, [box, other], [1, 5], [1], reclassify)
        assert due == [f % reclassify == 0, False]   # label 5 is not in the set


def test_no_gate_and_arguments(evam):
    N = evam.native
    host, ref = both(evam)
    _, due = step_both(evam, host, ref, 0, [(0, 0, 9, 9)], [0])
    assert due == [False] and host.state.slots[0].classified_at == N.TRACK_NONE
    lib = evam.load_library()
    st, cfg = N.EvamTrackState(), N.EvamTrackCfg(-1, 0.3)
    assert lib.evam_pp_track_host(st, cfg, 0, None, None, 0, None, 0, 1, None, None) == N.ERR_INVALID_ARG
    cfg = N.EvamTrackCfg(8, 0.3)
    assert lib.evam_pp_track_host(st, cfg, 0, None, None, 0, None, 0, 0, None, None) == N.ERR_INVALID_ARG  # reclassify 0
    assert lib.evam_pp_track_host(st, cfg, 0, None, None, 1, None, 0, 1, None, None) == N.ERR_INVALID_ARG  # NULL arrays
    assert lib.evam_pp_track_host(st, cfg, 0, None, None, 0, None, 0, 1, None, None) == N.OK
    for kind in ("zero-term", "short-term"):
        with pytest.raises(N.PreProcError) as e:
            N.track_cfg(kind)
        assert e.value.status == N.ERR_UNSUPPORTED
    assert N.track_cfg("zero-term-imageless").max_lost == 0 and N.track_cfg(None).max_lost == 8


@pytest.mark.parametrize("seed,max_lost,classify,reclassify", [(1, 8, "all", 4), (2, 0, [1], 3), (3, 2, None, 1)])
def test_random_sequences(evam, seed, max_lost, classify, reclassify):
    seqs = R.random_sequences(seed)   # 8 streams x 40 frames, 0..140 boxes, 3 labels
    assert len(seqs) == 8 and all(len(fr) == 40 for fr in seqs)
    want, states, ev = R.run_reference(seqs, max_lost, 0.3, classify, reclassify)
    # the preconditions, on the reference alone: a sweep that never reaches them shows nothing
    R.assert_events(ev, max_lost)
    cfg = evam.native.EvamTrackCfg(max_lost, 0.3)
    for s, frames in enumerate(seqs):
        host = evam.native.HostTracker(cfg=cfg)
        for f, (boxes, labels) in enumerate(frames):
            ids, due = host.step(f, boxes, labels, classify, reclassify)
            assert ids.tolist() == want[s][f][0], (s, f)
            assert due.tolist() == want[s][f][1], (s, f)
        assert evam.native.track_state_tuple(host.state) == states[s], s


def test_null_due_runs_the_gate(evam):
    """``evam_pp_track_host`` with a classify set and ``due == NULL``: ``classified_at`` is state, so the gate runs as
    it does with a due array (and as the kernel runs it with no due list)."""
    N, lib = evam.native, evam.load_library()
    cfg = N.EvamTrackCfg(8, 0.3)
    with_due, ref = both(evam)
    st = N.EvamTrackState()
    boxes = [(40, 40, 60, 60), (400, 40, 60, 60), (800, 40, 60, 60)]
    labels = np.asarray([1, 5, 2], np.int32)
    classify = np.asarray([1, 2], np.int32)
    for fi in (7, 8, 11, 12, 40):
        step_both(evam, with_due, ref, fi, boxes, labels, [1, 2], 4)
        rois = np.zeros((3, 5), np.int32)
        rois[:, 1:] = boxes
        ids = np.zeros(3, np.uint32)
        assert lib.evam_pp_track_host(st, cfg, fi, rois.ctypes.data, labels.ctypes.data, 3, classify.ctypes.data, 2, 4,
                                      ids.ctypes.data, None) == N.OK
        assert ids.tolist() == [1, 2, 3]
        assert N.track_state_tuple(st) == ref.state(), fi
        assert bytes(st) == bytes(with_due.state), fi
    assert [s[7] for s in ref.state()[1][:3]] == [40, N.TRACK_NONE, 40]   # due at 7, 11 and 40; label 5 never


@pytest.mark.parametrize("n,max_lost", [(128, 8), (127, 1), (128, 0)])
def test_chain_needs_n_rounds(evam, n, max_lost):
    frames, ids = R.chain_frames(n, seed=n + max_lost)
    assert ids != sorted(ids), "the permutation left the chain in slot order"
    want, ev = run_host_against_reference(evam, [frames], [[3, 4]], max_lost, 0.3, "all", 2)
    assert ev.rounds >= n, ev.rounds   # one match per round
    assert want[0][0][0] == list(range(1, n + 1)) and want[0][1][0] == ids


def test_two_label_chain(evam):
    frames, ids = R.two_label_chain_frames(64, seed=5)
    want, ev = run_host_against_reference(evam, [frames], [[0, 1]], 8, 0.3, [1], 1)
    assert ev.rounds >= 64, ev.rounds
    assert want[0][1][0] == ids


@pytest.mark.parametrize("max_lost", [0, 1, 8])
def test_disjoint_grid_at_threshold_zero(evam, max_lost):
    frames = R.disjoint_frames(128)
    want, ev = run_host_against_reference(evam, [frames], [[0, 1]], max_lost, 0.0, None, 1)
    assert ev.rounds >= 128 and ev.ties > 0, (ev.rounds, ev.ties)
    assert want[0][1][0] == list(range(1, 129))   # every key is 0: lowest slot, then lowest detection
    # at the default threshold no pair of the same input is a candidate
    want, ev = run_host_against_reference(evam, [frames], [[0, 1]], 8, 0.3, None, 1)
    assert ev.rounds == 0 and want[0][1][0] == [0] * 128


@pytest.mark.parametrize("max_lost", [0, 1, 8])
@pytest.mark.parametrize("iou", [0.0, 0.3, 1.0, float("nan"), 2.0])
def test_extreme_sequences(evam, iou, max_lost):
    """Boxes and labels at the ends of int32, sides around the 2^20 clamp, frame indices up to 0xFFFFFFFE."""
    seqs, fi = R.extreme_sequences(21, 2, 30)
    assert all(f[-1] == R.LAST_FRAME for f in fi)
    classify, reclassify = ("all", 3) if max_lost != 1 else ([-2**31, 0], 2**31 - 1)
    _, ev = run_host_against_reference(evam, seqs, fi, max_lost, iou, classify, reclassify)
    assert ev.ties > 0 and ev.over_d > 0, vars(ev)
    if max_lost:
        assert ev.exhausted > 0
    if iou != iou or iou >= 1.0:
        assert R.thr_key(iou) == 65536


def test_gpu_sequences_reach_the_events():
    """The sequences of ``test_gpu_track.py::test_track_device_equals_host``, on the reference alone: the events
    ``test_random_sequences`` asks of its own seeds. Also what makes the chain inputs necessary: no frame of the random
    sequences, these or the host sweep's, needs more than two matching rounds."""
    from track_cases import SEQ_SEEDS

    for n_streams, seed in SEQ_SEEDS.items():
        ev = R.run_reference(R.random_sequences(seed, n_streams, 16), 8, 0.3)[2]
        R.assert_events(ev, 8)
        assert 1 <= ev.rounds <= 2, (seed, ev.rounds)
    assert R.run_reference(R.random_sequences(1), 8, 0.3)[2].rounds == 2
