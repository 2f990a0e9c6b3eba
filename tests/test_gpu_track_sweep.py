"""``evam_pp_track_device_rois`` past the random sequences of ``test_gpu_track.py``, which need two matching rounds at
the most: inputs of 64, 127 and 128 rounds (``track_ref.chain_frames``, ``disjoint_frames``), thresholds 0.0, 1.0 and
NaN with ``max_lost`` 0, 1 and 8, boxes and labels at the ends of int32 with frame indices up to 0xFFFFFFFE, the list
edges the header promises (a count above the cap, entries outside the item range, an empty and a long classify set, a
gate without a due list, due caps around the due count) and grids and item tables larger than a chip and a ring slot.

Every case compares the device with ``HostTracker`` byte for byte (ids, due entries, due count, every slot's state), and
first ``HostTracker`` with ``track_ref.Tracker`` on the same input, whose events (rounds, ties, slot exhaustion) are
asserted before anything runs on the device. No tolerances anywhere."""
import contextlib

import numpy as np
import pytest

import track_ref as R
from track_cases import Host, check_call, check_states, host_against_reference, tracker_with_cfg, upload_call

pytestmark = pytest.mark.gpu

NAN = float("nan")
TYPE_OF = {0: "zero-term-imageless", 8: "short-term-imageless"}  # the public spellings; any other max_lost: a cfg


@contextlib.contextmanager
def session(evam, n_slots, max_lost=8, iou=0.3):
    """``(pp, tracker, host twin)`` on a fresh handle."""
    pp = evam.HipPreProcessor(device=0)
    tracker = None
    try:
        if max_lost in TYPE_OF:
            tracker = evam.DeviceTracker(pp, n_slots, TYPE_OF[max_lost], iou_threshold=iou)
        else:
            tracker = tracker_with_cfg(evam, pp, n_slots, evam.native.EvamTrackCfg(max_lost, iou))
        assert tracker.cfg.max_lost == max_lost
        yield pp, tracker, Host(evam, n_slots, tracker.cfg)
    finally:
        if tracker is not None:
            tracker.close()
        pp.close()


def table(items):
    return [(s, f) for s, f, _, _ in items]


def run_call(evam, gpu, sess, items, classify, reclassify, what, due_cap=None):
    """One call on the host twin and on the device, compared. Returns the due count."""
    import torch

    pp, tracker, host = sess
    rows, labs, want_ids, want_due = host.call(items, classify, reclassify)
    lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs, due_cap=due_cap)
    pp.track_rois(lst, labels, tracker, table(items), classify, reclassify, ids, due)
    return check_call(what, len(rows), want_ids, want_due, ids, due)


def drive(evam, gpu, sess, seqs, fi, chunks, classify, reclassify, slots=None):
    """``seqs`` in calls of ``chunks`` frames per stream, the streams in another order in every call."""
    n = len(seqs)
    slots = list(range(n)) if slots is None else slots
    assert sum(chunks) == len(seqs[0])
    f0 = 0
    for c, nf in enumerate(chunks):
        order = list(range(n))[::-1] if c % 2 else list(range(n))
        order = order[c % n:] + order[:c % n]
        items = [(slots[s], fi[s][f], *seqs[s][f]) for s in order for f in range(f0, f0 + nf)]
        f0 += nf
        run_call(evam, gpu, sess, items, classify, reclassify, f"call {c}")
    check_states(evam, sess[0], sess[1], sess[2], "after the last call")


# ---- long rounds ----

def long_input(kind):
    """``(frames of one stream, iou_threshold, the rounds the second frame needs)``."""
    if kind == "chain":
        return R.chain_frames(128, seed=11)[0], 0.3, 128
    if kind in ("chain127+12", "chain128+12"):
        n = int(kind[5:8])
        frames, _ = R.chain_frames(n, seed=n)
        extra = R.far_rows(12)
        frames[1] = (np.concatenate([frames[1][0], extra[0]]), np.concatenate([frames[1][1], extra[1]]))
        return frames, 0.3, n
    if kind == "disjoint":
        return R.disjoint_frames(128), 0.0, 128
    assert kind == "two-labels"
    return R.two_label_chain_frames(64, seed=5)[0], 0.3, 64


@pytest.mark.parametrize("kind,calls", [("chain", 1), ("chain", 2), ("chain127+12", 2), ("chain128+12", 1),
                                        ("disjoint", 1), ("two-labels", 2)])
def test_long_rounds(evam, gpu, kind, calls):
    frames, iou, rounds = long_input(kind)
    fi = [[3, 4]]
    want, ev = host_against_reference(evam, [frames], fi, 8, iou, "all", 2)
    assert ev.rounds >= rounds, f"{kind}: the reference needed {ev.rounds} rounds"
    if "+12" in kind:  # past D: the detections from index 128 on take no part
        assert ev.over_d == 1 and want[0][1][0][128:] == [0] * (len(frames[1][0]) - 128)
    with session(evam, 2, 8, iou) as sess:
        drive(evam, gpu, sess, [frames], fi, [2] if calls == 1 else [1, 1], "all", 2, slots=[1])


# ---- thresholds and ageing ----

def sweep_input(kind):
    if kind == "random":
        seqs = R.random_sequences(14, 3, 12)
        return seqs, [[5 * f for f in range(12)]] * 3
    return R.extreme_sequences(23, 3, 12)


@pytest.mark.parametrize("max_lost", [0, 1, 8])
@pytest.mark.parametrize("iou", [0.0, 1.0, NAN])
@pytest.mark.parametrize("kind", ["random", "extreme"])
def test_thresholds_and_ageing(evam, gpu, kind, iou, max_lost):
    seqs, fi = sweep_input(kind)
    _, ev = host_against_reference(evam, seqs, fi, max_lost, iou, "all", 3)
    assert ev.ties > 0 and ev.over_d > 0, vars(ev)
    if max_lost:
        assert ev.exhausted > 0, "the slots never ran out"
    with session(evam, 4, max_lost, iou) as sess:
        drive(evam, gpu, sess, seqs, fi, [2, 3, 7], "all", 3, slots=[2, 0, 3])


# ---- extremes ----

@pytest.mark.parametrize("reclassify", [1, 3, 2**31 - 1])
@pytest.mark.parametrize("classify", ["all", [-2**31, 0]], ids=["all", "min-and-0"])
def test_extreme_boxes_labels_and_frames(evam, gpu, classify, reclassify):
    seqs, fi = R.extreme_sequences(23, 3, 12)
    assert all(f[-1] == R.LAST_FRAME for f in fi)
    want, ev = host_against_reference(evam, seqs, fi, 8, 0.3, classify, reclassify)
    assert ev.ties > 0 and ev.exhausted > 0 and ev.over_d > 0, vars(ev)
    due = [d for frames in want for _, flags in frames for d in flags]
    assert any(due) and all(due) == (classify == "all" and reclassify == 1)   # interval 1: every entry, every frame
    with session(evam, 3) as sess:
        drive(evam, gpu, sess, seqs, fi, [1, 4, 2, 5], classify, reclassify)


# ---- list edges ----

def small_calls(n_streams=3, n_frames=6, per_call=3, seed=14):
    """``random_sequences`` as calls of ``per_call`` frames per stream: ``[items]``."""
    seqs = R.random_sequences(seed, n_streams, n_frames, max_boxes=40)
    return [[(s, f, *seqs[s][f]) for s in range(n_streams) for f in range(f0, f0 + per_call)]
            for f0 in range(0, n_frames, per_call)]


@pytest.mark.parametrize("count", ["rows", "uint32-max"])
def test_count_above_cap(evam, gpu, count):
    """``*list->count > list->cap``: the first ``cap`` rows are the list, and the cut falls inside an item."""
    import torch

    with session(evam, 3) as (pp, tracker, host):
        for c, items in enumerate(small_calls()):
            full = np.concatenate([np.full(len(b), i, np.int32) for i, (_, _, b, _) in enumerate(items)])
            cap = next(k for k in range(len(full) * 2 // 3, 0, -1) if full[k - 1] == full[k] and full[k] < len(items) - 2)
            cut, left = [], cap
            for s, f, b, lab in items:  # what the device may see: the items behind the cut are steps with no detections
                cut.append((s, f, b[:left], lab[:left]))
                left -= len(cut[-1][2])
            assert left == 0 and any(0 < len(k[2]) < len(i[2]) for k, i in zip(cut, items))
            rows, labs, want_ids, want_due = host.call(cut, "all", 2)
            assert len(rows) == cap
            lst, labels, ids, due = upload_call(evam, torch, gpu, rows, labs, cap=cap)
            lst.count.fill_(len(full) if count == "rows" else -1)   # the bits of a uint32
            pp.track_rois(lst, labels, tracker, table(items), "all", 2, ids, due)
            assert check_call(f"call {c}", cap, want_ids, want_due, ids, due) > 0
        check_states(evam, pp, tracker, host, "count above cap")


def test_entries_outside_the_item_range(evam, gpu):
    """Entries with ``src_index`` -1 in front of the first item and ``n_items``, ``n_items + 5`` behind the last get id
    0 and no due entry, and the others what they get without them (the host twin never sees them)."""
    import torch

    with session(evam, 3) as (pp, tracker, host):
        for c, items in enumerate(small_calls()):
            rows, labs, want_ids, want_due = host.call(items, "all", 2)
            n = len(items)
            stray = lambda src, k: np.asarray([(src, 10 * j, 10, 50, 50) for j in range(k)], np.int32)  # noqa: E731
            front, back = stray(-1, 3), np.concatenate([stray(n, 2), stray(n + 5, 2)])
            rows2 = np.concatenate([front, rows, back])
            labs2 = np.concatenate([np.zeros(3, np.int32), labs, np.zeros(4, np.int32)])
            ids2 = np.concatenate([np.zeros(3, np.uint32), want_ids, np.zeros(4, np.uint32)])
            lst, labels, ids, due = upload_call(evam, torch, gpu, rows2, labs2)
            pp.track_rois(lst, labels, tracker, table(items), "all", 2, ids, due)
            assert check_call(f"call {c}", len(rows2), ids2, want_due, ids, due) > 0
        check_states(evam, pp, tracker, host, "strays")


# 300 entries over 150 values, so most come twice; labels 0 and 2 are in, label 1 is not
LONG_SET = [int(v) if v != 1 else -1 for v in np.random.default_rng(3).integers(-100, 50, 298)] + [0, 2]


@pytest.mark.parametrize("classify", [[], LONG_SET], ids=["empty-set", "300-labels"])
def test_classify_sets(evam, gpu, classify):
    assert len(classify) in (0, 300) and len(set(classify)) < max(len(classify), 1)
    with session(evam, 3) as sess:
        total = 0
        for c, items in enumerate(small_calls()):
            total += run_call(evam, gpu, sess, items, classify, 2, f"call {c}")
        check_states(evam, sess[0], sess[1], sess[2], "classify set")
        labels = {int(v) for items in small_calls() for it in items for v in it[3]}
        if classify:
            assert total > 0 and labels & set(classify) and labels - set(classify)
        else:  # the gate is on and nothing is due: no slot was classified
            NONE = evam.native.TRACK_NONE
            assert total == 0 and all(s.classified_at == NONE for t in sess[2].trk for s in t.state.slots)


def test_gate_without_a_due_list(evam, gpu):
    """A classify set and ``due == NULL``: ``classified_at`` is set as with a due list, on the device and on the host."""
    import torch

    with session(evam, 3) as (pp, tracker, host):
        for c, items in enumerate(small_calls()):
            rows, labs, want_ids, want_due = host.call(items, [0, 2], 2)
            assert len(want_due)
            lst, labels, ids, _ = upload_call(evam, torch, gpu, rows, labs)
            pp.track_rois(lst, labels, tracker, table(items), [0, 2], 2, ids, None)
            assert np.array_equal(ids.cpu().numpy().view(np.uint32), want_ids), f"call {c}: ids"
        assert any(s.id and s.classified_at != evam.native.TRACK_NONE for t in host.trk for s in t.state.slots)
        check_states(evam, pp, tracker, host, "no due list")


@pytest.mark.parametrize("cap", ["1", "count", "count-1"])
def test_due_cap_around_the_due_count(evam, gpu, cap):
    with session(evam, 3) as sess:
        for c, items in enumerate(small_calls()):
            twin = Host(evam, 3, sess[1].cfg)   # the due count of this call, from a copy of the twin's states
            for a, b in zip(twin.trk, sess[2].trk):
                a.state = type(b.state).from_buffer_copy(b.state)
            count = len(twin.call(items, "all", 2)[3])
            assert count > 2
            due_cap = {"1": 1, "count": count, "count-1": count - 1}[cap]
            assert run_call(evam, gpu, sess, items, "all", 2, f"call {c}", due_cap=due_cap) == count
        check_states(evam, sess[0], sess[1], sess[2], "due cap")


# ---- grid and table size ----

def little_frames(rng, n_frames, empty_every=0):
    """Frames of 2..5 boxes that drift a few pixels; every ``empty_every``-th is empty."""
    k = int(rng.integers(2, 6))
    base = np.stack([rng.integers(0, 1800, k), rng.integers(0, 1000, k), rng.integers(20, 90, k), rng.integers(20, 90, k)],
                    axis=1).astype(np.int32)
    labels = rng.integers(0, 3, k).astype(np.int32)
    frames = []
    for f in range(n_frames):
        if empty_every and f % empty_every == empty_every - 1:
            frames.append((np.zeros((0, 4), np.int32), np.zeros(0, np.int32)))
            continue
        shown = rng.random(k) > 0.15
        base[:, :2] += rng.integers(-3, 4, (k, 2)).astype(np.int32)
        frames.append((base[shown].copy(), labels[shown].copy()))
    return frames


def test_more_workgroups_than_cus(evam, gpu):
    """300 stream slots of a 320-slot tracker in one call (one workgroup each, one per CU by its LDS), named in a
    scrambled order, two calls; the 20 slots never named stay fresh."""
    import torch

    assert 300 > torch.cuda.get_device_properties(gpu).multi_processor_count
    rng = np.random.default_rng(31)
    slots = [int(s) for s in rng.permutation(320)[:300]]
    seqs = [little_frames(rng, 2 + s % 2) for s in range(300)]   # two or three frames: one or two in the first call
    fi = [list(range(len(frames))) for frames in seqs]
    host_against_reference(evam, seqs, fi, 8, 0.3, "all", 2)
    with session(evam, 320) as sess:
        for c in range(2):
            order = rng.permutation(300)
            items = [(slots[s], f, *seqs[s][f]) for s in order
                     for f in (range(len(seqs[s]) - 1) if c == 0 else [len(seqs[s]) - 1])]
            run_call(evam, gpu, sess, items, "all", 2, f"call {c}")
        check_states(evam, sess[0], sess[1], sess[2], "300 slots")
        fresh = sess[2].state_bytes(next(s for s in range(320) if s not in slots))
        for s in set(range(320)) - set(slots):
            assert bytes(sess[1].read_state(sess[0], s)) == fresh and sess[2].trk[s].state.next_id == 0


def test_one_stream_300_items(evam, gpu):
    rng = np.random.default_rng(32)
    frames = little_frames(rng, 300, empty_every=3)
    fi = [[7 * f for f in range(300)]]
    assert sum(len(b) == 0 for b, _ in frames) >= 100
    host_against_reference(evam, [frames], fi, 8, 0.3, [0, 1], 5)
    with session(evam, 1) as sess:
        items = [(0, fi[0][f], *frames[f]) for f in range(300)]
        assert run_call(evam, gpu, sess, items, [0, 1], 5, "300 items") > 0
        check_states(evam, sess[0], sess[1], sess[2], "300 items")


def test_item_table_past_a_ring_slot(evam, gpu):
    """A call of 9,000 items (a 72,000-byte item table; a descriptor ring slot starts at 64 KiB) behind three small
    calls, which fill the ring's three slots, and in front of another, with no host synchronisation in between: the
    large block goes into a slot that is reallocated while the earlier calls are in flight. HostTracker against the
    device only: test_track_host.py pins HostTracker to the reference on the same rule."""
    import torch

    rng = np.random.default_rng(33)
    n_slots, per = 300, 30
    assert n_slots * per * 8 > 64 * 1024
    seqs = [little_frames(rng, per + 4, empty_every=0) for _ in range(n_slots)]
    empty = (np.zeros((0, 4), np.int32), np.zeros(0, np.int32))
    with session(evam, n_slots) as (pp, tracker, host):
        small = lambda j, f, k: [(s, f, *seqs[s][j]) for s in range(k)]  # noqa: E731
        big = [(s, 10 + f, *(seqs[s][3 + f] if (s + f) % 10 == 0 else empty)) for s in range(n_slots) for f in range(per)]
        calls = []
        for items in (small(0, 0, 2), small(1, 1, 3), small(2, 2, 4), big, small(per + 3, 50, 5)):
            rows, labs, want_ids, want_due = host.call(items, "all", 4)
            calls.append((items, len(rows), want_ids, want_due, upload_call(evam, torch, gpu, rows, labs)))
        assert len(calls[3][0]) == 9000 and 1000 < calls[3][1] < 4000
        torch.cuda.synchronize()  # the inputs are in place; from here on the host waits for nothing of its own accord
        for items, _, _, _, (lst, labels, ids, due) in calls:
            pp.track_rois(lst, labels, tracker, table(items), "all", 4, ids, due)
        torch.cuda.synchronize()
        for c, (_, n, want_ids, want_due, (_, _, ids, due)) in enumerate(calls):
            check_call(f"call {c}", n, want_ids, want_due, ids, due)
        check_states(evam, pp, tracker, host, "9,000 items")
