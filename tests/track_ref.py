"""The gvatrack rule in plain Python: the oracle of the tracker tests. Written from the rule's text (the comment in
``include/evam_pp.h``), not from the C++ header; it shares no code with the library.

State per stream: ``next_id`` (from 1) and ``T`` slots ``[id, label, x, y, w, h, lost, classified_at]`` (id 0: free,
``classified_at`` ``NONE``: never classified). Also the inputs the host, sanitizer-side and GPU tests share
(``random_sequences``; ``chain_frames``, ``two_label_chain_frames`` and ``disjoint_frames``, which need as many
matching rounds as there are tracks; ``extreme_sequences`` for the key arithmetic), and the events a sweep must reach
to show anything (``Events``, ``assert_events``). Every step also checks the kernel's claim on the CPU: matching all
mutual row-and-column maxima at once, round after round, gives the greedy matching (``mutual_best_rounds``)."""
import math

import numpy as np

T = 128
D = 128
NONE = 0xFFFFFFFF
SIDE_MAX = 1 << 20
FREE = (0, 0, 0, 0, 0, 0, 0, NONE)


def thr_key(iou_threshold: float) -> int:
    """floor(iou_threshold * 65536) clamped to [0, 65536], the threshold taken as the float32 the C struct carries; NaN
    gives 65536 (only identical boxes match)."""
    v = float(np.float32(iou_threshold)) * 65536.0
    if math.isnan(v) or v >= 65536.0:
        return 65536
    return max(int(math.floor(v)), 0)


def pair_key(t, d):
    """``(inter << 16) // union`` of two (x, y, w, h) boxes, or None when the union is empty."""
    tw, th = min(max(t[2], 0), SIDE_MAX), min(max(t[3], 0), SIDE_MAX)
    dw, dh = min(max(d[2], 0), SIDE_MAX), min(max(d[3], 0), SIDE_MAX)
    iw = max(0, min(t[0] + tw, d[0] + dw) - max(t[0], d[0]))
    ih = max(0, min(t[1] + th, d[1] + dh) - max(t[1], d[1]))
    inter = iw * ih
    union = tw * th + dw * dh - inter
    if union == 0:
        return None
    return (inter << 16) // union


def pair_keys(t, d):
    """``pair_key`` over broadcast int64 arrays ``[..., 4]``; -1 where the union is empty."""
    tw, th = np.clip(t[..., 2], 0, SIDE_MAX), np.clip(t[..., 3], 0, SIDE_MAX)
    dw, dh = np.clip(d[..., 2], 0, SIDE_MAX), np.clip(d[..., 3], 0, SIDE_MAX)
    iw = np.maximum(0, np.minimum(t[..., 0] + tw, d[..., 0] + dw) - np.maximum(t[..., 0], d[..., 0]))
    ih = np.maximum(0, np.minimum(t[..., 1] + th, d[..., 1] + dh) - np.maximum(t[..., 1], d[..., 1]))
    inter = iw * ih
    union = tw * th + dw * dh - inter
    return np.where(union == 0, -1, (inter << 16) // np.maximum(union, 1))


class Events:
    """What a run of the reference met (the preconditions of a sweep)."""

    def __init__(self):
        self.ties = 0            # rounds whose best key was shared by more than one candidate
        self.exhausted = 0       # detections that found no free slot
        self.over_d = 0          # frames with more than D detections
        self.longest = 0         # most frames any id was seen on
        self.reborn = 0          # slots freed by ageing that took a new id in a later (or the same) step
        self.refilled_same = 0   # ... in the same step
        self.rounds = 0          # most mutual-best matching rounds any step needed (mutual_best_rounds)
        self.seen = {}


def assert_events(ev: Events, max_lost: int):
    """The preconditions of a sweep over ``random_sequences``, on the reference alone: a sweep that never reaches them
    shows nothing. Slot exhaustion needs ``max_lost`` > 0 (with 0 every unmatched track is freed before the births, so
    D <= T detections always fit; a slot freed and refilled in one step is asked for instead), and an id that survives
    10 frames is asked for at ``max_lost`` 8 only."""
    assert ev.ties > 0, "no tie between candidates"
    if max_lost:
        assert ev.exhausted > 0, "the slots never ran out"
    else:
        assert ev.refilled_same > 0, "no slot was freed and refilled in one step"
    assert ev.over_d > 0, "no frame with more than D detections"
    assert ev.reborn > 0, "no track was dropped and a new id born in its slot"
    if max_lost == 8:
        assert ev.longest >= 10, "no id survived 10 frames"


def mutual_best_rounds(cand):
    """The matching the kernel's rounds make, restated: ``cand`` is the step's candidate list ``(key, slot, det)``,
    best first. A pass takes every candidate that is the best of its slot and the best of its detection among the
    unmatched; passes repeat until none is left. Returns ``({det: slot}, passes that took something)``."""
    match, rounds, left = {}, 0, cand
    while left:
        seen_t, seen_d, hit_t, hit_d = set(), set(), set(), set()
        for _, t, d in left:  # best first: the first candidate met of a slot / a detection is its best
            if t not in seen_t and d not in seen_d:
                match[d] = t
                hit_t.add(t)
                hit_d.add(d)
            seen_t.add(t)
            seen_d.add(d)
        rounds += 1  # the list's first candidate is always taken
        left = [c for c in left if c[1] not in hit_t and c[2] not in hit_d]
    return match, rounds


class Tracker:
    def __init__(self, max_lost: int = 8, iou_threshold: float = 0.3, events: Events | None = None):
        self.max_lost = int(max_lost)
        self.thr = thr_key(iou_threshold)
        self.next_id = 1
        self.slots = [list(FREE) for _ in range(T)]
        self.ev = events
        self._dropped = set()  # slots freed by ageing and not refilled yet

    def state(self):
        return self.next_id, [tuple(s) for s in self.slots]

    def step(self, fi: int, boxes, labels, classify=None, reclassify: int = 1):
        """One frame. ``boxes``: (x, y, w, h) rows; ``classify``: None (no gate), "all" or a collection of label ids.
        Returns ``(ids, due)`` lists."""
        boxes = [tuple(int(v) for v in b) for b in boxes]
        labels = [int(v) for v in labels]
        n = len(boxes)
        m = min(n, D)
        ev = self.ev
        if ev is not None and n > D:
            ev.over_d += 1
        # 2. candidates: the keys of every (live slot, participating detection) pair at once, in int64
        cand = []
        live = [t for t, s in enumerate(self.slots) if s[0]]
        if live and m:
            tb = np.asarray([self.slots[t][1:6] for t in live], np.int64)          # label, x, y, w, h
            db = np.asarray([(labels[d], *boxes[d]) for d in range(m)], np.int64)
            keys = pair_keys(tb[:, None, 1:], db[None, :, 1:])
            ok = (tb[:, None, 0] == db[None, :, 0]) & (keys >= self.thr)
            cand = [(int(keys[i, d]), live[i], int(d)) for i, d in zip(*np.nonzero(ok))]
        # 3./4. greedy matching: the largest key first, ties by lower slot, then lower detection index; a pair is taken
        # when it is reached with its track and its detection both unmatched (the repeated arg-max, unrolled)
        cand.sort(key=lambda c: (-c[0], c[1], c[2]))
        det_slot = [None] * n
        hit = set()
        for i, (k, t, d) in enumerate(cand):
            if t in hit or det_slot[d] is not None:
                continue
            if ev is not None:
                j = i + 1
                while j < len(cand) and cand[j][0] == k:
                    if cand[j][1] not in hit and det_slot[cand[j][2]] is None:
                        ev.ties += 1
                        break
                    j += 1
            self.slots[t][2:6] = boxes[d]
            self.slots[t][6] = 0
            hit.add(t)
            det_slot[d] = t
        # the kernel's claim, on every step the suite runs: matching all mutual maxima at once, round after round, gives
        # this same matching (the round count is a precondition counter only; the ids come from the walk above)
        by_rounds, rounds = mutual_best_rounds(cand)
        assert by_rounds == {d: t for d, t in enumerate(det_slot) if t is not None}, (fi, "mutual-best rounds differ")
        if ev is not None:
            ev.rounds = max(ev.rounds, rounds)
        # 5. ageing
        freed_now = set()
        for t, s in enumerate(self.slots):
            if s[0] and t not in hit:
                s[6] += 1
                if s[6] > self.max_lost:
                    self.slots[t] = list(FREE)
                    freed_now.add(t)
        self._dropped |= freed_now
        # 6. births
        for d in range(m):
            if det_slot[d] is not None:
                continue
            free = next((t for t, s in enumerate(self.slots) if not s[0]), None)
            if free is None:
                if ev is not None:
                    ev.exhausted += 1
                continue
            self.slots[free] = [self.next_id, labels[d], *boxes[d], 0, NONE]
            self.next_id += 1
            det_slot[d] = free
            if free in self._dropped:
                self._dropped.discard(free)
                if ev is not None:
                    ev.reborn += 1
                    ev.refilled_same += free in freed_now
        # ids and 7. the gate
        ids, due = [], []
        for d in range(n):
            s = self.slots[det_slot[d]] if det_slot[d] is not None else None
            ids.append(s[0] if s else 0)
            is_due = False
            if classify is not None and (classify == "all" or labels[d] in classify):
                is_due = s is None or s[7] == NONE or fi - s[7] >= reclassify
                if is_due and s is not None:
                    s[7] = fi
            due.append(is_due)
        if ev is not None:
            for i in ids:
                if i:
                    ev.seen[i] = ev.seen.get(i, 0) + 1
                    ev.longest = max(ev.longest, ev.seen[i])
        return ids, due


def random_sequences(seed: int, n_streams: int = 8, n_frames: int = 40, max_boxes: int = 140, n_labels: int = 3,
                     size=(1920, 1080)):
    """Per stream, per frame: ``(int32 [n, 4] boxes, int32 [n] labels)``: 0..max_boxes boxes that drift a few pixels,
    appear and vanish; some streams crowded (past T live tracks and D detections), some sparse, frames that are empty,
    exact duplicates (equal keys), and groups that stand still (keys of 65536 shared by duplicates)."""
    rng = np.random.default_rng(seed)
    W, H = size
    out = []
    for s in range(n_streams):
        crowd = max_boxes if s % 3 == 0 else int(rng.integers(3, 60))
        objs = []  # [x, y, w, h, label, vx, vy]
        frames = []
        for f in range(n_frames):
            target = 0 if rng.random() < 0.08 else int(rng.integers(max(0, crowd - 30), crowd + 1))
            objs = [o for o in objs if rng.random() > 0.06]      # vanish
            while len(objs) < target:                              # appear
                w, h = int(rng.integers(8, 200)), int(rng.integers(8, 200))
                objs.append([int(rng.integers(0, W - w)), int(rng.integers(0, H - h)), w, h, int(rng.integers(0, n_labels)),
                             int(rng.integers(-4, 5)), int(rng.integers(-4, 5))])
            for o in objs:                                         # drift, a little jitter in size
                o[0] += o[5]
                o[1] += o[6]
                if rng.random() < 0.2:
                    o[2] = max(4, o[2] + int(rng.integers(-2, 3)))
            shown = [o for o in objs if rng.random() > 0.1]        # missed detections: tracks age and come back
            rows = [o[:5] for o in shown[:max_boxes]]
            if rows and rng.random() < 0.3 and len(rows) < max_boxes:  # an exact duplicate: equal keys
                rows.insert(int(rng.integers(0, len(rows) + 1)), list(rows[int(rng.integers(0, len(rows)))]))
            order = rng.permutation(len(rows))
            a = np.asarray([rows[i] for i in order], np.int32).reshape(-1, 5)
            frames.append((np.ascontiguousarray(a[:, :4]), np.ascontiguousarray(a[:, 4])))
        out.append(frames)
    return out


def run_reference(seqs, max_lost: int = 8, iou_threshold: float = 0.3, classify=None, reclassify: int = 1,
                  frame_step: int = 1, frame_indices=None):
    """The reference over ``random_sequences`` output: ``(per stream per frame (ids, due), per stream state, Events)``.
    Frame f of stream s has frame index ``f * frame_step``, or ``frame_indices[s][f]`` where given."""
    ev = Events()
    results, states = [], []
    for s, frames in enumerate(seqs):
        ev.seen = {}
        trk = Tracker(max_lost, iou_threshold, ev)
        fi = [f * frame_step for f in range(len(frames))] if frame_indices is None else frame_indices[s]
        results.append([trk.step(int(fi[f]), b, lab, classify, reclassify) for f, (b, lab) in enumerate(frames)])
        states.append(trk.state())
    return results, states, ev


# ---- inputs that need as many matching rounds as there are tracks ----

CHAIN_W, CHAIN_H = 2000, 100


def chain_frames(n: int = 128, seed: int = 0, label: int = 0, y: int = 0):
    """Two frames of one stream and one label whose second frame needs ``n`` matching rounds, one match per round.

    Track i sits at x = X_i (boxes CHAIN_W x CHAIN_H), detection i at X_i + d_i with d_i = 2n - 2i and
    X_{i+1} - X_i = 4n - 4i - 1. Detection i is then d_i away from its own track and d_i - 1 from track i + 1, whose own
    detection is closer still (d_i - 2): every detection's best track is the next one over, every track's best
    detection is its own, and only the last pair is mutually best. The rule gives detection i the id of track i.
    A seeded permutation orders the tracks' births (frame 0) and another the detections (frame 1), so that a slot index
    is no chain index. Returns ``(frames, ids)``: ``[(boxes, labels)] * 2`` as ``random_sequences`` gives them, and
    the ids the second frame must get (the first frame's are 1..n)."""
    rng = np.random.default_rng(seed)
    xs = [0]
    for i in range(n - 1):
        xs.append(xs[-1] + 4 * n - 4 * i - 1)
    born, order = rng.permutation(n), rng.permutation(n)
    id_of = {int(c): j + 1 for j, c in enumerate(born)}  # chain index -> id: ids follow the order of birth
    f0 = np.asarray([(xs[c], y, CHAIN_W, CHAIN_H) for c in born], np.int32).reshape(-1, 4)
    f1 = np.asarray([(xs[c] + 2 * n - 2 * c, y, CHAIN_W, CHAIN_H) for c in order], np.int32).reshape(-1, 4)
    labels = np.full(n, label, np.int32)
    return [(f0, labels), (f1, labels.copy())], [id_of[int(c)] for c in order]


def interleave(a, b):
    """Two equally long ``(boxes, labels)`` frames as one, rows alternating a, b, a, b .."""
    boxes = np.stack([a[0], b[0]], axis=1).reshape(-1, 4)
    labels = np.stack([a[1], b[1]], axis=1).reshape(-1)
    return np.ascontiguousarray(boxes), np.ascontiguousarray(labels)


def two_label_chain_frames(n: int = 64, seed: int = 0):
    """Two chains of ``n`` in labels 0 and 1 on the same pixels, their rows interleaved: the label test carves the
    candidate matrix into two chains of ``n`` rounds each, which run side by side. Returns ``(frames, ids)``."""
    (a0, a1), ia = chain_frames(n, seed, label=0)
    (b0, b1), ib = chain_frames(n, seed + 1, label=1)
    # births alternate a, b: chain a's j-th born has id 2j + 1, chain b's 2j + 2
    ids = [v for pair in zip([2 * i - 1 for i in ia], [2 * i for i in ib]) for v in pair]
    return [interleave(a0, b0), interleave(a1, b1)], ids


def far_rows(k: int, label: int = 0):
    """``k`` small boxes far from every chain and grid and from each other: detections appended past D."""
    boxes = np.asarray([(50 * i, 500000, 30, 30) for i in range(k)], np.int32).reshape(-1, 4)
    return boxes, np.full(k, label, np.int32)


def disjoint_frames(n: int = 128, shift: int = 100000):
    """An ``n``-box grid and the same grid moved ``shift`` px, one label: at ``iou_threshold`` 0.0 every pair is a
    candidate of key 0, the ties fall to the lowest slot and then the lowest detection, one pair matches per round."""
    a = np.asarray([((i % 16) * 40, (i // 16) * 40, 30, 30) for i in range(n)], np.int32).reshape(-1, 4)
    b = a.copy()
    b[:, 0] += shift
    labels = np.zeros(n, np.int32)
    return [(a, labels), (b, labels.copy())]


EXTREME_FIELDS = (-2**31, -2**20, -1, 0, 1, 7, 100, 2**20 - 1, 2**20, 2**20 + 1, 2**31 - 1)
EXTREME_LABELS = (-2**31, 0, 2**31 - 1)
LAST_FRAME = 0xFFFFFFFE


def extreme_sequences(seed: int, n_streams: int = 2, n_frames: int = 30, max_boxes: int = 140, pool: int = 60):
    """Sequences for the key arithmetic: every box field drawn from ``EXTREME_FIELDS``, labels from
    ``EXTREME_LABELS``; about 70 % of a frame's rows come from a per-stream pool of ``pool`` rows (tracks persist,
    identical boxes recur), the rest are fresh. Frames hold 0..max_boxes rows. Returns ``(seqs, frame_indices)``:
    ``seqs`` as ``random_sequences``, ``frame_indices[s]`` ascending in uneven steps (one of them 2^31) and ending at
    ``LAST_FRAME``, the largest index the API takes."""
    rng = np.random.default_rng(seed)
    fields, labs = np.asarray(EXTREME_FIELDS, np.int64), np.asarray(EXTREME_LABELS, np.int64)

    def rows(k):
        return np.concatenate([rng.choice(fields, (k, 4)), rng.choice(labs, (k, 1))], axis=1)

    seqs, indices = [], []
    for _ in range(n_streams):
        base = rows(pool)
        frames = []
        for _ in range(n_frames):
            k = 0 if rng.random() < 0.08 else int(rng.integers(0, max_boxes + 1))
            from_pool = rng.random(k) < 0.7
            a = np.where(from_pool[:, None], base[rng.integers(0, pool, k)], rows(k)).astype(np.int32).reshape(-1, 5)
            frames.append((np.ascontiguousarray(a[:, :4]), np.ascontiguousarray(a[:, 4])))
        steps = rng.choice(np.asarray([1, 1, 2, 3, 5, 7, 1000, 1 << 24], np.int64), max(n_frames - 1, 0))
        if n_frames > 2:
            steps[int(rng.integers(0, n_frames - 1))] = 1 << 31
        idx = LAST_FRAME - np.concatenate([np.cumsum(steps[::-1])[::-1], [0]]).astype(np.int64)
        assert idx[0] >= 0 and (np.diff(idx) > 0).all() and idx[-1] == LAST_FRAME
        seqs.append(frames)
        indices.append([int(v) for v in idx])
    return seqs, indices
