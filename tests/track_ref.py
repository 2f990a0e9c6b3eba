"""The gvatrack rule in plain Python: the oracle of the tracker tests. Written from the rule's text (the comment in
``include/evam_pp.h``), not from the C++ header; it shares no code with the library.

State per stream: ``next_id`` (from 1) and ``T`` slots ``[id, label, x, y, w, h, lost, classified_at]`` (id 0: free,
``classified_at`` ``NONE``: never classified). Also the random sequences the host, sanitizer-side and GPU tests share
(``random_sequences``), and the events a sweep must reach to show anything (``Events``)."""
import math

import numpy as np

T = 128
D = 128
NONE = 0xFFFFFFFF
SIDE_MAX = 1 << 20
FREE = (0, 0, 0, 0, 0, 0, 0, NONE)


def thr_key(iou_threshold: float) -> int:
    """floor(iou_threshold * 65536), the threshold taken as the float32 the C struct carries."""
    return min(max(int(math.floor(float(np.float32(iou_threshold)) * 65536.0)), 0), 65536)


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
        self.seen = {}


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
                  frame_step: int = 1):
    """The reference over ``random_sequences`` output: ``(per stream per frame (ids, due), per stream state, Events)``.
    Frame f of a stream has frame index ``f * frame_step``."""
    ev = Events()
    results, states = [], []
    for frames in seqs:
        ev.seen = {}
        trk = Tracker(max_lost, iou_threshold, ev)
        results.append([trk.step(f * frame_step, b, lab, classify, reclassify) for f, (b, lab) in enumerate(frames)])
        states.append(trk.state())
    return results, states, ev
