"""Two references for SSD DetectionOutput (the rule of include/evam_pp.h, "SSD DetectionOutput").

``detection_output_bits``: the rule step by step in ``numpy.float32`` arithmetic (every operation one IEEE single
operation, in the order the rule states), including the ``evam_expf`` polynomial. The library's host helper, the native
check program and the kernels must equal it bit for bit.

``detection_output_f64``: the same semantics in plain Python floats (``math.exp``, Python sorts), which also says whether
a case is *decided with margin*: every score more than 1e-6 (relative) away from the threshold and from its neighbour in
order, every evaluated IoU more than 1e-4 away from ``nms_threshold``, no decoded value non-finite. On such a case a
float32 implementation must arrive at the same survivors.

A config here is a plain dict: num_classes, background_label, top_k, keep_top_k, confidence_threshold, nms_threshold.
"""
import math

import numpy as np

F = np.float32
INF = F(np.inf)


def expf_bits(x):
    """``evam_expf`` on a float32 array: Cody-Waite reduction by round(x / ln 2) (the round is the add and subtract of
    1.5 * 2^23), exp(r) = 1 + r + r^2 q(r) with a degree-5 q, the power of two applied as two exponent inserts."""
    x = np.asarray(x, F)
    xc = np.where(np.isnan(x), F(0), np.clip(x, F(-104), F(89))).astype(F)
    with np.errstate(all="ignore"):
        magic = F(12582912.0)
        k = (xc * F(1.44269504088896341) + magic) + (-magic)
        r = xc + k * F(-0.693359375)
        r = r + k * F(2.12194440e-4)
        q = np.full_like(r, F(1.9875691500e-4))
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            q = q * r + F(c)
        y = (q * (r * r) + r) + F(1)
        ki = k.astype(np.int64)
        k1 = ki >> 1
        k2 = ki - k1
        s1 = ((k1 + 127) << 23).astype(np.uint32).view(F)
        s2 = ((k2 + 127) << 23).astype(np.uint32).view(F)
        res = (y * s1) * s2
    res = np.where(x > F(89), INF, res)
    res = np.where(x < F(-104), F(0), res)
    return np.where(np.isnan(x), F(np.nan), res).astype(F)


def decode_bits(prior, var, l):
    """Step 3 on float32 arrays ``[m, 4]``: ``([m, 4] boxes, [m] all four values finite)``."""
    with np.errstate(all="ignore"):
        pw = prior[:, 2] - prior[:, 0]
        ph = prior[:, 3] - prior[:, 1]
        pcx = (prior[:, 0] + prior[:, 2]) * F(0.5)
        pcy = (prior[:, 1] + prior[:, 3]) * F(0.5)
        cx = ((var[:, 0] * l[:, 0]) * pw) + pcx
        cy = ((var[:, 1] * l[:, 1]) * ph) + pcy
        w = expf_bits(var[:, 2] * l[:, 2]) * pw
        h = expf_bits(var[:, 3] * l[:, 3]) * ph
        hw, hh = w * F(0.5), h * F(0.5)
        box = np.stack([cx - hw, cy - hh, cx + hw, cy + hh], axis=1).astype(F)
    return box, np.isfinite(box).all(axis=1)


def area_bits(b):
    with np.errstate(all="ignore"):
        a = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return np.where((b[..., 2] < b[..., 0]) | (b[..., 3] < b[..., 1]), F(0), a).astype(F)


def jaccard_bits(a, kept):
    """Step 5's overlap of box ``a`` [4] with every box of ``kept`` [k, 4], float32."""
    with np.errstate(all="ignore"):
        disjoint = (kept[:, 0] > a[2]) | (kept[:, 2] < a[0]) | (kept[:, 1] > a[3]) | (kept[:, 3] < a[1])
        iw = np.minimum(a[2], kept[:, 2]) - np.maximum(a[0], kept[:, 0])
        ih = np.minimum(a[3], kept[:, 3]) - np.maximum(a[1], kept[:, 1])
        inter = iw * ih
        j = inter / ((area_bits(a) + area_bits(kept)) - inter)
    return np.where(disjoint | (iw <= 0) | (ih <= 0), F(0), j).astype(F)


def detection_output_bits(loc, conf, priors, cfg):
    """``(float32 [N, K, 7] blob, uint32 [N] counts)`` by the rule, in float32."""
    C, K, top_k = cfg["num_classes"], cfg["keep_top_k"], cfg["top_k"]
    thr, nms = F(cfg["confidence_threshold"]), F(cfg["nms_threshold"])
    loc = np.asarray(loc, F)
    N = loc.shape[0]
    loc = loc.reshape(N, -1, 4)
    P = loc.shape[1]
    conf = np.asarray(conf, F).reshape(N, P, C)
    pr = np.asarray(priors, F).reshape(2, P, 4)
    out = np.zeros((N, K, 7), F)
    out[:, :, 0] = -1
    counts = np.zeros(N, np.uint32)
    for n in range(N):
        kept = []  # (class, score, p, box)
        for c in range(C):
            if c == cfg["background_label"]:
                continue
            s = conf[n, :, c]
            with np.errstate(invalid="ignore"):
                idx = np.nonzero(np.isfinite(s) & (s > thr))[0]
            idx = idx[np.lexsort((idx, -s[idx].astype(np.float64)))][:top_k]  # score descending, then p
            box, ok = decode_bits(pr[0, idx], pr[1, idx], loc[n, idx])
            kb = np.zeros((len(idx), 4), F)
            nk = 0
            for j in range(len(idx)):
                if not ok[j]:
                    continue
                if nk and not np.all(jaccard_bits(box[j], kb[:nk]) <= nms):
                    continue
                kb[nk] = box[j]
                nk += 1
                kept.append((c, s[idx[j]], int(idx[j]), box[j]))
        if len(kept) > K:
            kept = sorted(kept, key=lambda e: (-float(e[1]), e[0], e[2]))[:K]
        kept.sort(key=lambda e: (e[0], -float(e[1]), e[2]))
        for r, (c, sc, p, b) in enumerate(kept):
            out[n, r] = (F(n), F(c), sc, b[0], b[1], b[2], b[3])
        counts[n] = len(kept)
    return out, counts


def detection_output_f64(loc, conf, priors, cfg):
    """``(set of survivors (n, c, p), decided_with_margin)`` in Python floats."""
    C, K, top_k = cfg["num_classes"], cfg["keep_top_k"], cfg["top_k"]
    thr, nms = float(F(cfg["confidence_threshold"])), float(F(cfg["nms_threshold"]))
    loc = np.asarray(loc, np.float64)
    N = loc.shape[0]
    loc = loc.reshape(N, -1, 4)
    P = loc.shape[1]
    conf = np.asarray(conf, np.float64).reshape(N, P, C)
    pr = np.asarray(priors, np.float64).reshape(2, P, 4).tolist()
    margin = True

    def close(a, b, rel=1e-6):
        return abs(a - b) <= rel * max(abs(a), abs(b))

    def area(b):
        return 0.0 if b[2] < b[0] or b[3] < b[1] else (b[2] - b[0]) * (b[3] - b[1])

    def iou(a, b):
        if b[0] > a[2] or b[2] < a[0] or b[1] > a[3] or b[3] < a[1]:
            return 0.0
        iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
        if iw <= 0 or ih <= 0:
            return 0.0
        inter = iw * ih
        return inter / (area(a) + area(b) - inter)

    survivors = set()
    for n in range(N):
        kept = []
        ln = loc[n].tolist()
        for c in range(C):
            if c == cfg["background_label"]:
                continue
            s = conf[n, :, c].tolist()
            if any(math.isfinite(v) and close(v, thr) for v in s):
                margin = False
            cand = sorted((p for p in range(P) if math.isfinite(s[p]) and s[p] > thr), key=lambda p: (-s[p], p))
            if any(close(s[a], s[b]) for a, b in zip(cand, cand[1:top_k + 1])):
                margin = False
            boxes = []
            for p in cand[:top_k]:
                (x0, y0, x1, y1), v, l = pr[0][p], pr[1][p], ln[p]
                pw, ph = x1 - x0, y1 - y0
                try:
                    cx, cy = v[0] * l[0] * pw + (x0 + x1) * 0.5, v[1] * l[1] * ph + (y0 + y1) * 0.5
                    w, h = math.exp(v[2] * l[2]) * pw, math.exp(v[3] * l[3]) * ph
                    b = (cx - w * 0.5, cy - h * 0.5, cx + w * 0.5, cy + h * 0.5)
                except OverflowError:
                    b = (math.inf,) * 4
                if not all(math.isfinite(t) and abs(t) < 1e30 for t in b):
                    margin = False
                    continue
                drop = False
                for kb in boxes:
                    j = iou(b, kb)
                    if abs(j - nms) <= 1e-4:
                        margin = False
                    if not j <= nms:
                        drop = True
                        break
                if not drop:
                    boxes.append(b)
                    kept.append((c, s[p], p))
        if len(kept) > K:
            kept.sort(key=lambda e: (-e[1], e[0], e[2]))
            if close(kept[K - 1][1], kept[K][1]):
                margin = False
            kept = kept[:K]
        survivors.update((n, c, p) for c, _, p in kept)
    return survivors, margin


def blob_rows(out, counts):
    """``[(n, class, score bits)]`` of a blob's survivor rows (a row does not name its prior)."""
    rows = []
    for n in range(out.shape[0]):
        for r in range(int(counts[n])):
            rows.append((n, int(out[n, r, 1]), out[n, r, 2].view(np.uint32).item()))
    return rows
