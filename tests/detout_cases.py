"""Seeded cases for SSD DetectionOutput: targeted ones with hand-written expectations, single-parameter sweeps of a
base shape, dense cases that drive the top_k selection, and seeded random combinations.

A case is a dict: name, kind ("targeted" / "sweep" / "dense" / "random"), loc [N, P*4], conf [N, P*C], priors [2, P*4]
(all float32), cfg (the dict tests/detout_ref.py takes) and, for targeted cases, expect: per image the survivors
(class, p) in row order. Targeted cases have loc = 0 and dyadic priors, so a survivor's box is its prior, exactly.
"""
import functools

import numpy as np

F = np.float32
VAR = (0.1, 0.1, 0.2, 0.2)

P_VALUES = (1, 63, 64, 65, 255, 257, 1000, 4099)
C_VALUES = (2, 3, 21)
TOP_K_VALUES = (1, 7, 64, 400, 1024)
K_VALUES = (1, 5, 200, 1024)
N_VALUES = (1, 3, 33)
BASE = dict(N=3, P=257, C=3, top_k=64, K=200)


def make_cfg(C, top_k, K, bg=0, thr=0.25, nms=0.5):
    return dict(num_classes=C, background_label=bg, top_k=top_k, keep_top_k=K, confidence_threshold=float(F(thr)),
                nms_threshold=float(F(nms)))


# ---- targeted ----------------------------------------------------------------------------------------------------
def _targeted(name, boxes, scores, cfg, expect, loc=None, N=1):
    """boxes: P prior boxes; scores: {(n, p, c): s}, everything else 0.0625; loc: {(n, p, j): delta}."""
    P, C = len(boxes), cfg["num_classes"]
    priors = np.zeros((2, P, 4), F)
    priors[0] = np.asarray(boxes, F)
    priors[1] = VAR
    conf = np.full((N, P, C), 0.0625, F)
    for (n, p, c), s in scores.items():
        conf[n, p, c] = s
    l = np.zeros((N, P, 4), F)
    for (n, p, j), v in (loc or {}).items():
        l[n, p, j] = v
    return dict(name=name, kind="targeted", loc=l.reshape(N, -1), conf=conf.reshape(N, -1), priors=priors.reshape(2, -1),
                cfg=cfg, expect=expect)


def targeted_cases():
    A, A2 = (0, 0, .5, .25), (0, 0, .25, .25)                   # IoU exactly 0.5 in float32
    far = [(.5 + i / 16, .5, .5 + i / 16 + 1 / 32, .75) for i in range(8)]  # disjoint from A, A2 and each other
    below = float(np.nextafter(F(0.5), F(0)))
    out = []
    out.append(_targeted("none", [A, far[0]], {}, make_cfg(3, 8, 8), [[]]))
    out.append(_targeted("one", [A, far[0], far[1]], {(0, 2, 1): .875}, make_cfg(3, 8, 8), [[(1, 2)]]))
    tie = {(0, p, c): .5 for p in range(4) for c in (1, 2)}
    out.append(_targeted("ties_k3", far[:4], tie, make_cfg(3, 8, 3), [[(1, 0), (1, 1), (1, 2)]]))
    out.append(_targeted("ties_k5", far[:4], tie, make_cfg(3, 8, 5), [[(1, 0), (1, 1), (1, 2), (1, 3), (2, 0)]]))
    out.append(_targeted("ties_topk2", far[:4], tie, make_cfg(3, 2, 8), [[(1, 0), (1, 1), (2, 0), (2, 1)]]))
    out.append(_targeted("identical_equal", [A, A, far[0]], {(0, 0, 1): .5, (0, 1, 1): .5}, make_cfg(3, 8, 8), [[(1, 0)]]))
    out.append(_targeted("identical_second_wins", [A, A, far[0]], {(0, 0, 1): .5, (0, 1, 1): .75}, make_cfg(3, 8, 8),
                         [[(1, 1)]]))
    out.append(_targeted("iou_at_threshold", [A, A2], {(0, 0, 1): .875, (0, 1, 1): .75}, make_cfg(3, 8, 8, nms=0.5),
                         [[(1, 0), (1, 1)]]))
    out.append(_targeted("iou_above_threshold", [A, A2], {(0, 0, 1): .875, (0, 1, 1): .75}, make_cfg(3, 8, 8, nms=below),
                         [[(1, 0)]]))
    # a chain of top_k boxes 4u wide, u apart: neighbours overlap 3/5, boxes two apart 2/6. Scores fall along the chain:
    # every odd box is killed by the even one before it, every even box meets kept boxes two apart only.
    L, u = 16, 1 / 2048
    chain = [(i * u, 0, i * u + 4 * u, .25) for i in range(L)]
    out.append(_targeted("chain", chain, {(0, i, 1): (64 - i) / 128 + .25 for i in range(L)}, make_cfg(2, L, L),
                         [[(1, i) for i in range(0, L, 2)]]))
    # p1 (the best score) covers p0 and p2 and would suppress both were its box finite: its width delta is +inf (or
    # its x delta NaN), so it is dropped and both stay
    big, left, right = (0, 0, .5, .5), (0, 0, .5, .25 + 1 / 64), (0, .25 - 1 / 64, .5, .5)
    nf = {(0, 1, 1): .875, (0, 0, 1): .75, (0, 2, 1): .625}
    out.append(_targeted("nonfinite_delta", [left, big, right], nf, make_cfg(2, 8, 8), [[(1, 0), (1, 2)]],
                         loc={(0, 1, 2): np.inf}))
    out.append(_targeted("nonfinite_delta_nan", [left, big, right], nf, make_cfg(2, 8, 8), [[(1, 0), (1, 2)]],
                         loc={(0, 1, 0): np.nan}))
    out.append(_targeted("finite_delta_suppresses", [left, big, right], nf, make_cfg(2, 8, 8), [[(1, 1)]]))
    neg = (.5, .5, .25, .25)  # negative size: area 0, overlaps nothing
    out.append(_targeted("negative_prior", [(0, 0, 1, 1), neg, neg], {(0, 0, 1): .875, (0, 1, 1): .75, (0, 2, 1): .625},
                         make_cfg(2, 8, 8), [[(1, 0), (1, 1), (1, 2)]]))
    out.append(_targeted("inf_nan_scores", far[:4], {(0, 0, 1): np.inf, (0, 1, 1): np.nan, (0, 2, 1): 2.0, (0, 3, 1): .5,
                                                      (0, 0, 2): -np.inf}, make_cfg(3, 8, 8), [[(1, 2), (1, 3)]]))
    over = {(0, 0, 1): .875, (0, 1, 1): .75, (0, 2, 1): .625, (0, 3, 1): .5}
    out.append(_targeted("over_top_k", [A, A, far[0], far[1]], over, make_cfg(2, 2, 8), [[(1, 0)]]))
    out.append(_targeted("under_top_k", [A, A, far[0], far[1]], over, make_cfg(2, 4, 8), [[(1, 0), (1, 2), (1, 3)]]))
    tot = {(0, 0, 1): .875, (0, 1, 2): .75, (0, 2, 1): .625, (1, 3, 2): .5}
    out.append(_targeted("total_above_k", far[:4], tot, make_cfg(3, 8, 2), [[(1, 0), (2, 1)], [(2, 3)]], N=2))
    out.append(_targeted("total_below_k", far[:4], tot, make_cfg(3, 8, 4), [[(1, 0), (1, 2), (2, 1)], [(2, 3)]], N=2))
    bgs = {(0, 0, 0): .875, (0, 1, 1): .75, (0, 2, 2): .625}
    out.append(_targeted("background_none", far[:3], bgs, make_cfg(3, 8, 8, bg=-1), [[(0, 0), (1, 1), (2, 2)]]))
    out.append(_targeted("background_0", far[:3], bgs, make_cfg(3, 8, 8, bg=0), [[(1, 1), (2, 2)]]))
    out.append(_targeted("background_middle", far[:3], bgs, make_cfg(3, 8, 8, bg=1), [[(0, 0), (2, 2)]]))
    return out


def expected_blob(case):
    """The blob and counts a targeted case's expectation stands for."""
    cfg = case["cfg"]
    N, K, C = case["loc"].shape[0], cfg["keep_top_k"], cfg["num_classes"]
    pr = case["priors"].reshape(2, -1, 4)
    conf = case["conf"].reshape(N, -1, C)
    out = np.zeros((N, K, 7), F)
    out[:, :, 0] = -1
    counts = np.zeros(N, np.uint32)
    for n, rows in enumerate(case["expect"]):
        for r, (c, p) in enumerate(rows):
            out[n, r] = (n, c, conf[n, p, c], *pr[0, p])
        counts[n] = len(rows)
    return out, counts


# ---- generated ---------------------------------------------------------------------------------------------------
def generated(name, kind, seed, N, P, C, top_k, K, per_class=None, bg=0, small=False, quantize=0):
    """Priors come in pairs (2i, 2i + 1) that overlap strongly, so NMS has work; `per_class` candidates are expected per
    (image, class); `small` priors hardly overlap beyond their pair (dense cases); `quantize` > 0 rounds the scores to
    that many levels, so that many are equal."""
    rng = np.random.default_rng(seed)
    if per_class is None:
        per_class = float(np.clip(400.0 / (N * max(C - 1, 1)), 1.5, 10.0))
    lo, hi = (0.002, 0.01) if small else (0.05, 0.3)
    half = (P + 1) // 2
    ctr = np.repeat(rng.uniform(0.1, 0.9, (half, 2)), 2, axis=0)[:P]
    size = np.repeat(rng.uniform(lo, hi, (half, 2)), 2, axis=0)[:P]
    ctr[1::2] += size[1::2] * 0.06  # the twin of a pair: IoU about 0.8
    priors = np.zeros((2, P, 4), F)
    priors[0, :, :2] = ctr - size / 2
    priors[0, :, 2:] = ctr + size / 2
    priors[1] = VAR
    loc = rng.normal(0, 0.15, (N, P, 4)).astype(F)
    conf = rng.uniform(0.0, 0.2, (N, P, C))
    hot = rng.random((N, P, C)) < min(1.0, per_class / P)
    twin = hot[:, 0:2 * (P // 2):2] & (rng.random((N, P // 2, C)) < 0.5)  # a hot prior's twin, half the time
    hot[:, 1::2] |= twin
    conf[hot] = rng.uniform(0.3, 1.0, int(hot.sum()))
    if quantize:
        conf = np.round(conf * quantize) / quantize
    return dict(name=name, kind=kind, loc=loc.reshape(N, -1), conf=conf.astype(F).reshape(N, -1),
                priors=priors.reshape(2, -1), cfg=make_cfg(C, top_k, K, bg=bg), expect=None)


def sweep_cases():
    out = [generated("base", "sweep", 100, **BASE)]
    for key, values in (("P", P_VALUES), ("C", C_VALUES), ("top_k", TOP_K_VALUES), ("K", K_VALUES), ("N", N_VALUES)):
        for i, v in enumerate(values):
            if BASE[key] == v:
                continue
            out.append(generated(f"{key}={v}", "sweep", 200 + 10 * len(out) + i, **{**BASE, key: v}))
    return out


def dense_cases():
    """More candidates than top_k in a class: the selection, the truncation and equal scores at the cut."""
    return [
        generated("dense_64", "dense", 301, N=2, P=257, C=3, top_k=64, K=200, per_class=150),
        generated("dense_64_ties", "dense", 302, N=2, P=255, C=3, top_k=64, K=5, per_class=200, quantize=16, bg=-1),
        generated("dense_7_ties", "dense", 303, N=3, P=65, C=2, top_k=7, K=5, per_class=40, quantize=8),
        generated("dense_400", "dense", 304, N=1, P=1000, C=2, top_k=400, K=200, per_class=700, small=True),
        generated("dense_1024", "dense", 305, N=2, P=4099, C=2, top_k=1024, K=1024, per_class=2000, small=True),
        generated("dense_1024_ties", "dense", 306, N=1, P=4099, C=3, top_k=1024, K=1024, per_class=2500, small=True,
                  quantize=64, bg=1),
    ]


RANDOM_SEEDS = tuple(range(1000, 1020))


def random_cases():
    out = []
    for seed in RANDOM_SEEDS:
        rng = np.random.default_rng(seed)
        pick = lambda v: int(v[rng.integers(len(v))])  # noqa: E731
        N, P, C, top_k, K = pick(N_VALUES), pick(P_VALUES), pick(C_VALUES), pick(TOP_K_VALUES), pick(K_VALUES)
        bg = int(rng.integers(-1, C))
        out.append(generated(f"random_{seed}", "random", seed, N, P, C, top_k, K, bg=bg))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(targeted_cases() + sweep_cases() + dense_cases() + random_cases())


def case_names(kinds=None):
    return [c["name"] for c in all_cases() if kinds is None or c["kind"] in kinds]


def case(name):
    for c in all_cases():
        if c["name"] == name:
            return c
    raise KeyError(name)
