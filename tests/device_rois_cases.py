"""Seeded SSD detection batches for the device-ROI tests, and the Python chain they are checked against.

A batch is what a detector hands a gvaclassify stage: ``det`` float32 ``[n, K, 7]`` rows of (image_id, label, conf,
x0, y0, x1, y1), one frame size and one transform per item. ``python_rois`` is the host path restated with the
package's own functions: ``postproc.parse_ssd_batch`` -> ``postproc.detections_to_regions`` -> the label filter ->
``pipeline_server.roi_inside``; the rects it lists, in its order, are what ``evam_pp_ssd_rois_host`` and
``evam_pp_ssd_rois`` must produce.

The rows mix: boxes partly outside [0, 1]; x1 < x0; zero-area boxes; confidences exactly at the threshold (and one
float32 step below it); a terminator in the middle of an item with high-confidence rows after it; items with no row;
dyadic boxes whose products with the (even) frame size land exactly on .5; fractional and negative labels.
"""
from collections import namedtuple

import numpy as np

SIZES = [(352, 198), (320, 180), (64, 48), (200, 120)]  # even sizes; 352 = 32 * 11 and 198 = 2 * 99 give exact .5 products
THRESHOLD = 0.4
TENSOR = (96, 64)
KINDS = ["none", "identity", "letterbox_tl", "letterbox_center", "central_crop", "mixed"]

Batch = namedtuple("Batch", "det sizes xf tensor threshold labels")


def transform_fields(kind, W, H, TW, TH):
    """The evam_transform fields of a full-frame item of a W x H frame into a TW x TH tensor (include/evam_pp.h)."""
    sx, sy = TW / W, TH / H
    if kind == "identity":
        rw, rh, ox, oy = TW, TH, 0, 0
    else:
        crop = kind == "central_crop"
        x_dom = sx >= sy if crop else sx <= sy
        rw, rh = (TW, int(H * sx)) if x_dom else (int(W * sy), TH)
        rw, rh = max(rw, 1), max(rh, 1)
        if crop:
            rw, rh = max(rw, TW), max(rh, TH)
            ox, oy = -((rw - TW) // 2), -((rh - TH) // 2)
        else:
            rw, rh = min(rw, TW), min(rh, TH)
            ox, oy = ((TW - rw) // 2, (TH - rh) // 2) if kind == "letterbox_center" else (0, 0)
    return dict(scale_x=rw / W, scale_y=rh / H, crop_x=0, crop_y=0, crop_w=W, crop_h=H, pad_x=ox, pad_y=oy,
                resized_w=rw, resized_h=rh)


def make_transforms(evam, kind, sizes, tensor, rng):
    """None, or the ``evam_transform`` array of the items (scales rounded to float32, as the library returns them)."""
    if kind == "none":
        return None
    arr = (evam.native.EvamTransform * len(sizes))()
    each = ["identity", "letterbox_tl", "letterbox_center", "central_crop"]
    for i, (W, H) in enumerate(sizes):
        k = each[int(rng.integers(len(each)))] if kind == "mixed" else kind
        for name, v in transform_fields(k, W, H, *tensor).items():
            setattr(arr[i], name, v)
    return arr


def make_batch(evam, seed, n, K, kind="none", labels=None, threshold=THRESHOLD, sizes=None, density=0.5):
    rng = np.random.default_rng(seed)
    sizes = sizes or [SIZES[int(rng.integers(len(SIZES)))] for _ in range(n)]
    thr32 = np.float32(threshold)
    det = np.zeros((n, K, 7), np.float32)
    det[:, :, 1] = rng.integers(0, 6, (n, K))
    det[:, :, 2] = np.where(rng.random((n, K)) < density, rng.uniform(threshold, 1.0, (n, K)),
                            rng.uniform(0.0, threshold, (n, K)))
    box = rng.uniform(-0.25, 1.25, (n, K, 4)).astype(np.float32)
    lo, hi = np.minimum(box[..., :2], box[..., 2:]), np.maximum(box[..., :2], box[..., 2:])
    det[:, :, 3:5], det[:, :, 5:7] = lo, hi
    flat = det.reshape(-1, 7)
    pick = lambda frac: np.flatnonzero(rng.random(len(flat)) < frac)  # noqa: E731
    for r in pick(0.08):    # x1 < x0 (and y)
        flat[r, 3:7] = flat[r, [5, 6, 3, 4]]
    for r in pick(0.06):    # zero area
        flat[r, 5] = flat[r, 3]
    for r in pick(0.15):    # dyadic: k / 64 across, k / 4 down: products with 352 x 198 end in .5
        flat[r, 3], flat[r, 5] = sorted(rng.integers(0, 65, 2) / 64.0)
        flat[r, 4], flat[r, 6] = sorted(rng.integers(0, 5, 2) / 4.0)
    for r in pick(0.08):    # confidence exactly at the threshold, or one float32 step below it
        flat[r, 2] = thr32 if rng.random() < 0.6 else np.nextafter(thr32, np.float32(0))
    for r in pick(0.08):    # labels that int() truncates; negative ones
        flat[r, 1] = rng.choice([2.75, 0.5, -0.5, -1.0, 3.999])
    for i in range(n):
        u = rng.random()
        if u < 0.2 and K > 1:      # a terminator in the middle, high-confidence rows after it
            t = int(rng.integers(1, K))
            det[i, t, 0] = -1.0
            det[i, t + 1:, 2] = 0.99
        elif u < 0.3:              # no row at all
            det[i, 0, 0] = -1.0
            det[i, 1:, 2] = 0.99
        elif u < 0.4:              # nothing above the threshold
            det[i, :, 2] = rng.uniform(0.0, threshold * 0.99, K)
    return Batch(det, sizes, make_transforms(evam, kind, sizes, TENSOR, rng), TENSOR, threshold, labels)


def python_rois(evam, b):
    """The host path: ``[(item, x, y, w, h)]`` in the order a classify stage would crop them."""
    P, roi_inside = evam.postproc, evam.pipeline_server.roi_inside
    from importlib import import_module

    xfs = None if b.xf is None else import_module(evam.__name__ + ".preproc").Transforms(b.xf)
    out = []
    for i, dets in enumerate(P.parse_ssd_batch(b.det, b.threshold)):
        W, H = b.sizes[i]
        for r in P.detections_to_regions(dets, None if xfs is None else xfs[i], W, H, b.tensor[0], b.tensor[1]):
            if b.labels is not None and r.label_id not in b.labels:
                continue
            if roi_inside(r.x, r.y, r.w, r.h, W, H):
                out.append((i, r.x, r.y, r.w, r.h))
    return out


def host_rois(evam, b, cap=None):
    return evam.native.ssd_rois_host(b.det, b.sizes, b.xf, b.tensor, b.threshold, b.labels, cap)


CASES = [(n, K, kind, labels) for n in (1, 3, 64) for K in (1, 10, 200)
         for kind, labels in (("none", None), ("mixed", (1, 2, 4)))]
CASES += [(3, 10, kind, lab) for kind in KINDS[1:5] for lab in (None, (0, 3))]


def case_id(c):
    n, K, kind, labels = c
    return f"n{n}-K{K}-{kind}-{'all' if labels is None else 'labels'}"
