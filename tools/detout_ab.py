#!/usr/bin/env python3
"""SSD DetectionOutput on the device against what a user has without it (diagnostic, needs the GPU).

Heads of N = 32 images in two layouts, both of published SSD models (the same P and C on both sides):
  ssd300_voc       P = 8732 priors, C = 21 classes  (SSD300 / VGG-16 on PASCAL VOC, Liu et al. 2016: 38^2*4 + 19^2*6 +
                   10^2*6 + 5^2*6 + 3^2*4 + 1^2*4 priors), top_k 400, keep_top_k 200, confidence 0.01, NMS 0.45;
  ssd_mobilenet    P = 1917 priors, C = 91 classes  (SSD-MobileNet-v1 300x300 on COCO, TensorFlow Object Detection API:
                   19^2*3 + (10^2 + 5^2 + 3^2 + 2^2 + 1^2)*6 priors), top_k 100, keep_top_k 100, confidence 0.01, NMS 0.45.
The heads are synthetic (seeded): class probabilities are the softmax of unit-normal logits with the background logit
raised by 7, and ``--objects`` planted objects per image that raise one class on a few overlapping priors; the deltas
are normal(0, 0.5). Every step uses the next of ``--sets`` head sets.

Routes:
  D  ``HipPreProcessor.detection_output`` on device tensors: the two launches' device time (events around the call, a
     synchronisation after each) and the host's time inside the call;
  H  the alternative without it: both heads copied to the host, ``detection_output_host`` there (one thread), the blob
     copied back; wall time from the synchronised start to the blob on the device.
The blobs of both routes are compared byte for byte. Nobody has to win: the figures are for DESIGN.md §5.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = {
    "ssd300_voc": dict(P=8732, C=21, top_k=400, keep_top_k=200),
    "ssd_mobilenet": dict(P=1917, C=91, top_k=100, keep_top_k=100),
}


def quantiles(v):
    v = sorted(v)
    return {"median_us": round(v[len(v) // 2], 2), "p10_us": round(v[len(v) // 10], 2),
            "p90_us": round(v[(9 * len(v)) // 10], 2)}


def make_heads(np, seed, N, P, C, objects):
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0.05, 0.95, (P, 2))
    size = rng.uniform(0.05, 0.5, (P, 2))
    priors = np.zeros((2, P, 4), np.float32)
    priors[0, :, :2] = ctr - size / 2
    priors[0, :, 2:] = ctr + size / 2
    priors[1] = (0.1, 0.1, 0.2, 0.2)
    loc = rng.normal(0, 0.5, (N, P, 4)).astype(np.float32)
    logits = rng.normal(0, 1, (N, P, C))
    logits[:, :, 0] += 7
    for n in range(N):
        for _ in range(objects):
            c = int(rng.integers(1, C))
            p0 = int(rng.integers(0, P - 8))
            logits[n, p0:p0 + 6, c] += rng.uniform(8, 12)
            priors[0, p0:p0 + 6] = priors[0, p0] + rng.normal(0, 0.004, (6, 4))  # overlapping: NMS has work
            loc[n, p0:p0 + 6] = loc[n, p0]
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    conf = (e / e.sum(axis=2, keepdims=True)).astype(np.float32)
    return loc.reshape(N, -1), conf.reshape(N, -1), priors.reshape(2, -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--objects", type=int, default=12)
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import __graft_entry__ as g

    evam = g.import_package()
    dev = torch.device("cuda:0")
    pp = evam.HipPreProcessor(device=0)
    src = open(os.path.join(ROOT, g.PKG, "csrc", "evam_detout_kernels.h"), "rb").read()
    result = {"tool": "tools/detout_ab.py", "kernel_src_sha16": hashlib.sha256(src).hexdigest()[:16],
              "device": torch.cuda.get_device_name(0), "n": args.n, "objects_per_image": args.objects,
              "sets": args.sets, "warmup": args.warmup, "steps": args.steps, "rows": []}
    for name, lay in LAYOUTS.items():
        P, C = lay["P"], lay["C"]
        attrs = dict(num_classes=C, background_label_id=0, top_k=lay["top_k"], keep_top_k=lay["keep_top_k"],
                     confidence_threshold=0.01, nms_threshold=0.45)
        cfg = evam.DetectionOutputConfig.from_attributes(attrs)
        sets = []
        priors = None
        for s in range(args.sets):
            loc, conf, pr = make_heads(np, 1000 + s, args.n, P, C, args.objects)
            priors = pr if priors is None else priors  # one constant prior tensor, as in a model
            sets.append((torch.from_numpy(loc).to(dev), torch.from_numpy(conf).to(dev)))
        d_priors = torch.from_numpy(priors).to(dev)
        out = torch.empty((args.n, lay["keep_top_k"], 7), dtype=torch.float32, device=dev)
        counts = torch.zeros((args.n,), dtype=torch.int32, device=dev)

        def route_d(k):
            loc, conf = sets[k % args.sets]
            return pp.detection_output(loc, conf, d_priors, cfg, out=out, counts=counts)

        def route_h(k):
            loc, conf = sets[k % args.sets]
            blob, _ = evam.detection_output_host(loc.cpu().numpy(), conf.cpu().numpy(), priors, cfg)
            return torch.from_numpy(blob).to(dev)

        # equal bytes first
        same = True
        survivors = []
        for k in range(args.sets):
            a = route_d(k).cpu().numpy().tobytes()
            survivors.append(int(counts.sum().item()))
            same &= a == route_h(k).cpu().numpy().tobytes()
        for k in range(args.warmup):
            route_d(k)
        torch.cuda.synchronize()
        d_dev, d_host = [], []
        for t in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            route_d(t)
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            d_dev.append(a.elapsed_time(b) * 1e3)
            d_host.append((t1 - t0) * 1e6)
        h_wall = []
        for t in range(max(3, args.steps // 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            route_h(t)
            torch.cuda.synchronize()
            h_wall.append((time.perf_counter() - t0) * 1e6)
        row = {"layout": name, "P": P, "C": C, "top_k": lay["top_k"], "keep_top_k": lay["keep_top_k"],
               "head_bytes": args.n * P * (4 + C) * 4, "survivors_per_set": survivors, "blobs_equal": bool(same),
               "D_device": quantiles(d_dev), "D_host_call": quantiles(d_host), "H_wall": quantiles(h_wall),
               "H_steps": len(h_wall)}
        row["H_over_D"] = round(row["H_wall"]["median_us"] / row["D_device"]["median_us"], 2)
        result["rows"].append(row)
        print(json.dumps(row))
    pp.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
