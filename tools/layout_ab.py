#!/usr/bin/env python3
"""Planar against interleaved output, one launch at a time with device events (diagnostic, needs the GPU).

Routes, per shape:
  P  planar ``convert`` into a contiguous [N,3,H,W] tensor;
  T  planar ``convert`` followed by ``out.contiguous(memory_format=torch.channels_last)`` on the same stream, events
     around both: the only way to a channels-last tensor without interleaved kernels;
  I  ``convert`` into a channels-last tensor (one pass).

Shapes come from ``bench.WORKLOADS`` (c2, c4, c1) plus ``export``: 32 x 1080p NV12 -> [32,1080,1920,3] u8 at source
size (9,331,200 algorithmic bytes per frame); bytes per launch are the library's own accounting (evam_pp_stats).
Every launch uses the next of ``--sets`` (>= 5) frame / output sets, so neither L2 nor the 256 MB Infinity Cache
holds the data, as bench.py does. ``--baseline`` times P and T only, through
API that exists without the layout field, so the same file runs against an older checkout of the library:

  python tools/layout_ab.py --baseline --out /tmp/layout_ab_parent.json      (in the older checkout)
  python tools/layout_ab.py --out /tmp/layout_ab_tree.json

Prints one JSON line per (shape, route) and writes them all, stamped, to ``--out``.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SHAPES = ("c2", "c4", "c1", "export")


def workload(name):
    if name == "export":
        return dict(desc="export: 32x 1920x1080 NV12 -> 32x1080x1920x3 u8 BGR at source size", fourcc="NV12",
                    src=(1920, 1080), frames=32, dst=(1920, 1080), dtype="u8", norm=False, mode="no-aspect-ratio")
    return bench.WORKLOADS[name]


def algorithmic_bytes(evam, torch, pp, frames, out, info):
    """The library's own accounting of one launch (evam_pp_stats): the source rows the taps touch, read once, plus
    every output byte, written once. The same for all three routes of a shape, so their rates compare as their
    times do."""
    N = evam.native
    pp.set_option(N.OPT_STATS, 1)
    pp.convert(frames, out, info)
    torch.cuda.synchronize()
    st = pp.stats()
    pp.set_option(N.OPT_STATS, 0)
    return int(st.src_bytes + st.dst_bytes)


def time_route(torch, fn, sets, warmup, steps):
    for k in range(warmup):
        fn(k % sets)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for t in range(steps):
        ev[t][0].record()
        fn(t % sets)
        ev[t][1].record()
        torch.cuda.synchronize()  # one launch at a time
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": round(us[len(us) // 2], 2), "p10_us": round(us[len(us) // 10], 2),
            "p90_us": round(us[(9 * len(us)) // 10], 2), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--baseline", action="store_true", help="P and T only (API of a library without the layout field)")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default=os.environ.get("EVAM_SHA", "unknown"))
    a = ap.parse_args()
    if a.sets < 5 or a.steps < 100 or a.warmup < 10:
        ap.error("--sets >= 5, --steps >= 100, --warmup >= 10")
    import torch

    if not torch.cuda.is_available():
        sys.exit("layout_ab.py needs a GPU")
    import __graft_entry__ as g

    evam = g.import_package()
    dev = torch.device("cuda:0")
    src_dir = os.path.join(ROOT, "edge-video-analytics-microservice_amd", "csrc")
    sha = hashlib.sha256(b"".join(open(os.path.join(src_dir, f), "rb").read() for f in sorted(os.listdir(src_dir))
                                  if f.endswith((".hip", ".h")))).hexdigest()[:16]
    result = {"tool": "tools/layout_ab.py", "git_head": a.head, "kernel_src_sha16": sha, "baseline": a.baseline,
              "sets": a.sets, "warmup": a.warmup, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "rows": []}
    pp = evam.HipPreProcessor(device=0)
    for name in a.shapes.split(","):
        wl = workload(name)
        n, (DW, DH) = wl["frames"], wl["dst"]
        dt = torch.float32 if wl["dtype"] == "f32" else torch.uint8
        info = bench.make_info(evam, wl)
        frames = [evam.ImageBatch(bench.device_frames(evam, torch, wl, n, dev, seed=100 + k)) for k in range(a.sets)]
        planar = [torch.empty((n, 3, DH, DW), dtype=dt, device=dev) for _ in range(a.sets)]
        nbytes = algorithmic_bytes(evam, torch, pp, frames[0], planar[0], info)
        routes = [("P", lambda k: pp.convert(frames[k], planar[k], info)),
                  ("T", lambda k: (pp.convert(frames[k], planar[k], info),
                                   planar[k].contiguous(memory_format=torch.channels_last)))]
        if not a.baseline:
            inter = [torch.empty((n, 3, DH, DW), dtype=dt, device=dev, memory_format=torch.channels_last)
                     for _ in range(a.sets)]
            routes.append(("I", lambda k: pp.convert(frames[k], inter[k], info)))
        for route, fn in routes:
            r = time_route(torch, fn, a.sets, a.warmup, a.steps)
            gbs = nbytes / (r["median_us"] * 1e-6) / 1e9
            row = {"shape": name, "route": route, **r, "algorithmic_bytes": nbytes, "GBs": round(gbs, 1),
                   "frac_of_8TBs": round(gbs / bench.HBM_PEAK_GBS, 4), "kernels": int(pp.stats().kernels)}
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
        del frames, planar, routes
        torch.cuda.empty_cache()
    pp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
