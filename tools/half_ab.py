#!/usr/bin/env python3
"""fp32 output against 16-bit (fp16 / bf16) output, one launch at a time with device events (diagnostic, needs the GPU).

Routes, per shape and 16-bit type:
  F  fp32 ``convert``;
  C  fp32 ``convert`` followed by ``.to(dtype)`` of what it wrote, on the same stream, events around both: the only
     way to a 16-bit tensor without 16-bit kernels (a second full pass over the fp32 staging tensor);
  H  ``convert`` into a 16-bit tensor (``PreProcInfo.precision``): one pass, 2-byte elements written by the kernels.

Shapes come from ``bench.WORKLOADS`` (c2, c4, c5, c3: the float configs, C5 with its clip-ring slots, C3 with its
seeded ROI sets). Every launch uses the next of ``--sets`` (>= 5) frame / output sets, so neither L2 nor the 256 MB
Infinity Cache holds the data, as bench.py does. Bytes per launch are the library's own accounting (evam_pp_stats:
src_bytes + dst_bytes), so H's rate counts the bytes H moves. ``--baseline`` times F and C only, through API that
exists without the 16-bit types, so the same file runs in a checkout of the parent commit:

  python tools/half_ab.py --baseline --out /tmp/half_ab_parent.json      (in the parent checkout)
  python tools/half_ab.py --out /tmp/half_ab_tree.json

Prints one JSON line per (shape, type, route), then one verdict line per (shape, type): H's median against C's, and
against F's median widened by F's own relative spread ((p90 - p10) / median over its repeats in this run). Writes
everything, stamped, to ``--out``.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SHAPES = ("c2", "c4", "c5", "c3")
TYPES = ("f16", "bf16")


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
    med, p10, p90 = us[len(us) // 2], us[len(us) // 10], us[(9 * len(us)) // 10]
    return {"median_us": round(med, 2), "p10_us": round(p10, 2), "p90_us": round(p90, 2),
            "rel_spread": round((p90 - p10) / med, 4), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--types", default=",".join(TYPES))
    ap.add_argument("--baseline", action="store_true", help="F and C only (API of a library without the 16-bit types)")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default=os.environ.get("EVAM_SHA", "unknown"))
    a = ap.parse_args()
    if a.sets < 5 or a.steps < 100 or a.warmup < 10:
        ap.error("--sets >= 5, --steps >= 100, --warmup >= 10")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("half_ab.py needs a GPU")
    import __graft_entry__ as g

    evam = g.import_package()
    N = evam.native
    dev = torch.device("cuda:0")
    src_dir = os.path.join(ROOT, "edge-video-analytics-microservice_amd", "csrc")
    sha = hashlib.sha256(b"".join(open(os.path.join(src_dir, f), "rb").read() for f in sorted(os.listdir(src_dir))
                                  if f.endswith((".hip", ".h")))).hexdigest()[:16]
    result = {"tool": "tools/half_ab.py", "git_head": a.head, "kernel_src_sha16": sha, "baseline": a.baseline,
              "sets": a.sets, "warmup": a.warmup, "hbm_peak_GBs": bench.HBM_PEAK_GBS, "rows": [], "verdicts": []}
    pp = evam.HipPreProcessor(device=0)
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}
    prec = {"f16": "FP16", "bf16": "BF16"}
    for name in a.shapes.split(","):
        wl = bench.WORKLOADS[name]
        n, (DW, DH), ring = wl["frames"], wl["dst"], wl.get("ring")
        frames = [evam.ImageBatch(bench.device_frames(evam, torch, wl, n, dev, seed=100 + k)) for k in range(a.sets)]
        rois = None
        if wl.get("rois"):
            rois = [evam.RoiBatch(np.array(bench.seed_rois(wl["rois"], n, *wl["src"], seed=k), dtype=np.int32))
                    for k in range(a.sets)]
        items = len(rois[0]) if rois else n
        slots = items * (ring or 1)

        def call(k, out, info):
            # C5: slot k % ring of every stream's clip (slot_stride = ring), as the stage writes it
            kw = {"slot_offset": k % ring, "slot_stride": ring} if ring else {}
            pp.convert(frames[k], out, info, rois=rois[k] if rois else None, **kw)

        def written(k, out):
            return out.view(items, ring, 3, DH, DW)[:, k % ring] if ring else out

        def stat_bytes(out, info):
            pp.set_option(N.OPT_STATS, 1)
            call(0, out, info)
            torch.cuda.synchronize()
            st = pp.stats()
            pp.set_option(N.OPT_STATS, 0)
            return int(st.src_bytes), int(st.dst_bytes)

        info32 = bench.make_info(evam, wl)
        f32 = [torch.empty((slots, 3, DH, DW), dtype=torch.float32, device=dev) for _ in range(a.sets)]
        src32, dst32 = stat_bytes(f32[0], info32)
        for ty in a.types.split(","):
            routes = [("F", src32 + dst32, lambda k: call(k, f32[k], info32)),
                      # C reads the fp32 tensor back and writes the 16-bit one: the bytes of both passes
                      ("C", src32 + 2 * dst32 + dst32 // 2,
                       lambda k: (call(k, f32[k], info32), written(k, f32[k]).to(tdt[ty])))]
            half = None
            if not a.baseline:
                info16 = bench.make_info(evam, wl)
                info16.precision = prec[ty]
                half = [torch.empty((slots, 3, DH, DW), dtype=tdt[ty], device=dev) for _ in range(a.sets)]
                src16, dst16 = stat_bytes(half[0], info16)
                routes.append(("H", src16 + dst16, lambda k: call(k, half[k], info16)))
            med = {}
            for route, nbytes, fn in routes:
                r = time_route(torch, fn, a.sets, a.warmup, a.steps)
                gbs = nbytes / (r["median_us"] * 1e-6) / 1e9
                row = {"shape": name, "type": ty, "route": route, **r, "bytes_moved": nbytes, "GBs": round(gbs, 1),
                       "frac_of_8TBs": round(gbs / bench.HBM_PEAK_GBS, 4), "kernels": int(pp.stats().kernels)}
                result["rows"].append(row)
                med[route] = r
                print(json.dumps(row), flush=True)
            if not a.baseline:
                fm, cm, hm, sp = med["F"]["median_us"], med["C"]["median_us"], med["H"]["median_us"], med["F"]["rel_spread"]
                v = {"shape": name, "type": ty, "F_median_us": fm, "C_median_us": cm, "H_median_us": hm,
                     "F_rel_spread": sp, "H_below_C": hm < cm, "H_within_F_spread": hm <= fm * (1.0 + sp),
                     "H_over_F": round(hm / fm, 4), "H_over_C": round(hm / cm, 4)}
                result["verdicts"].append(v)
                print(json.dumps(v), flush=True)
            del half, routes
            torch.cuda.empty_cache()
        del frames, f32
        torch.cuda.empty_cache()
    pp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
