#!/usr/bin/env python3
"""Host-list against device-list ROI pre-processing, one launch at a time with device events (diagnostic, needs the GPU).

Workload: the C3 shape of ``bench.WORKLOADS`` — 32 1080p NV12 frames, ``bench.seed_rois`` 50 per frame (1,600 ROIs) ->
1600x3x72x72 fp32; every launch uses the next of ``--sets`` (>= 5) frame / ROI / output sets, as bench.py does.

Routes:
  H      ``convert(..., rois=<RoiBatch>)``: the host plans the launch order and writes the records (evam_pp_run);
  D1600  ``convert(..., rois=<DeviceRoiList>)`` of the same rects, cap = 1,600: records built on the device, list order;
  D2048  the same with cap = 2,048: 448 workgroups more that return at once.
Per route: the launch's device time (events around the call, a synchronisation after each) and the host's time inside
the call (perf_counter around it), medians with p10 / p90. ``--baseline`` times H only, through API the parent commit
has, so the same file measures the parent's library in the same session:

  EVAM_PP_LIB=ab/libevam_pp_parent.so python tools/device_rois_ab.py --baseline --out profiles/x_parent.json
  python tools/device_rois_ab.py --pipeline --out profiles/device_rois_ab.json --parent profiles/x_parent.json

``--pipeline`` adds detect -> classify through the pipeline server with the ``device_rois`` option off and on: 32
streams of 1080p NV12 frames from a device-resident pool, a synthetic detector that answers on the device with
``--dets`` boxes per frame (64x64 input), a classifier stub on 72x72 fp32 crops; frames per second of each.
``--parent`` merges a ``--baseline`` result and adds the verdict: the tree's H median inside the parent's own p10-p90.
"""
import argparse
import hashlib
import json
import os
import queue
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

PIPE = {
    "type": "GStreamer",
    "template": ["{auto_source} ! decodebin",
                 " ! gvadetect model={models[ab_detector][1][network]} name=det",
                 " ! gvaclassify model={models[ab_classifier][1][network]} name=cls",
                 " ! gvametaconvert name=metaconvert ! appsink name=appsink"],
    "description": "device_rois_ab: detection + ROI classification",
    "parameters": {"type": "object", "properties": {}},
}


def quantiles(v):
    v = sorted(v)
    return {"median_us": round(v[len(v) // 2], 2), "p10_us": round(v[len(v) // 10], 2),
            "p90_us": round(v[(9 * len(v)) // 10], 2)}


def time_route(torch, fn, sets, warmup, steps):
    for k in range(warmup):
        fn(k % sets)
    torch.cuda.synchronize()
    dev, host = [], []
    for t in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn(t % sets)
        host.append((time.perf_counter() - t0) * 1e6)
        b.record()
        torch.cuda.synchronize()  # one launch at a time
        dev.append(a.elapsed_time(b) * 1e3)
    return {"launch": quantiles(dev), "host_call": quantiles(host), "steps": steps}


def pipeline_rate(evam, torch, dev, device_rois, streams, frames, dets):
    ps = evam.pipeline_server
    tmp = tempfile.mkdtemp(prefix="evam_device_rois_ab_")
    pdir = os.path.join(tmp, "pipelines", "detect_classify", "ab")
    os.makedirs(pdir)
    json.dump(PIPE, open(os.path.join(pdir, "pipeline.json"), "w"))
    for net, (w, h), proc in (("ab_detector", (64, 64), {"input_preproc": [], "output_postproc": [{"labels": ["bg", "car"]}]}),
                              ("ab_classifier", (72, 72), {"input_preproc": [{"format": "image", "params": {"range": [0, 1]}}],
                                                           "output_postproc": [{"layer_name": "color", "attribute_name": "color",
                                                                                "labels": ["dark", "light"]}]})):
        mdir = os.path.join(tmp, "models", net, "1")
        os.makedirs(os.path.join(mdir, "FP32"))
        open(os.path.join(mdir, "FP32", f"{net}.xml"), "w").write(bench.IR_STUB.format(w=w, h=h))
        json.dump(proc, open(os.path.join(mdir, f"{net}.json"), "w"))
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    xy = torch.rand((64, dets, 2), device=dev, generator=gen) * 0.7
    wh = torch.rand((64, dets, 2), device=dev, generator=gen) * 0.2 + 0.05
    table = torch.cat([torch.zeros((64, dets, 1), device=dev), torch.ones((64, dets, 1), device=dev),
                       torch.full((64, dets, 1), 0.9, device=dev), xy, xy + wh], 2).contiguous()
    cap = 64 * dets
    ps.PipelineServer.start({"pipeline_dir": os.path.join(tmp, "pipelines"), "model_dir": os.path.join(tmp, "models"),
                             "batch_max": 64, "batch_target": 64, "batch_wait_ms": 1.0, "device_rois": device_rois,
                             "device_rois_cap": cap})
    try:
        ps.PipelineServer.register_model("ab_detector/1", ps.InferenceModel(lambda t: table[:t.shape[0]], (64, 64), name="det"))
        ps.PipelineServer.register_model("ab_classifier/1", ps.InferenceModel(
            lambda t: {"color": t[:, 0, 0, :2].contiguous()}, (72, 72), name="cls", out_dtype="f32"))
        wl = bench.WORKLOADS["c3"]
        pool = bench.device_frames(evam, torch, wl, 64, dev, seed=9)
        qs = []
        for k in range(streams):
            q = queue.Queue()
            for t in range(frames):
                q.put(pool[(k + t) % len(pool)])
            q.put(None)
            qs.append(q)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipes = []
        for k in range(streams):
            p = ps.PipelineServer.pipeline("detect_classify", "ab")
            p.start(source={"type": "application", "input": qs[k]}, destination={}, parameters={})
            pipes.append(p)
        for p in pipes:
            st = p.wait(600)
            assert st["state"] == "COMPLETED", st
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        hub = ps.PipelineServer.hub(0)
        fused = sum(1 for e in hub.fused_batches if e["fused"])
        return {"device_rois": device_rois, "streams": streams, "frames": streams * frames, "dets_per_frame": dets,
                "seconds": round(el, 3), "frames_per_s": round(streams * frames / el, 1),
                "rois_per_s": round(streams * frames * dets / el, 1), "batches": len(hub.batches),
                "fused_batches": fused, "cap": cap}
    finally:
        ps.PipelineServer.stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true", help="H only (API of a library without the device-list calls)")
    ap.add_argument("--pipeline", action="store_true", help="also detect -> classify through the pipeline server")
    ap.add_argument("--parent", default="", help="a --baseline result of the parent's library, merged into --out")
    ap.add_argument("--sets", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames", type=int, default=256, help="frames per stream of the pipeline runs")
    ap.add_argument("--dets", type=int, default=8, help="detections per frame of the pipeline runs")
    ap.add_argument("--build-seconds", default="", help="tree,parent build() seconds to record")
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default=os.environ.get("EVAM_SHA", "unknown"))
    a = ap.parse_args()
    if a.sets < 5 or a.steps < 100 or a.warmup < 10:
        ap.error("--sets >= 5, --steps >= 100, --warmup >= 10")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("device_rois_ab.py needs a GPU")
    import __graft_entry__ as g

    evam = g.import_package()
    N = evam.native
    dev = torch.device("cuda:0")
    src_dir = os.path.join(ROOT, "edge-video-analytics-microservice_amd", "csrc")
    sha = hashlib.sha256(b"".join(open(os.path.join(src_dir, f), "rb").read() for f in sorted(os.listdir(src_dir))
                                  if f.endswith((".hip", ".h")))).hexdigest()[:16]
    result = {"tool": "tools/device_rois_ab.py", "git_head": a.head, "kernel_src_sha16": sha, "baseline": a.baseline,
              "library": os.environ.get("EVAM_PP_LIB", "libevam_pp.so"), "sets": a.sets, "warmup": a.warmup, "rows": []}
    wl = bench.WORKLOADS["c3"]
    n, (DW, DH) = wl["frames"], wl["dst"]
    frames = [evam.ImageBatch(bench.device_frames(evam, torch, wl, n, dev, seed=100 + k)) for k in range(a.sets)]
    rects = [np.array(bench.seed_rois(wl["rois"], n, *wl["src"], seed=k), dtype=np.int32) for k in range(a.sets)]
    rois = [evam.RoiBatch(r) for r in rects]
    items = len(rois[0])
    info = bench.make_info(evam, wl)
    pp = evam.HipPreProcessor(device=0)
    routes = [("H", items, lambda k, o: pp.convert(frames[k], o[k], info, rois=rois[k]))]
    if not a.baseline:
        for cap in (items, 2048):
            lists = [evam.DeviceRoiList(cap, device=dev).set(r) for r in rects]
            routes.append((f"D{cap}", cap, lambda k, o, lists=lists: pp.convert(frames[k], o[k], info, rois=lists[k])))
    for name, rows, fn in routes:
        outs = [torch.empty((rows, 3, DH, DW), dtype=torch.float32, device=dev) for _ in range(a.sets)]
        r = time_route(torch, lambda k: fn(k, outs), a.sets, a.warmup, a.steps)
        row = {"route": name, "rois": items, "rows": rows, **r, "kernels": int(pp.stats().kernels)}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        del outs
        torch.cuda.empty_cache()
    pp.close()
    del frames
    torch.cuda.empty_cache()
    assert all(r["kernels"] == N.KERNEL_ROI for r in result["rows"])
    if a.pipeline and not a.baseline:
        result["pipeline"] = []
        for on in (False, True):
            row = pipeline_rate(evam, torch, dev, on, a.streams, a.frames, a.dets)
            result["pipeline"].append(row)
            print(json.dumps(row), flush=True)
    if a.parent:
        par = json.load(open(a.parent))
        result["parent"] = {k: par[k] for k in ("git_head", "kernel_src_sha16", "library", "rows")}
        ph = next(r for r in par["rows"] if r["route"] == "H")["launch"]
        th = next(r for r in result["rows"] if r["route"] == "H")["launch"]
        result["verdict"] = {"parent_H": ph, "tree_H": th,
                             "tree_H_within_parent_p10_p90": ph["p10_us"] <= th["median_us"] <= ph["p90_us"],
                             "tree_H_not_above_parent_p90": th["median_us"] <= ph["p90_us"]}
        print(json.dumps(result["verdict"]), flush=True)
    if a.build_seconds:
        t, p = a.build_seconds.split(",")
        result["build_seconds"] = {"tree": float(t), "parent": float(p)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
