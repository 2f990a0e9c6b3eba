#!/usr/bin/env python3
"""detect -> track -> classify ticks with ``reclassify-interval`` 1 and 4, server option ``device_rois`` off and on
(diagnostic, needs the GPU).

Workload: the C3 shape of ``bench.WORKLOADS`` through the pipeline server — ``--streams`` (32) streams of 1080p NV12
frames from a device-resident pool, one frame of every stream per tick; a synthetic detector that answers on the device
with ``--dets`` (50) boxes per frame (64x64 input) which drift up to three pixels per frame, so the tracker keeps their
ids; a classifier stub on 72x72 fp32 crops. Per (interval, device_rois) it reports the tick time (wall clock over the
whole run / ticks), the classifier rows per tick (the crops actually pre-processed and classified), how many batches
ran fused, and whether every tick held every stream.

``--tree DIR`` runs the package of another checkout (built there) with this same file, so one session measures the
parent commit beside the tree: at the parent gvatrack is not a stage (no ids: every region is classified on every
frame) and a ``reclassify-interval`` above 1 is not fused.

  python tools/device_track_ab.py --tree ../parent --out profiles/x_parent.json
  python tools/device_track_ab.py --parent profiles/x_parent.json --out profiles/device_track_ab.json

``--only on:4`` runs one variant (for a ``rocprofv3 --kernel-trace --stats`` run of its own; ``--kernel-stats CSV``
merges the ``evam_pp_track*`` and ``evam_pp_roi*`` rows of its kernel_stats file into ``--out``).
"""
import argparse
import csv
import hashlib
import json
import os
import queue
import sys
import tempfile
import time

PIPE = {
    "type": "GStreamer",
    "template": ["{auto_source} ! decodebin",
                 " ! gvadetect model={models[ab_detector][1][network]} name=det",
                 " ! gvatrack name=trk",
                 " ! gvaclassify model={models[ab_classifier][1][network]} name=cls",
                 " ! gvametaconvert name=metaconvert ! appsink name=appsink"],
    "description": "device_track_ab: detection + tracking + ROI classification",
    "parameters": {"type": "object", "properties": {"reclassify-interval": {"element": "cls", "type": "integer"}}},
}


def run_variant(evam, bench, torch, dev, device_rois, interval, streams, frames, dets, cap):
    ps = evam.pipeline_server
    tmp = tempfile.mkdtemp(prefix="evam_device_track_ab_")
    pdir = os.path.join(tmp, "pipelines", "detect_track_classify", "ab")
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
    # row i of a tick's batch is stream i (every tick holds one frame of every stream, in one order): its boxes start at
    # xy[i] and move by vel[i] per tick, at most 3 px of 1920 x 1080 per frame, and stay inside the frame for 400 ticks
    xy = torch.rand((streams, dets, 2), device=dev, generator=gen) * 0.25 + 0.3
    wh = torch.rand((streams, dets, 2), device=dev, generator=gen) * 0.12 + 0.04
    vel = (torch.rand((streams, dets, 2), device=dev, generator=gen) * 2 - 1) * torch.tensor([3 / 1920, 3 / 1080], device=dev)
    head = torch.cat([torch.zeros((streams, dets, 1), device=dev), torch.ones((streams, dets, 1), device=dev),
                      torch.full((streams, dets, 1), 0.9, device=dev)], 2)
    calls, rows, sizes = [0], [0], []

    def detector(t):
        p = xy + vel * float(calls[0])
        calls[0] += 1
        sizes.append(int(t.shape[0]))
        return torch.cat([head, p, p + wh], 2)[:t.shape[0]].contiguous()

    def classifier(t):
        rows[0] += int(t.shape[0])
        return {"color": t[:, 0, 0, :2].contiguous()}

    ps.PipelineServer.start({"pipeline_dir": os.path.join(tmp, "pipelines"), "model_dir": os.path.join(tmp, "models"),
                             "batch_max": streams * dets, "batch_target": streams, "batch_wait_ms": 2000.0,
                             "device_rois": device_rois, "device_rois_cap": cap})
    try:
        ps.PipelineServer.register_model("ab_detector/1", ps.InferenceModel(detector, (64, 64), name="det"))
        ps.PipelineServer.register_model("ab_classifier/1", ps.InferenceModel(classifier, (72, 72), name="cls",
                                                                              out_dtype="f32"))
        wl = bench.WORKLOADS["c3"]
        pool = bench.device_frames(evam, torch, wl, 64, dev, seed=9)
        qs = [queue.Queue() for _ in range(streams)]
        pipes = []
        for k in range(streams):
            p = ps.PipelineServer.pipeline("detect_track_classify", "ab")
            p.start(source={"type": "application", "input": qs[k]}, destination={},
                    parameters={"reclassify-interval": interval})
            pipes.append(p)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(frames):
            # frame t of every stream once tick t - 1 is launched (its detector was called): a tick holds one frame of
            # every stream, and the next one is queued while the device still runs this one
            while calls[0] < t:
                if time.perf_counter() - t0 > 300 or any(p.status()["state"] == "ERROR" for p in pipes):
                    raise RuntimeError(f"tick {t} never launched: {[p.status() for p in pipes][:2]}")
                time.sleep(0.0001)
            for k in range(streams):
                qs[k].put(pool[(k + t) % len(pool)])
        for q in qs:
            q.put(None)
        for p in pipes:
            st = p.wait(600)
            assert st["state"] == "COMPLETED", st
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        hub = ps.PipelineServer.hub(0)
        fused = [e for e in hub.fused_batches if e["fused"]]
        ticks = len(sizes)
        # a fused batch classifies its list's count (the tensor has cap rows); the host path the rows the stub saw
        n_rows = sum(min(e["count"], e["cap"]) for e in fused) + (rows[0] - len(fused) * cap if fused else rows[0])
        return {"device_rois": device_rois, "reclassify_interval": interval, "streams": streams, "ticks": ticks,
                "every_tick_full": all(s == streams for s in sizes), "dets_per_frame": dets, "seconds": round(el, 3),
                "tick_ms": round(el / ticks * 1e3, 3), "frames_per_s": round(streams * frames / el, 1),
                "classifier_rows_per_tick": round(n_rows / ticks, 1), "fused_batches": len(fused),
                "batches": len(hub.batches), "cap": cap}
    finally:
        ps.PipelineServer.stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="", help="the checkout whose package runs (default: this file's)")
    ap.add_argument("--parent", default="", help="a result of the parent's tree, merged into --out")
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames", type=int, default=120, help="frames per stream")
    ap.add_argument("--dets", type=int, default=50)
    ap.add_argument("--cap4", type=int, default=640, help="device_rois_cap of the interval-4 runs (interval 1: streams x dets)")
    ap.add_argument("--only", default="", help="one variant, e.g. on:4")
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 kernel_stats.csv to merge (tracker and ROI kernels)")
    ap.add_argument("--out", default="")
    ap.add_argument("--head", default=os.environ.get("EVAM_SHA", "unknown"))
    a = ap.parse_args()
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch

    if not torch.cuda.is_available():
        sys.exit("device_track_ab.py needs a GPU")
    import __graft_entry__ as g
    import bench

    evam = g.import_package()
    assert os.path.dirname(os.path.abspath(g.__file__)) == root, g.__file__
    dev = torch.device("cuda:0")
    src_dir = os.path.join(root, "edge-video-analytics-microservice_amd", "csrc")
    sha = hashlib.sha256(b"".join(open(os.path.join(src_dir, f), "rb").read() for f in sorted(os.listdir(src_dir))
                                  if f.endswith((".hip", ".h")))).hexdigest()[:16]
    result = {"tool": "tools/device_track_ab.py", "git_head": a.head, "kernel_src_sha16": sha,
              "has_gvatrack": "gvatrack" in evam.pipeline_server.STAGES, "rows": []}
    variants = [(on, iv) for iv in (1, 4) for on in (False, True)]
    if a.only:
        on, iv = a.only.split(":")
        variants = [(on == "on", int(iv))]
    run_variant(evam, bench, torch, dev, True, 1, a.streams, 10, a.dets, a.streams * a.dets)  # warm-up, not reported
    for on, iv in variants:
        row = run_variant(evam, bench, torch, dev, on, iv, a.streams, a.frames, a.dets,
                          a.streams * a.dets if iv == 1 else a.cap4)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.kernel_stats:
        keep = [r for r in csv.DictReader(open(a.kernel_stats)) if any(k in r.get("Name", "") for k in ("evam_pp_track", "evam_pp_roi", "evam_pp_ssd"))]
        result["kernel_stats"] = keep
    if a.parent:
        par = json.load(open(a.parent))
        result["parent"] = {k: par[k] for k in ("git_head", "kernel_src_sha16", "has_gvatrack", "rows")}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
