#!/usr/bin/env python3
"""JPEG encoding of the published frame, measured (bench.py is the flagship's yardstick and is not involved).

  python tools/jpeg_bench.py kernels     32 x 1080p NV12 frames of bench.device_frames at level 95: device time per
                                         evam_pp_encode_jpeg call by HIP events, bytes produced, the time of
                                         HipPreProcessor.encode_jpeg (device + copy + retries), and, where Pillow
                                         imports, the CPU time of Pillow encoding the same BGR frames on 16 threads.
                                         Per-stage times: run it under `rocprofv3 --kernel-trace --stats --` (the
                                         five evam_jpeg_* kernels and the export kernel appear by name).
  python tools/jpeg_bench.py pipeline --mode raw|jpeg
                                         bench.py --via pipeline's set-up with destination mode "publisher":
                                         32 streams, one frame each per tick, wall time per 32-frame tick. --mode raw
                                         uses nothing this tool's commit added, so the same file runs on the parent.

Each prints one JSON line."""
import argparse
import io
import json
import os
import queue
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402


def frames_for(evam, torch, content, n, device):
    wl = bench.WORKLOADS["c2"]
    imgs = bench.device_frames(evam, torch, wl, n, device, seed=7)
    if content == "smooth":  # a gradient plus a little noise: closer to camera frames than i.i.d. bytes
        for im in imgs:
            for p in im.planes:
                r, c = p.shape
                ramp = (torch.arange(c, device=device)[None, :] * 255 // c + torch.arange(r, device=device)[:, None] * 97 // r)
                p.copy_(((ramp % 256) + (p >> 5)).clamp_(0, 255).to(torch.uint8))
    return imgs


def kernels(args, evam, torch):
    dev = torch.device("cuda:0")
    N = evam.native
    out = {"what": "jpeg kernels", "frames": args.frames, "size": [1920, 1080], "level": args.level,
           "device": torch.cuda.get_device_name(0)}
    pp = evam.HipPreProcessor(device=0)
    stride = N.jpeg_bound(1920, 1080) if args.stride == "bound" else 1024 + 1920 * 1088
    buf = torch.empty((args.frames, stride), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(args.frames, dtype=torch.int32, device=dev)
    for content in ("noise", "smooth"):
        imgs = evam.ImageBatch(frames_for(evam, torch, content, args.frames, dev))
        for _ in range(args.warmup):
            pp.encode_jpeg_into(imgs, buf, sizes, args.level)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ev[0].record()
        for i in range(args.steps):
            pp.encode_jpeg_into(imgs, buf, sizes, args.level)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
        lens = sizes.cpu().numpy().astype(np.int64)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            files = pp.encode_jpeg(imgs, args.level)
        e2e = (time.perf_counter() - t0) / args.steps * 1e3
        r = {"device_ms_per_call_median": round(ms[len(ms) // 2], 3), "device_ms_min": round(ms[0], 3),
             "bytes_per_frame_mean": int(lens.mean()), "bytes_total": int(lens.sum()), "slot_stride": stride,
             "frames_over_default_slot": int((lens > 1024 + 1920 * 1088).sum()),
             "encode_jpeg_ms_per_call": round(e2e, 3), "raw_bytes_total": args.frames * 1920 * 1080 * 3}
        assert [len(f) for f in files] == lens.tolist()
        try:
            from concurrent.futures import ThreadPoolExecutor

            from PIL import Image

            bgr = pp.export_bgr(imgs).cpu().numpy()

            def enc(a):
                b = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(a[..., ::-1])).save(b, "JPEG", quality=args.level, subsampling=2)
                return b.getvalue()

            with ThreadPoolExecutor(16) as ex:
                list(ex.map(enc, bgr[:16]))
                t0 = time.perf_counter()
                ref = list(ex.map(enc, bgr))
                r["pillow_16_threads_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            r["equal_to_pillow"] = ref == files
        except ImportError:
            r["pillow_16_threads_ms"] = None
        out[content] = r
    pp.close()
    print(json.dumps(out))


def pipeline(args, evam, torch):
    ps = evam.pipeline_server
    wl = bench.WORKLOADS["c2"]
    tmp = tempfile.mkdtemp(prefix="evam_jpeg_bench_")
    pdir = os.path.join(tmp, "pipelines", "object_detection", "bench")
    os.makedirs(pdir)
    json.dump(bench.PIPE_TEMPLATE, open(os.path.join(pdir, "pipeline.json"), "w"))
    mdir = os.path.join(tmp, "models", "bench_detector", "1")
    os.makedirs(os.path.join(mdir, "FP32"))
    open(os.path.join(mdir, "FP32", "bench_detector.xml"), "w").write(bench.IR_STUB.format(w=512, h=512))
    json.dump({"input_preproc": []}, open(os.path.join(mdir, "bench_detector.json"), "w"))
    empty = torch.full((1, 1, 7), -1.0)
    S, F = args.streams, args.frames_per_stream
    ps.PipelineServer.start({"pipeline_dir": os.path.join(tmp, "pipelines"), "model_dir": os.path.join(tmp, "models"),
                             "device": 0, "batch_max": S, "batch_wait_ms": 1.0, "batch_target": S, "runner": "device"})
    ps.PipelineServer.register_model("bench_detector/1", ps.InferenceModel(
        lambda t: empty.expand(t.shape[0], 1, 7), (512, 512), name="bench"))
    pool = frames_for(evam, torch, args.content, 2 * S, torch.device("cuda:0"))
    dst = {"type": "application", "mode": "publisher"}
    if args.mode == "jpeg":
        dst["encoding"] = {"type": "jpeg", "level": args.level}

    def run(n):
        qs, outs, pipes, got = [], [], [], [0] * S

        def drain(k, q):
            while (x := q.get()) is not None:
                got[k] += len(x[1])

        for k in range(S):
            q = queue.Queue()
            for t in range(n):
                q.put(pool[(k + t * S) % len(pool)])
            q.put(None)
            qs.append(q)
            outs.append(queue.Queue())
        threads = [threading.Thread(target=drain, args=(k, outs[k]), daemon=True) for k in range(S)]
        for t in threads:
            t.start()
        t0 = time.perf_counter()
        for k in range(S):
            p = ps.PipelineServer.pipeline("object_detection", "bench")
            p.start(source={"type": "application", "input": qs[k]}, destination={"metadata": dict(dst, output=outs[k])},
                    parameters={"detection-properties": {"batch-size": 1}})
            pipes.append(p)
        for p in pipes:
            st = p.wait(600)
            if st["state"] != "COMPLETED":
                raise RuntimeError(f"pipeline ended {st}")
        for t in threads:
            t.join(60)
        return time.perf_counter() - t0, sum(got)

    run(4)
    el, nbytes = run(F)
    ps.PipelineServer.stop()
    print(json.dumps({"what": "publisher pipeline", "mode": args.mode, "content": args.content, "level": args.level,
                      "streams": S, "frames_per_stream": F, "elapsed_s": round(el, 4),
                      "ms_per_32_frame_tick": round(el / (S * F / 32) * 1e3, 3), "frames_per_s": round(S * F / el, 1),
                      "published_bytes_per_frame": nbytes // (S * F), "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernels", "pipeline"])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--level", type=int, default=95)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stride", choices=["bound", "default"], default="bound")
    ap.add_argument("--mode", choices=["raw", "jpeg"], default="jpeg")
    ap.add_argument("--content", choices=["noise", "smooth"], default="noise")
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--frames-per-stream", type=int, default=24)
    args = ap.parse_args()
    import torch

    import __graft_entry__ as g

    evam = g.import_package()
    (kernels if args.what == "kernels" else pipeline)(args, evam, torch)


if __name__ == "__main__":
    main()
