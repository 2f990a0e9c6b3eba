#!/usr/bin/env python3
"""JPEG decoding of source frames, measured (bench.py is the flagship's yardstick and is not involved).

  python tools/jpeg_dec_bench.py [--files 32] [--steps 20] [--warmup 3] [--content noise|smooth]
                                 [--fourcc BGRX|NV12|I420]

The files are 1080p frames of bench.device_frames content, encoded by HipPreProcessor.encode_jpeg at quality 90.
--fourcc BGRX is libjpeg's default decode (evam_pp_decode_jpeg); NV12 / I420 are the files' raw 4:2:0 planes
(evam_pp_decode_jpeg_planes: five kernels, no component planes in scratch, no colour pass).
Measured for --files files per call and for one file alone:
  - device time per decode call and files/s, by HIP events around --steps calls launched back to back
    (launches in flight, as bench.py runs its steps);
  - host time per call (parse, staging copy, launches), from the wall clock of the launching loop;
  - HipPreProcessor.decode_jpeg (allocation, call, status read-back) per call;
  - the library's own host twin (evam_pp_decode_jpeg_host) on one core;
  - Pillow on 16 threads decoding the same files, where Pillow imports.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats --` (the evam_jdec_* kernels appear by name).
Prints one JSON line."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def make_files(evam, torch, pp, n, content, dev):
    imgs = bench.device_frames(evam, torch, bench.WORKLOADS["c2"], n, dev, seed=7)
    if content == "smooth":  # a gradient plus a little noise: closer to camera frames than i.i.d. bytes
        for im in imgs:
            for p in im.planes:
                r, c = p.shape
                ramp = (torch.arange(c, device=dev)[None, :] * 255 // c + torch.arange(r, device=dev)[:, None] * 97 // r)
                p.copy_(((ramp % 256) + (p >> 5)).clamp_(0, 255).to(torch.uint8))
    return pp.encode_jpeg(imgs, 90), imgs[0].width, imgs[0].height


def measure(evam, torch, pp, files, w, h, steps, warmup, dev, fourcc):
    n = len(files)
    imgs = evam.ImageBatch([evam.Image.alloc(fourcc, w, h, device=dev) for _ in range(n)])
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    for _ in range(warmup):
        pp.decode_jpeg_into(files, imgs, status)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        pp.decode_jpeg_into(files, imgs, status)
    host_us = (time.perf_counter() - t0) / steps * 1e6
    e1.record()
    torch.cuda.synchronize()
    assert not status.cpu().any()
    dev_us = e0.elapsed_time(e1) / steps * 1e3
    t0 = time.perf_counter()
    for _ in range(max(steps // 4, 1)):
        pp.decode_jpeg(files, fourcc)
    api_us = (time.perf_counter() - t0) / max(steps // 4, 1) * 1e6
    return {"files": n, "us_per_call": round(dev_us, 1), "files_per_s": round(n / dev_us * 1e6, 1),
            "host_us_per_call": round(host_us, 1), "decode_jpeg_us_per_call": round(api_us, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--content", choices=("noise", "smooth"), default="smooth")
    ap.add_argument("--fourcc", choices=("BGRX", "NV12", "I420"), default="BGRX")
    args = ap.parse_args()
    import torch

    import __graft_entry__ as g

    evam = g.import_package()
    dev = torch.device("cuda:0")
    pp = evam.HipPreProcessor(device=0)
    files, w, h = make_files(evam, torch, pp, args.files, args.content, dev)
    out = {"what": "jpeg decode", "fourcc": args.fourcc, "size": [w, h], "quality": 90, "content": args.content,
           "file_bytes_mean": int(sum(map(len, files)) / len(files)), "device": torch.cuda.get_device_name(0),
           "batch": measure(evam, torch, pp, files, w, h, args.steps, args.warmup, dev, args.fourcc),
           "single": measure(evam, torch, pp, files[:1], w, h, args.steps, args.warmup, dev, args.fourcc)}
    t0 = time.perf_counter()
    if args.fourcc == "BGRX":
        evam.native.decode_jpeg_host(files[:4])
    else:
        evam.native.decode_jpeg_planes_host(files[:4], evam.preproc.FOURCC_BY_NAME[args.fourcc])
    out["host_twin_one_core_files_per_s"] = round(4 / (time.perf_counter() - t0), 2)
    try:
        from PIL import Image

        def dec(f):
            return Image.open(io.BytesIO(f)).convert("RGB").tobytes()[:1]

        with ThreadPoolExecutor(16) as ex:
            list(ex.map(dec, files))
            t0 = time.perf_counter()
            for _ in range(3):
                list(ex.map(dec, files))
            out["pillow_16_threads_files_per_s"] = round(3 * len(files) / (time.perf_counter() - t0), 1)
    except ImportError:
        out["pillow_16_threads_files_per_s"] = None
    pp.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
