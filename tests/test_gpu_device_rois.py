"""Device-resident ROI lists on the GPU: ``evam_pp_ssd_rois`` against its host twin, and ``evam_pp_run_device_rois``
(``HipPreProcessor.convert(..., rois=<DeviceRoiList>)``) bit-exact against the host-list ``convert`` of the same rects
and against the C oracle. Frames are at most 352x198; outputs are 24x24 and 72x72 (one unit per entry) and 256x160
(three row tiles per entry)."""
import json
import queue
import zlib

import numpy as np
import pytest

import device_rois_cases as C
import source_layouts as SL
from test_pipeline_server import PIPES, model_dir, ps  # noqa: F401  (fixtures of the pipeline-server tests)
from test_gpu_half import half_full, narrow_bits, same_bits
from test_gpu_parity import FORMATS, assert_same, fc, run_oracle, upload

pytestmark = pytest.mark.gpu

NORM = {"range": (0.0, 1.0), "mean": (0.406, 0.456, 0.485), "std": (0.225, 0.224, 0.229)}
SRC_SIZES = [(352, 198), (320, 180), (64, 48)]
RESIZES = {"plain": dict(resize="no-aspect-ratio"), "letterbox": dict(resize="aspect-ratio", placement="center"),
           "crop": dict(resize="aspect-ratio", crop="central")}
SENTINEL = 7


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def make_frames(O, rng, fmt, sizes=SRC_SIZES):
    return [O.random_frame(rng, fc(O, fmt), w, h, pitch_align=64) for w, h in sizes]


def make_rects(rng, sizes, n):
    """n rects over the sources, every one with a non-empty intersection: partly outside on each side, 1x1, whole
    frames, odd origins and sizes."""
    out = []
    for j in range(n):
        si = j % len(sizes)
        W, H = sizes[si]
        kind = j % 8
        if kind == 0:
            r = (0, 0, W, H)
        elif kind == 1:
            r = (int(rng.integers(0, W)), int(rng.integers(0, H)), 1, 1)
        elif kind == 2:   # over the left / top edge
            r = (-int(rng.integers(1, 20)), -int(rng.integers(1, 20)), int(rng.integers(25, W)), int(rng.integers(25, H)))
        elif kind == 3:   # over the right / bottom edge
            x, y = int(rng.integers(W // 2, W - 1)), int(rng.integers(H // 2, H - 1))
            r = (x, y, W, H)
        else:             # inside, odd origins and sizes as they fall
            w, h = int(rng.integers(2, W // 2)), int(rng.integers(2, H // 2))
            r = (int(rng.integers(0, W - w)) | (j & 1), int(rng.integers(0, H - h)) | (j & 1), w | 1, h | 1)
        out.append((si,) + r)
    return out


def make_info(evam, out, resize, rgb):
    return evam.PreProcInfo(color_space="RGB" if rgb else "BGR", fill=(5, 50, 250),
                            precision="FP16" if out == "f16" else None, **RESIZES[resize],
                            **(NORM if out != "u8" else {}))


def sentinel_out(torch, out, shape, gpu):
    if out == "f16":
        return half_full(torch, shape, "f16", gpu, value=SENTINEL)
    return torch.full(shape, SENTINEL, dtype=torch.uint8 if out == "u8" else torch.float32, device=gpu)


def compare(torch, out, got, ref, what):
    if out == "f16":
        same_bits(torch, got, narrow_bits(torch, ref, "f16"), what)
    else:
        assert_same(got.cpu().numpy(), ref, what)


def oracle_ref(O, coracle, frames, shape, out, info, rects, slot_offset=0, slot_stride=1):
    ref, _ = run_oracle(O, coracle, frames, shape, "u8" if out == "u8" else "f32", info, rois=rects,
                        slot_offset=slot_offset, slot_stride=slot_stride, init=SENTINEL)
    return ref


def device_list(evam, torch, gpu, rects, cap):
    lst = evam.DeviceRoiList(cap, device=gpu)
    lst.rois.fill_(-3)
    return lst.set(np.asarray(rects, np.int32).reshape(-1, 5))


# ---- evam_pp_ssd_rois ----------------------------------------------------------------------------------------------

def run_ssd(evam, torch, gpu, pp, b, cap):
    frames = [evam.Image(evam.native.FOURCC_NV12, w, h, []) for w, h in b.sizes]
    lst = evam.DeviceRoiList(cap, device=gpu)
    lst.rois.fill_(-3)
    lst.count.fill_(-1)
    det = torch.from_numpy(b.det).to(gpu)
    got = pp.detections_to_rois(det, frames, b.xf, b.tensor, b.threshold, b.labels, lst)
    assert got is lst
    torch.cuda.synchronize()
    return lst.rois.cpu().numpy(), int(lst.count.cpu().numpy().view(np.uint32)[0])


def test_ssd_rois_device_equals_host(evam, gpu):
    import torch

    pp = evam.HipPreProcessor(device=0)
    try:
        cases = [(c, None) for c in C.CASES] + [((65, 1024, "mixed", None), None), ((65, 1024, "none", (0, 5)), None),
                                               ((8, 50, "mixed", None), 7), ((3, 200, "none", None), 1)]
        total = 0
        for case, cap in cases:
            n, K, kind, labels = case
            b = C.make_batch(evam, seed_of("ssd", case), n, K, kind, labels)
            want, count = C.host_rois(evam, b)
            room = cap if cap is not None else n * K
            rois, got_count = run_ssd(evam, torch, gpu, pp, b, room)
            what = f"{C.case_id(case)} cap {room}"
            assert got_count == count, f"{what}: count {got_count}, host {count}"
            m = min(count, room)
            assert np.array_equal(rois[:m], want[:m]), what
            assert (rois[m:] == -3).all(), f"{what}: entries past the count were written"
            if cap is not None:
                assert count > cap, f"{what}: the case was meant to overflow"
            total += count
        assert total > 1000
        # no detection at all: count 0, the list buffer keeps its sentinel; [n, 1, K, 7] is taken as [n, K, 7]
        b = C.make_batch(evam, 3, 5, 20)
        b.det[:, :, 2] = 0.0
        rois, got_count = run_ssd(evam, torch, gpu, pp, b, 16)
        assert got_count == 0 and (rois == -3).all()
        b = C.make_batch(evam, 4, 5, 20, "mixed")
        lst = pp.detections_to_rois(torch.from_numpy(b.det[:, None]).to(gpu),
                                    [evam.Image(evam.native.FOURCC_BGR, w, h, []) for w, h in b.sizes], b.xf, b.tensor,
                                    b.threshold)
        torch.cuda.synchronize()
        want, count = C.host_rois(evam, b)
        assert int(lst.count.cpu()[0]) == count > 0 and np.array_equal(lst.rois.cpu().numpy()[:count], want)
    finally:
        pp.close()


# ---- evam_pp_run_device_rois -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("resize", list(RESIZES))
@pytest.mark.parametrize("out", ["u8", "f32", "f16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_device_list_convert_bit_exact(evam, O, coracle, gpu, fmt, out, resize):
    import torch

    rng = np.random.default_rng(seed_of("exact", fmt, out, resize))
    frames = make_frames(O, rng, fmt)
    imgs = upload(evam, frames, gpu)
    rgb = (FORMATS.index(fmt) + ["u8", "f32", "f16"].index(out) + list(RESIZES).index(resize)) % 2 == 1
    info = make_info(evam, out, resize, rgb)
    pp = evam.HipPreProcessor(device=0)
    try:
        # (output size, rects, cap, slot offset, slot stride); 256x160 is three row tiles per entry; 75x40 is an odd
        # width: one pixel per lane (evam_pp_roi<.., 1, 2, DEV>), where every even width takes two
        plans = [((24, 24), 40, 48, 1, 2), ((72, 72), 40, 48, 0, 1)]
        if resize == "plain":
            plans += [((256, 160), 9, 12, 2, 1), ((75, 40), 3, 4, 0, 1)]
        for (DW, DH), n, cap, off, stride in plans:
            rects = make_rects(rng, SRC_SIZES, n)
            shape = (off + cap * stride, 3, DH, DW)
            what = f"{fmt} {out} {resize} {'RGB' if rgb else 'BGR'} -> {DW}x{DH} slots {off}+{stride}i"
            ref = oracle_ref(O, coracle, frames, shape, out, info, rects, off, stride)
            host = sentinel_out(torch, out, shape, gpu)
            pp.convert(imgs, host, info, rois=np.asarray(rects, np.int32), slot_offset=off, slot_stride=stride)
            got = sentinel_out(torch, out, shape, gpu)
            status = torch.full((cap,), 99, dtype=torch.int32, device=gpu)
            lst = device_list(evam, torch, gpu, rects, cap)
            assert pp.convert(imgs, got, info, rois=lst, slot_offset=off, slot_stride=stride, status=status) is None
            torch.cuda.synchronize()
            st = pp.stats()
            assert st.kernels == evam.native.KERNEL_ROI and st.n_items == cap, what
            compare(torch, out, got, ref, what + " (device list vs oracle)")  # the whole tensor: sentinels included
            assert torch.equal(got.view(torch.uint8), host.view(torch.uint8)), what + " (device list vs host list)"
            assert (status == 0).all(), what
    finally:
        pp.close()


def test_invalid_entries_are_skipped(evam, O, coracle, gpu):
    import torch

    N = evam.native
    rng = np.random.default_rng(21)
    frames = make_frames(O, rng, "NV12")
    imgs = upload(evam, frames, gpu)
    info = make_info(evam, "f32", "letterbox", False)
    good = make_rects(rng, SRC_SIZES, 12)
    rects = list(good)
    bad = {2: ((0, 400, 10, 8, 8), N.ERR_EMPTY_ROI), 5: ((3, 0, 0, 16, 16), N.ERR_INVALID_ARG),
           6: ((-1, 0, 0, 16, 16), N.ERR_INVALID_ARG), 9: ((1, -50, -50, 50, 50), N.ERR_EMPTY_ROI),
           11: ((2, 10, 48, 5, 5), N.ERR_EMPTY_ROI)}
    for i, (r, _) in bad.items():
        rects[i] = r
    pp = evam.HipPreProcessor(device=0)
    try:
        for DW, DH in ((72, 72), (256, 160)):
            cap = 16
            shape = (cap, 3, DH, DW)
            ref = oracle_ref(O, coracle, frames, shape, "f32", info, [r for i, r in enumerate(rects) if i not in bad])
            want = np.full(shape, SENTINEL, np.float32)
            want[[i for i in range(len(rects)) if i not in bad]] = ref[:len(rects) - len(bad)]
            got = sentinel_out(torch, "f32", shape, gpu)
            status = torch.full((cap,), 99, dtype=torch.int32, device=gpu)
            pp.convert(imgs, got, info, rois=device_list(evam, torch, gpu, rects, cap), status=status)
            torch.cuda.synchronize()
            st = status.cpu().numpy()
            for i in range(cap):
                assert st[i] == (bad[i][1] if i in bad else 0), f"status[{i}] = {st[i]}"
            assert_same(got.cpu().numpy(), want, f"{DW}x{DH}: invalid entries skipped, every other slot exact")
    finally:
        pp.close()


def test_count_zero_and_cap_one(evam, O, coracle, gpu):
    import torch

    rng = np.random.default_rng(22)
    frames = make_frames(O, rng, "I420")
    imgs = upload(evam, frames, gpu)
    info = make_info(evam, "u8", "plain", True)
    pp = evam.HipPreProcessor(device=0)
    try:
        got = sentinel_out(torch, "u8", (6, 3, 24, 24), gpu)
        status = torch.full((6,), 99, dtype=torch.int32, device=gpu)
        pp.convert(imgs, got, info, rois=evam.DeviceRoiList(6, device=gpu), status=status)  # count 0
        torch.cuda.synchronize()
        assert (got == SENTINEL).all() and (status == 0).all()
        rect = [(1, 31, 17, 101, 55)]
        ref = oracle_ref(O, coracle, frames, (1, 3, 24, 24), "u8", info, rect)
        got = sentinel_out(torch, "u8", (1, 3, 24, 24), gpu)
        pp.convert(imgs, got, info, rois=device_list(evam, torch, gpu, rect, 1))
        torch.cuda.synchronize()
        assert_same(got.cpu().numpy(), ref, "cap 1")
        # a count above the capacity (an overflowing producer): the first cap entries, nothing else
        lst = device_list(evam, torch, gpu, make_rects(rng, SRC_SIZES, 4), 4)
        rects = lst.rois.cpu().numpy().tolist()
        lst.count.fill_(1000)
        ref = oracle_ref(O, coracle, frames, (5, 3, 24, 24), "u8", info, [tuple(r) for r in rects])
        got = sentinel_out(torch, "u8", (5, 3, 24, 24), gpu)
        pp.convert(imgs, got, info, rois=lst)
        torch.cuda.synchronize()
        assert_same(got.cpu().numpy(), ref, "count above cap")
    finally:
        pp.close()


def test_calls_in_flight(evam, O, coracle, gpu):
    """24 calls with new lists and outputs on three handles, each on its own stream, with no host synchronisation
    between them: the handle-owned record buffer and source table are reused safely. Each output equals the same call
    run alone."""
    import torch

    rng = np.random.default_rng(23)
    fmts = ["NV12", "BGRX", "I420"]
    frames = {f: make_frames(O, rng, f) for f in fmts}
    imgs = {f: upload(evam, frames[f], gpu) for f in fmts}
    pps = [evam.HipPreProcessor(device=0) for _ in fmts]
    streams = [torch.cuda.Stream(device=gpu) for _ in fmts]
    calls = []
    for j in range(24):
        h = j % 3
        out = ["u8", "f32"][(j // 3) % 2]
        DW, DH = [(24, 24), (72, 72), (256, 160)][(j // 6) % 3]
        n, cap = (5, 8) if DW == 256 else (int(rng.integers(1, 30)), 32)
        calls.append((h, out, (DW, DH), make_rects(rng, SRC_SIZES, n), cap,
                      make_info(evam, out, list(RESIZES)[j % 3], j % 2 == 1)))
    torch.cuda.synchronize()
    try:
        keep, outs = [], []
        for h, out, (DW, DH), rects, cap, info in calls:
            with torch.cuda.stream(streams[h]):
                lst = device_list(evam, torch, gpu, rects, cap)
                got = sentinel_out(torch, out, (cap, 3, DH, DW), gpu)
                pps[h].convert(imgs[fmts[h]], got, info, rois=lst)
            keep.append(lst)
            outs.append(got)
        torch.cuda.synchronize()
        alone = evam.HipPreProcessor(device=0)
        try:
            for j, (h, out, (DW, DH), rects, cap, info) in enumerate(calls):
                want = sentinel_out(torch, out, (cap, 3, DH, DW), gpu)
                alone.convert(imgs[fmts[h]], want, info, rois=device_list(evam, torch, gpu, rects, cap))
                torch.cuda.synchronize()
                assert torch.equal(outs[j], want), f"call {j} ({fmts[h]} {out} {DW}x{DH}, {len(rects)} rects)"
                if j < 3:  # ... and that call is the oracle's
                    ref = oracle_ref(O, coracle, frames[fmts[h]], (cap, 3, DH, DW), out, info, rects)
                    compare(torch, out, want, ref, f"call {j} alone")
        finally:
            alone.close()
    finally:
        for p in pps:
            p.close()


def test_refusals(evam, O, coracle, gpu):
    import torch

    N = evam.native
    rng = np.random.default_rng(24)
    frames = make_frames(O, rng, "NV12")
    imgs = upload(evam, frames, gpu)
    other = upload(evam, make_frames(O, rng, "BGRX", [(64, 48)]), gpu)
    info = make_info(evam, "u8", "plain", False)
    rects = make_rects(rng, SRC_SIZES, 6)
    pp = evam.HipPreProcessor(device=0)
    try:
        def refused(status, srcs, out, lst):
            before = out.clone()
            with pytest.raises(evam.PreProcError) as e:
                pp.convert(srcs, out, info, rois=lst)
            torch.cuda.synchronize()
            assert e.value.status == status, str(e.value)
            assert torch.equal(out, before), "a refused call wrote to the output"

        lst = device_list(evam, torch, gpu, rects, 8)
        plain = sentinel_out(torch, "u8", (8, 3, 24, 24), gpu)
        refused(N.ERR_UNSUPPORTED, imgs + other, plain, lst)                      # two fourccs
        nhwc = torch.full((8, 3, 24, 24), SENTINEL, dtype=torch.uint8, device=gpu).contiguous(
            memory_format=torch.channels_last)
        refused(N.ERR_UNSUPPORTED, imgs, nhwc, lst)                               # interleaved output
        wide = sentinel_out(torch, "u8", (8, 3, 2, 1540), gpu)
        refused(N.ERR_UNSUPPORTED, imgs, wide, lst)                               # no ROI-kernel plan for this width
        with pytest.raises(evam.PreProcError) as e:
            evam.DeviceRoiList(0, device=gpu)
        assert e.value.status == N.ERR_INVALID_ARG
        for field, value in (("cap", 0), ("cap", -4), ("rois", None), ("count", None)):
            broken = device_list(evam, torch, gpu, rects, 8)
            setattr(broken._c, field, value)                                      # what the C ABI itself answers
            refused(N.ERR_INVALID_ARG, imgs, plain, broken)
        lib = evam.load_library()
        assert lib.evam_pp_run_device_rois(pp._h, None, 0, None, None, None, None) == N.ERR_INVALID_ARG
        # the handle then runs a good call exactly
        ref = oracle_ref(O, coracle, frames, (8, 3, 24, 24), "u8", info, rects)
        pp.convert(imgs, plain, info, rois=lst)
        torch.cuda.synchronize()
        assert_same(plain.cpu().numpy(), ref, "a good call after the refusals")
    finally:
        pp.close()


@pytest.mark.parametrize("fmt", ["NV12", "I420"])
def test_source_layouts(evam, O, coracle, gpu, fmt):
    """Frames whose planes have their own pitches and bases (tests/source_layouts.py): the device-built records carry
    each plane's pitch from the per-source table."""
    import torch

    rng = np.random.default_rng(seed_of("layouts", fmt))
    frames = make_frames(O, rng, fmt)
    imgs, hosts = SL.lay_out_all(evam, torch, O, frames, ["unequal+base16", "window+reversed", "compact"], rng, gpu)
    info = make_info(evam, "f32", "crop", fmt == "I420")
    rects = make_rects(rng, SRC_SIZES, 24)
    pp = evam.HipPreProcessor(device=0)
    try:
        for DW, DH, n in ((72, 72, 24), (256, 160, 6)):
            shape = (n + 2, 3, DH, DW)
            ref = oracle_ref(O, coracle, hosts, shape, "f32", info, rects[:n])
            got = sentinel_out(torch, "f32", shape, gpu)
            pp.convert(imgs, got, info, rois=device_list(evam, torch, gpu, rects[:n], n + 2))
            torch.cuda.synchronize()
            assert_same(got.cpu().numpy(), ref, f"{fmt} laid-out planes -> {DW}x{DH}")
    finally:
        pp.close()


# ---- the pipeline server's "device_rois" option -----------------------------------------------------------------------

def run_detect_classify(ps, O, model_dir, frames, boxes, options, detector_on_device=True):
    """The detect -> classify pipeline of tests/pipelines over ``frames`` with the random detections ``boxes`` (the
    set-up of test_pipeline_server.test_end_to_end_random_detections_bit_exact): (JSON lines, the classifier's input
    tensors in call order, the hub's fused_batches, the hub's batches)."""
    import torch

    cls_in, seen = [], [0]

    def detector(t):
        n = t.shape[0]
        out = torch.full((n, 10, 7), -1.0)
        for i in range(n):
            for j, r in enumerate(boxes[seen[0] + i]):
                out[i, j] = torch.tensor([0.0] + r)
        seen[0] += n
        return out.to(t.device) if detector_on_device else out

    def classifier(t):
        cls_in.append(t.detach().float().cpu().numpy().copy())
        m = t[:, 0, 3, 5] * 0.5 + t[:, 2, 20, 11] * 0.25  # element-wise: a row's result does not depend on the batch
        return {"color": torch.stack([1 - m, m], 1)}

    ps.PipelineServer.start(dict({"pipeline_dir": PIPES, "model_dir": model_dir, "runner": "device", "batch_max": 4},
                                 **options))
    try:
        ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
        ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(classifier, (24, 24), name="cls"))
        qin, qout = queue.Queue(), queue.Queue()
        for f in frames:
            qin.put({"fourcc": f.fourcc, "width": f.width, "height": f.height, "planes": f.planes})
        qin.put(None)
        p = ps.PipelineServer.pipeline("detect_classify", "hip")
        p.start(source={"type": "application", "input": qin},
                destination={"metadata": {"type": "application", "output": qout, "mode": "json"}},
                parameters={"detection-properties": {"pre-process-backend": "hip"}})
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
        lines = []
        while True:
            x = qout.get(timeout=5)
            if x is None:
                break
            lines.append(json.loads(x))
        hub = ps.PipelineServer.hub(0)
        return lines, cls_in, [dict(e) for e in hub.fused_batches], list(hub.batches)
    finally:
        ps.PipelineServer.stop()


def test_pipeline_device_rois(ps, evam, model_dir, gpu, O, coracle):
    rng = np.random.default_rng(31)
    n_frames, W, H = 24, 352, 198
    frames = [O.random_frame(rng, O.NV12, W, H, pattern="gradient" if k % 3 == 0 else "uniform")
              for k in range(n_frames)]
    boxes = []  # per frame: [label, conf, x0, y0, x1, y1] rows (normalised); label 1 is `car`, the classified class
    for _ in range(n_frames):
        rows = []
        for _ in range(int(rng.integers(0, 9))):
            x0, y0 = rng.uniform(-0.1, 0.9, 2)
            x1, y1 = x0 + rng.uniform(0.01, 0.6), y0 + rng.uniform(0.01, 0.6)
            rows.append([float(rng.integers(1, 3)), float(rng.choice([0.9, 0.5, 0.3])), x0, y0, x1, y1])
        boxes.append(rows)
    off_lines, off_in, off_fused, off_batches = run_detect_classify(ps, O, model_dir, frames, boxes, {})
    assert len(off_lines) == n_frames and off_fused == []
    assert {b[0][0] for b in off_batches} == {"gvadetect", "gvaclassify"}

    on_lines, on_in, fused, batches = run_detect_classify(ps, O, model_dir, frames, boxes, {"device_rois": True})
    assert on_lines == off_lines, "the JSON lines differ with device_rois on"
    assert len(fused) == n_frames // 4 and all(e["fused"] and e["cap"] == 4 and e["reason"] is None for e in fused)
    assert {b[0][0] for b in batches} == {"detect+classify"}
    # the default cap (batch_max = 4) is below some ticks' detections here: a run with room for every region, whose
    # classifier rows below each count are the oracle's crops of the boxes the JSON reports, in order
    on_lines, on_in, fused, _ = run_detect_classify(ps, O, model_dir, frames, boxes,
                                                    {"device_rois": True, "device_rois_cap": 40})
    assert on_lines == off_lines
    assert all(e["fused"] and e["cap"] == 40 and e["count"] <= 40 for e in fused) and len(on_in) == len(fused)
    crops = [(k, o["x"], o["y"], o["w"], o["h"]) for k, d in enumerate(on_lines) for o in d.get("objects", [])
             if "color" in o]
    assert len(crops) > 10 and sum(e["count"] for e in fused) == len(crops)
    assert all(t.shape == (40, 3, 24, 24) for t in on_in)
    got = np.concatenate([t[:e["count"]] for t, e in zip(on_in, fused)])
    ref = np.zeros(got.shape, np.float32)
    lut1 = O.np_norm_lut(1, (0.0, 1.0))
    for i, (k, x, y, w, h) in enumerate(crops):
        coracle.preprocess_item(frames[k], (x, y, w, h), ref, i, color_rgb=True, lut=lut1)
    bad = [i for i in range(len(crops)) if not np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32))]
    assert not bad, f"classifier rows differ: {[(i, crops[i]) for i in bad[:5]]}"
    # ticks stay in flight (inflight 3): some batch was launched before the one before it completed
    assert any(b["launched"] < a["completed"] for a, b in zip(fused, fused[1:])), fused
    # overflow: a cap below one tick's detections; the regions beyond it take the host path, the JSON is equal
    over_lines, _, over, _ = run_detect_classify(ps, O, model_dir, frames, boxes,
                                                 {"device_rois": True, "device_rois_cap": 2})
    assert over_lines == off_lines and any(e["count"] > 2 for e in over) and all(e["fused"] for e in over)
    # a detector that answers on the CPU: today's path, recorded as such
    cpu_lines, _, cpu, _ = run_detect_classify(ps, O, model_dir, frames, boxes, {"device_rois": True},
                                               detector_on_device=False)
    assert cpu_lines == off_lines and len(cpu) == n_frames // 4
    assert all(not e["fused"] and "device" in e["reason"] for e in cpu)
