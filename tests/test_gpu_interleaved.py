"""Interleaved (NHWC) output against the CPU oracle's planar output, bit-exact.

A channels-last ``[N,3,H,W]`` tensor read back with ``.cpu().numpy()`` is logical NCHW, so it compares directly with
the planar oracle; every test also checks that the tensor's HWC view is contiguous, i.e. that the bytes really are
interleaved. Every output has one slot more than the call writes at each end: the call starts at ``slot_offset = 1``
into a tensor pre-filled with 7, and the first and last slots must still hold 7 afterwards (a wide store running past
a row or slot end lands there).
"""
import ctypes
import os
import queue
import re
import zlib

import numpy as np
import pytest

import bench
from test_gpu_fullsize import host_frames, oracle_items
from test_gpu_parity import FORMATS, assert_same, fc, random_case, run_oracle, upload
from test_gpu_plans import all_seven, expect_items
from test_pipeline_server import PIPES, make_model_tree

pytestmark = pytest.mark.gpu

NORM = {"range": (0.0, 1.0), "mean": (0.406, 0.456, 0.485), "std": (0.225, 0.224, 0.229)}


def tdtype(torch, dtype):
    return torch.float32 if dtype == "f32" else torch.uint8


def nhwc_full(torch, shape, dtype, device, value=7):
    """A channels-last [N,3,H,W] tensor filled with ``value``."""
    out = torch.empty(shape, dtype=tdtype(torch, dtype), device=device, memory_format=torch.channels_last)
    out.fill_(value)
    assert out.permute(0, 2, 3, 1).is_contiguous()
    return out


def check_nhwc(evam, torch, O, coracle, gpu, pp, frames, dst, dtype, info, rois=None, what="", imgs=None):
    """One interleaved call at slot_offset 1 into n + 2 slots of 7, the whole tensor against the planar oracle."""
    n = len(rois) if rois else len(frames)
    shape = (n + 2, 3, dst[1], dst[0])
    out = nhwc_full(torch, shape, dtype, gpu)
    pp.convert(imgs or upload(evam, frames, gpu), out, info, rois=[evam.Roi(*r) for r in rois] if rois else None,
               slot_offset=1)
    torch.cuda.synchronize()
    assert out.permute(0, 2, 3, 1).is_contiguous()
    ref, _ = run_oracle(O, coracle, frames, shape, dtype, info, rois=rois, slot_offset=1)
    got = out.cpu().numpy()
    assert (got[0] == 7).all() and (got[-1] == 7).all(), f"{what}: a guard slot was written"
    assert_same(got, ref, what)
    return pp.stats().kernels


@pytest.fixture(scope="module")
def pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("src,dst", [((64, 48), (512, 512)), ((66, 50), (33, 17)), ((96, 64), (96, 64)),
                                     ((64, 48), (1, 37)), ((64, 48), (1, 1)), ((2, 2), (40, 3)),
                                     ((200, 120), (300, 70)), ((200, 120), (600, 40)), ((640, 360), (520, 200))])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_full_frame(evam, O, coracle, gpu, pp, fmt, src, dst, dtype):
    """3 full frames, BGR and RGB: wide (512, 300, 600: the wave kernel and its tile edges), rows and slots on every
    residue mod 4 (33 x 17 u8: 99-byte rows, 1,683-byte slots; fp32 rows of 396 bytes), the identity (export) path,
    rows narrower than one lane's four pixels, a 2 x 2 source, and 520 x 200 (fp32: the strip kernel at two pixels per
    lane, its fifth strip 8 columns wide)."""
    import torch

    rng = np.random.default_rng(zlib.crc32(repr((fmt, src, dst)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), src[0], src[1], pattern=p) for p in ("uniform", "gradient", "uniform")]
    imgs = upload(evam, frames, gpu)
    for color in ("BGR", "RGB"):
        info = evam.PreProcInfo(color_space=color, **(NORM if dtype == "f32" else {}))
        check_nhwc(evam, torch, O, coracle, gpu, pp, frames, dst, dtype, info, what=f"{fmt} {src}->{dst} {dtype} {color}",
                   imgs=imgs)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("placement", ["top_left", "center"])
def test_letterbox(evam, O, coracle, gpu, pp, fmt, dtype, placement):
    """aspect-ratio into 300 x 120 (padding columns) and 72 x 72 (padding rows), a distinct fill per channel."""
    import torch

    rng = np.random.default_rng(zlib.crc32(repr((fmt, dtype, placement)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), 200, 120) for _ in range(3)]
    imgs = upload(evam, frames, gpu)
    for color in ("BGR", "RGB"):
        info = evam.PreProcInfo(resize="aspect-ratio", placement=placement, fill=(4, 5, 6), color_space=color,
                                **(NORM if dtype == "f32" else {}))
        for dst in ((300, 120), (72, 72)):
            check_nhwc(evam, torch, O, coracle, gpu, pp, frames, dst, dtype, info,
                       what=f"letterbox {fmt} {dtype} {placement} {color} -> {dst}", imgs=imgs)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_aspect_central_crop(evam, O, coracle, gpu, pp, dtype):
    import torch

    rng = np.random.default_rng(4)
    frames = [O.random_frame(rng, O.BGRX, 768, 432) for _ in range(2)]
    info = evam.PreProcInfo(resize="aspect-ratio", crop="central", **(NORM if dtype == "f32" else {}))
    check_nhwc(evam, torch, O, coracle, gpu, pp, frames, (224, 224), dtype, info, what=f"central crop {dtype}")


@pytest.mark.parametrize("fmt", ["NV12", "BGRX"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_roi_batch(evam, O, coracle, gpu, pp, fmt, dtype):
    """The 104 ROIs of test_gpu_parity.test_roi_batch (edge, odd and partly-outside rects, mixed geometry) -> 72 x 72."""
    import torch

    rng = np.random.default_rng(11)
    W, H = 320, 240
    frames = [O.random_frame(rng, fc(O, fmt), W, H) for _ in range(2)]
    rois = []
    for si in range(2):
        for _ in range(50):
            w = int(rng.integers(3, 200))
            h = int(rng.integers(3, 150))
            x = int(rng.integers(-20, W - 2))
            y = int(rng.integers(-20, H - 2))
            w, h = max(w, 3 - x), max(h, 3 - y)
            rois.append((si, x, y, w, h))
    rois += [(0, 0, 0, W, H), (1, W - 3, H - 3, 10, 10), (0, 1, 1, 1, 1), (1, 5, 7, 9, 11)]
    info = evam.PreProcInfo(color_space="RGB", **({"range": (0.0, 1.0)} if dtype == "f32" else {}))
    check_nhwc(evam, torch, O, coracle, gpu, pp, frames, (72, 72), dtype, info, rois=rois, what=f"roi batch {fmt} {dtype}")


def test_ring_slots(evam, O, coracle, gpu, pp):
    """A [2*16+1, 3, 24, 40] channels-last ring written at slot_offset t, slot_stride 16 for t = 0..2."""
    import torch

    rng = np.random.default_rng(8)
    shape = (2 * 16 + 1, 3, 24, 40)
    out = nhwc_full(torch, shape, "f32", gpu)
    ref = np.full(shape, 7, np.float32)
    info = evam.PreProcInfo(resize="aspect-ratio", crop="central", **NORM)
    for t in range(3):
        frames = [O.random_frame(rng, O.BGRX, 96, 54) for _ in range(2)]
        pp.convert(upload(evam, frames, gpu), out, info, slot_offset=t, slot_stride=16)
        part, _ = run_oracle(O, coracle, frames, shape, "f32", info, slot_offset=t, slot_stride=16)
        for s in (t, 16 + t):
            ref[s] = part[s]
    torch.cuda.synchronize()
    assert out.permute(0, 2, 3, 1).is_contiguous()
    assert_same(out.cpu().numpy(), ref, "channels-last ring")


@pytest.mark.parametrize("dtype,dst", [("u8", (40, 24)), ("f32", (33, 17))])
def test_explicit_slots(evam, O, coracle, gpu, pp, dtype, dst):
    """slots=[...]: a permuted table with gaps; unwritten slots keep 7."""
    import torch

    rng = np.random.default_rng(21)
    frames = [O.random_frame(rng, O.NV12, 120, 64, pattern="gradient" if i % 2 else "uniform") for i in range(5)]
    slots = [9, 0, 17, 4, 12]
    shape = (19, 3, dst[1], dst[0])
    out = nhwc_full(torch, shape, dtype, gpu)
    info = evam.PreProcInfo(color_space="RGB", **(NORM if dtype == "f32" else {}))
    pp.convert(upload(evam, frames, gpu), out, info, slots=slots)
    torch.cuda.synchronize()
    ref, _ = run_oracle(O, coracle, frames, (5, 3, dst[1], dst[0]), dtype, info)
    got = out.cpu().numpy()
    for i, s in enumerate(slots):
        assert_same(got[s], ref[i], f"item {i} -> slot {s}")
    assert (got[np.setdiff1d(np.arange(19), slots)] == 7).all()


def test_odd_base(evam, O, coracle, gpu, pp):
    """convert into big[1:] of a u8 channels-last [4,3,17,33]: the view starts 1,683 bytes in, at an odd address."""
    import torch

    rng = np.random.default_rng(31)
    frames = [O.random_frame(rng, O.NV12, 66, 50) for _ in range(2)]
    big = nhwc_full(torch, (4, 3, 17, 33), "u8", gpu)
    view = big[1:]
    assert view.data_ptr() % 2 == 1 and view.permute(0, 2, 3, 1).is_contiguous()
    pp.convert(upload(evam, frames, gpu), view, None)
    torch.cuda.synchronize()
    ref, _ = run_oracle(O, coracle, frames, (4, 3, 17, 33), "u8", None, slot_offset=1)
    assert_same(big.cpu().numpy(), ref, "odd base")


@pytest.mark.parametrize("n", [2, 32])
def test_hot_c2_channels_last(evam, O, coracle, gpu, n):
    """C2 (1080p NV12 -> 512 x 512 fp32, normalised) into a channels-last tensor, off the generic kernel."""
    import torch

    wl = bench.WORKLOADS["c2"]
    K = 2
    imgs = bench.device_frames(evam, torch, wl, K, gpu, seed=1234)
    info = bench.make_info(evam, wl)
    DW, DH = wl["dst"]
    ref = oracle_items(O, coracle, host_frames(O, imgs), [(k, 0, 0, 0, 0) for k in range(K)], (K, 3, DH, DW), "f32", info)
    ref_dev = torch.from_numpy(ref).to(gpu)
    out = nhwc_full(torch, (n + 2, 3, DH, DW), "f32", gpu)
    h = evam.HipPreProcessor(device=0)
    try:
        h.convert([imgs[i % K] for i in range(n)], out, info, slot_offset=1)
        torch.cuda.synchronize()
        assert h.stats().kernels & evam.native.KERNEL_GENERIC == 0, h.stats().kernels
    finally:
        h.close()
    assert out.permute(0, 2, 3, 1).is_contiguous()
    expect_items(torch, out[1:n + 1], ref_dev, torch.arange(n, device=gpu) % K, ref, f"c2 channels-last x {n}")
    assert all_seven(torch, out[0]) and all_seven(torch, out[n + 1])


@pytest.mark.parametrize("fmt", ["NV12", "I420"])
@pytest.mark.parametrize("shape", ["c1", "letterbox", "letterbox_columns"])
def test_hot_u8_upscale_channels_last(evam, O, coracle, gpu, fmt, shape):
    """32-frame u8 vertical upscales into channels-last tensors (C1: 768 x 432 -> 512 x 512; 200 x 120 letterboxed
    into 512 x 512, padding rows, and into 640 x 256, padding columns), BGR and RGB: the launches the band kernel
    serves in planar form, off the generic kernel."""
    import torch

    src, dst, kw = {"c1": ((768, 432), (512, 512), {}),
                    "letterbox": ((200, 120), (512, 512), {"resize": "aspect-ratio", "placement": "center", "fill": (4, 5, 6)}),
                    "letterbox_columns": ((200, 120), (640, 256), {"resize": "aspect-ratio", "fill": (4, 5, 6)})}[shape]
    K, n = 2, 32
    imgs = bench.device_frames(evam, torch, dict(fourcc=fmt, src=src), K, gpu, seed=7)
    frames = host_frames(O, imgs)
    h = evam.HipPreProcessor(device=0)
    try:
        for color in ("BGR", "RGB"):
            info = evam.PreProcInfo(color_space=color, **kw)
            ref = oracle_items(O, coracle, frames, [(k, 0, 0, 0, 0) for k in range(K)], (K, 3, dst[1], dst[0]), "u8", info)
            ref_dev = torch.from_numpy(ref).to(gpu)
            out = nhwc_full(torch, (n + 2, 3, dst[1], dst[0]), "u8", gpu)
            h.convert([imgs[i % K] for i in range(n)], out, info, slot_offset=1)
            torch.cuda.synchronize()
            assert h.stats().kernels & evam.native.KERNEL_GENERIC == 0, h.stats().kernels
            assert out.permute(0, 2, 3, 1).is_contiguous()
            expect_items(torch, out[1:n + 1], ref_dev, torch.arange(n, device=gpu) % K, ref, f"{shape} {fmt} {color}")
            assert all_seven(torch, out[0]) and all_seven(torch, out[n + 1])
    finally:
        h.close()


@pytest.mark.parametrize("fmt,src", [("NV12", (1920, 1080)), ("I420", (768, 432)), ("BGRX", (768, 432))])
@pytest.mark.parametrize("n", [2, 32])
def test_hot_export_bgr(evam, O, coracle, gpu, fmt, src, n):
    """export_bgr at source size: [n, H, W, 3] u8 equal to the oracle's identity output in HWC order, off the
    generic kernel, into the caller's ``out`` without touching its neighbours."""
    import torch

    wl = dict(fourcc=fmt, src=src)
    K = 2
    imgs = bench.device_frames(evam, torch, wl, K, gpu, seed=99)
    W, H = src
    ref = oracle_items(O, coracle, host_frames(O, imgs), [(k, 0, 0, 0, 0) for k in range(K)], (K, 3, H, W), "u8",
                       evam.PreProcInfo())
    ref_hwc = np.ascontiguousarray(ref.transpose(0, 2, 3, 1))
    ref_dev = torch.from_numpy(ref_hwc).to(gpu)
    big = torch.full((n + 2, H, W, 3), 7, dtype=torch.uint8, device=gpu)
    h = evam.HipPreProcessor(device=0)
    try:
        got = h.export_bgr([imgs[i % K] for i in range(n)], out=big[1:n + 1])
        torch.cuda.synchronize()
        assert h.stats().kernels & evam.native.KERNEL_GENERIC == 0, h.stats().kernels
        assert got.shape == (n, H, W, 3) and got.is_contiguous() and got.data_ptr() == big[1].data_ptr()
        expect_items(torch, got, ref_dev, torch.arange(n, device=gpu) % K, ref_hwc, f"export {fmt} x {n}")
        assert all_seven(torch, big[0]) and all_seven(torch, big[n + 1])
        if n == 2:
            fresh = h.export_bgr(imgs, color_space="RGB")
            torch.cuda.synchronize()
            assert fresh.shape == (2, H, W, 3) and fresh.dtype == torch.uint8
            assert torch.equal(fresh, ref_dev.flip(-1))
    finally:
        h.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVAM_FUZZ_NHWC_CASES", "32"))))
def test_random_configurations(evam, O, coracle, gpu, pp, seed):
    """test_gpu_parity's seeded random calls with the output made channels-last (one more slot at the end)."""
    import torch

    fmt, frames, shape, dtype, info, rois, offset, stride = random_case(evam, O, np.random.default_rng(5000 + seed))
    shape = (shape[0] + 1,) + tuple(shape[1:])
    what = f"seed {seed}: {fmt} {[(f.width, f.height) for f in frames]} -> {shape} {dtype} {info} " \
           f"{'%d rois' % len(rois) if rois else 'frames'} offset {offset} stride {stride}"
    out = nhwc_full(torch, shape, dtype, gpu)
    pp.convert(upload(evam, frames, gpu), out, info, rois=[evam.Roi(*r) for r in rois] if rois else None,
               slot_offset=offset, slot_stride=stride)
    torch.cuda.synchronize()
    assert out.permute(0, 2, 3, 1).is_contiguous()
    ref, _ = run_oracle(O, coracle, frames, shape, dtype, info, rois=rois, slot_offset=offset, slot_stride=stride)
    got = out.cpu().numpy()
    assert (got[-1] == 7).all(), what
    assert_same(got, ref, what)


def test_errors(evam, O, gpu, pp):
    import torch

    N = evam.native
    rng = np.random.default_rng(1)
    imgs = upload(evam, [O.random_frame(rng, O.NV12, 64, 48), O.random_frame(rng, O.NV12, 32, 48)], gpu)
    # an unknown layout value, through the C ABI
    out = torch.zeros((2, 3, 8, 16), dtype=torch.uint8, device=gpu)
    t = N.EvamTensor()
    t.data, t.n, t.c, t.h, t.w, t.slot_offset, t.slot_stride, t.layout = out.data_ptr(), 2, 3, 8, 16, 0, 1, 2
    batch = evam.ImageBatch(imgs)
    cfg = evam.PreProcInfo().to_c(N.DTYPE_U8)
    rc = pp._lib.evam_pp_run(pp._h, batch.c_array, 2, None, 2, ctypes.byref(cfg), ctypes.byref(t), None)
    assert rc == N.ERR_INVALID_ARG and b"layout" in pp._lib.evam_pp_last_error()
    t.layout, t.reserved = N.LAYOUT_NHWC, 12345  # reserved is ignored
    assert pp._lib.evam_pp_run(pp._h, batch.c_array, 2, None, 2, ctypes.byref(cfg), ctypes.byref(t), None) == N.OK
    torch.cuda.synchronize()
    # contiguous in neither format
    with pytest.raises(evam.PreProcError) as e:
        pp.convert(imgs, torch.zeros((2, 3, 8, 32), dtype=torch.uint8, device=gpu)[:, :, :, ::2])
    assert e.value.status == N.ERR_INVALID_ARG
    # export of frames of two sizes
    with pytest.raises(evam.PreProcError) as e:
        pp.export_bgr(imgs)
    assert e.value.status == N.ERR_INVALID_ARG


# ---- pipeline server ---------------------------------------------------------------------------------------------
@pytest.fixture
def server(evam, tmp_path):
    ps = evam.pipeline_server
    mdir = make_model_tree(str(tmp_path / "models"), {
        "det_alias": {"det_ver": (64, 64, {"json_schema_version": "2.0.0", "input_preproc": [],
                                           "output_postproc": [{"labels": ["bg", "car"]}]})}})
    yield ps, mdir
    ps.PipelineServer.stop()


def nv12_source(O, n=3, w=66, h=50, seed=3):
    rng = np.random.default_rng(seed)
    frames = [O.random_frame(rng, O.NV12, w, h) for _ in range(n)]
    return frames, {"type": "frames", "frames": [{"fourcc": f.fourcc, "width": f.width, "height": f.height,
                                                   "planes": f.planes} for f in frames]}


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_pipeline_publisher(evam, O, coracle, gpu, server, runner):
    """Destination mode "publisher": (meta, packed BGR bytes) per frame, in order, then the end marker."""
    import torch

    ps, mdir = server
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir, "runner": runner})
    ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(
        lambda t: torch.full((t.shape[0], 1, 7), -1.0), (64, 64), name="det"))
    frames, src = nv12_source(O)
    qout = queue.Queue()
    p = ps.PipelineServer.pipeline("detect", "hip")
    p.start(source=src, destination={"metadata": {"type": "application", "output": qout, "mode": "publisher"}})
    st = p.wait(60)
    assert st["state"] == "COMPLETED", st
    got = []
    while (x := qout.get(timeout=5)) is not None:
        got.append(x)
    assert qout.empty() and len(got) == 3
    ref, _ = run_oracle(O, coracle, frames, (3, 3, 50, 66), "u8")
    for i, (meta, data) in enumerate(got):
        assert isinstance(data, bytes) and len(data) == 50 * 66 * 3
        assert (meta["height"], meta["width"], meta["channels"]) == (50, 66, 3)
        assert meta["caps"] == "video/x-raw, format=(string)BGR, width=(int)66, height=(int)50"
        assert re.fullmatch(r"[A-Z0-9]{10}", meta["img_handle"])
        assert data == ref[i].transpose(1, 2, 0).tobytes(), f"frame {i}"


def test_pipeline_nhwc_model(evam, O, gpu, server):
    """A layout="nhwc" model receives the stage's channels-last blob, with the planar run's values."""
    import torch

    ps, mdir = server
    seen = {"nchw": [], "nhwc": []}

    def model(kind):
        def fn(t):
            seen[kind].append((t.is_contiguous(), t.is_contiguous(memory_format=torch.channels_last), t.cpu().clone()))
            return torch.full((t.shape[0], 1, 7), -1.0)
        return fn

    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir})
    for kind in ("nchw", "nhwc"):
        ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(model(kind), (64, 64), name="det",
                                                                                layout=kind))
        _, src = nv12_source(O)
        p = ps.PipelineServer.pipeline("detect", "hip")
        p.start(source=src, destination={})
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
    assert seen["nchw"] and all(c and not cl for c, cl, _ in seen["nchw"])
    assert seen["nhwc"] and all(cl and not c for c, cl, _ in seen["nhwc"])
    a = torch.cat([t for _, _, t in seen["nchw"]])
    b = torch.cat([t for _, _, t in seen["nhwc"]])
    assert a.shape == b.shape == (3, 3, 64, 64) and torch.equal(a.view(torch.int32), b.view(torch.int32))
