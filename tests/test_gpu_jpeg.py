"""GPU JPEG encoding of the published frame against tests/jpeg_ref.py, byte for byte.

Every expected file is ``jpeg_ref.encode(identity BGR of the frame, quality)``: the oracle's BGR image of the frame at
source size (``oracle.np_to_bgr``, what ``export_bgr`` publishes), through the numpy restatement of libjpeg that
tests/test_jpeg_host.py pins to libjpeg-turbo files. Contents chosen for the bit packer are asserted on the reference's
own ``stats``, so a case cannot pass without meeting the hard part."""
import ctypes
import queue
import re

import numpy as np
import pytest

import jpeg_ref
from jpeg_content import content
from test_gpu_parity import fc, upload
from test_pipeline_server import PIPES, make_model_tree

pytestmark = pytest.mark.gpu

HEADER = 623


@pytest.fixture(scope="module")
def pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


def bgr_frame(O, img, fmt="BGR", seed=0):
    """A BGR / BGRX HostFrame holding ``img`` [H, W, 3], rows padded to a 64-byte pitch with random bytes."""
    h, w = img.shape[:2]
    n = 4 if fmt == "BGRX" else 3
    pitch = -(-(w * n) // 64) * 64
    plane = np.random.default_rng(seed).integers(0, 256, (h, pitch), dtype=np.uint8)
    px = plane[:, :w * n].reshape(h, w, n)
    px[..., :3] = img
    return O.HostFrame(fc(O, fmt), w, h, [plane])


def expected(O, frame, quality):
    return jpeg_ref.encode(O.np_to_bgr(frame, 0, 0, frame.width, frame.height), quality)


def check(evam, O, gpu, pp, frames, quality, what, imgs=None):
    """``imgs``: the device images of ``frames`` where the caller placed them itself (default: one upload per plane)."""
    files = pp.encode_jpeg(imgs or upload(evam, frames, gpu), quality)
    assert pp.stats().kernels & evam.native.KERNEL_JPEG
    assert len(files) == len(frames)
    for i, (f, got) in enumerate(zip(frames, files)):
        ref, _ = expected(O, f, quality)
        assert len(got) == len(ref), f"{what} frame {i}: {len(got)} bytes, reference {len(ref)}"
        if got != ref:
            k = next(j for j in range(len(ref)) if got[j] != ref[j])
            raise AssertionError(f"{what} frame {i}: first difference at byte {k} of {len(ref)}")


@pytest.mark.parametrize("fmt", ["NV12", "I420"])
@pytest.mark.parametrize("size", [(16, 16), (18, 18), (24, 40), (26, 10), (50, 34), (200, 120), (640, 360)])
def test_yuv_sizes(evam, O, gpu, pp, fmt, size):
    """Noise at 95 and a gradient at 75. 640 x 360 is 22.5 MCU rows (a bottom row of dummy Y blocks) and 44 pack
    groups; 18, 26, 50 and 200 leave dummy or partly padded blocks on the right."""
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    check(evam, O, gpu, pp, [O.random_frame(rng, fc(O, fmt), w, h, pitch_align=64)], 95, f"{fmt} {w}x{h} noise")
    check(evam, O, gpu, pp, [O.random_frame(rng, fc(O, fmt), w, h, pitch_align=64, pattern="gradient")], 75,
          f"{fmt} {w}x{h} gradient")


@pytest.mark.parametrize("fmt", ["BGRX", "BGR"])
@pytest.mark.parametrize("size", [(1, 1), (17, 9), (23, 25), (33, 47)])
def test_bgr_sizes(evam, O, gpu, pp, fmt, size):
    w, h = size
    check(evam, O, gpu, pp, [bgr_frame(O, content("noise", w, h, w), fmt)], 95, f"{fmt} {w}x{h} noise")
    check(evam, O, gpu, pp, [bgr_frame(O, content("grad", w, h), fmt)], 75, f"{fmt} {w}x{h} gradient")


def test_c1_source_size(evam, O, gpu, pp):
    rng = np.random.default_rng(5)
    check(evam, O, gpu, pp, [O.random_frame(rng, O.NV12, 768, 432, pitch_align=64, pattern="gradient")], 95, "768x432")


def test_dense_blocks(evam, O, gpu, pp):
    """A constant frame: blocks of a few bits each, about five to an output word."""
    f = bgr_frame(O, content("const", 48, 32))
    _, st = expected(O, f, 95)
    assert st["min_block_bits"] <= 6
    check(evam, O, gpu, pp, [f], 95, "constant")


def test_zero_runs(evam, O, gpu, pp):
    """A per-pixel checkerboard at quality 10: runs of 16 zeros (ZRL codes)."""
    f = bgr_frame(O, content("checker", 48, 32))
    _, st = expected(O, f, 10)
    assert st["zrl"] > 0
    check(evam, O, gpu, pp, [f], 10, "checkerboard")


def test_saturated_noise(evam, O, gpu, pp):
    """Channels of 0 or 255 at quality 100: the largest coefficient categories, stuffed 0xFF bytes, and a file larger
    than encode_jpeg's default slot, so its second pass with the worst-case bound runs."""
    f = bgr_frame(O, content("sat", 50, 34, 3))
    ref, st = expected(O, f, 100)
    assert st["max_category"] >= 10 and st["stuffed"] > 0
    assert len(ref) > 1024 + 64 * 48
    check(evam, O, gpu, pp, [f], 100, "saturated noise")


def test_slot_grows_after_overflow(evam, O, gpu):
    """The call after one that needed the second pass starts with slots large enough, and is as exact."""
    f = bgr_frame(O, content("sat", 50, 34, 3))
    ref = expected(O, f, 100)[0]
    imgs = upload(evam, [f, f], gpu)
    with evam.HipPreProcessor(device=0) as h:
        assert h.encode_jpeg(imgs, 100) == [ref, ref]
        assert len(ref) <= h._jpeg_need[(50, 34)] <= evam.jpeg_bound(50, 34)
        assert h.encode_jpeg(imgs, 100) == [ref, ref]
        assert h.encode_jpeg(imgs[:1], 10) == [expected(O, f, 10)[0]]


def test_batch_and_reuse(evam, O, gpu, pp):
    """Five different frames in one call, the same call again (scratch and tables reused), then another size and
    quality on the same handle."""
    rng = np.random.default_rng(11)
    frames = [O.random_frame(rng, O.NV12, 200, 120, pitch_align=64, pattern=p)
              for p in ("uniform", "gradient", "uniform", "gradient", "uniform")]
    refs = [expected(O, f, 95)[0] for f in frames]
    assert len(set(refs)) == 5
    imgs = upload(evam, frames, gpu)
    for _ in range(2):
        assert pp.encode_jpeg(imgs, 95) == refs
    small = [O.random_frame(rng, O.I420, 50, 34, pitch_align=64) for _ in range(2)]
    assert pp.encode_jpeg(upload(evam, small, gpu), 50) == [expected(O, f, 50)[0] for f in small]
    assert pp.encode_jpeg(imgs, 95) == refs


def test_overflow_keeps_to_its_slot(evam, O, gpu, pp):
    """dst_stride = header + 64 on noise: sizes[i] is still the true length, the bytes after every slot are
    untouched, and the next call with room is exact."""
    import torch

    rng = np.random.default_rng(13)
    frames = [O.random_frame(rng, O.NV12, 200, 120, pitch_align=64) for _ in range(3)]
    refs = [expected(O, f, 95)[0] for f in frames]
    imgs = upload(evam, frames, gpu)
    stride, guard = HEADER + 64, 256
    N = evam.native
    # one frame per call into rows of stride + guard bytes: every slot has its own guard behind it
    rows = torch.full((3, stride + guard), 7, dtype=torch.uint8, device=gpu)
    sizes = torch.zeros(3, dtype=torch.int32, device=gpu)
    pp._bind_stream()
    for i in range(3):
        arr = (N.EvamImage * 1).from_buffer_copy(imgs[i].c_bytes())
        rc = pp._lib.evam_pp_encode_jpeg(pp._h, arr, 1, 95, ctypes.c_void_p(rows[i].data_ptr()), stride,
                                         ctypes.c_void_p(sizes[i:].data_ptr()))
        assert rc == 0
    torch.cuda.synchronize()
    assert sizes.cpu().tolist() == [len(r) for r in refs]
    got = rows.cpu().numpy()
    for i in range(3):
        assert (got[i, stride:] == 7).all(), f"slot {i}: bytes behind the slot were written"
        assert got[i, :HEADER].tobytes() == refs[i][:HEADER]
    # the three in one call, slots back to back, a guard behind the last
    packed = torch.full((3 * stride + guard,), 7, dtype=torch.uint8, device=gpu)
    sizes.zero_()
    pp.encode_jpeg_into(imgs, packed[:3 * stride].view(3, stride), sizes, 95)
    torch.cuda.synchronize()
    assert sizes.cpu().tolist() == [len(r) for r in refs]
    assert bool((packed[3 * stride:] == 7).all())
    assert packed[:3 * stride].view(3, stride)[:, :HEADER].cpu().numpy().tobytes() == b"".join(r[:HEADER] for r in refs)
    big = torch.full((3, max(len(r) for r in refs) + guard), 7, dtype=torch.uint8, device=gpu)
    pp.encode_jpeg_into(imgs, big, sizes, 95)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    for i in range(3):
        assert got[i, :len(refs[i])].tobytes() == refs[i]
        assert (got[i, len(refs[i]):] == 7).all()


def test_in_flight(evam, O, gpu):
    """Three handles on three streams, 12 calls round-robin, no synchronisation until the end."""
    import torch

    rng = np.random.default_rng(17)
    frames = [O.random_frame(rng, O.NV12, 200, 120, pitch_align=64, pattern="gradient" if i & 1 else "uniform")
              for i in range(12)]
    refs = [expected(O, f, 90)[0] for f in frames]
    imgs = upload(evam, frames, gpu)
    cap = max(len(r) for r in refs) + 64
    streams = [torch.cuda.Stream(device=gpu) for _ in range(3)]
    handles = [evam.HipPreProcessor(device=0, stream=s) for s in streams]
    outs = [torch.zeros((1, cap), dtype=torch.uint8, device=gpu) for _ in range(12)]
    sizes = [torch.zeros(1, dtype=torch.int32, device=gpu) for _ in range(12)]
    torch.cuda.synchronize()  # uploads and fills ran on the default stream
    try:
        for i in range(12):
            handles[i % 3].encode_jpeg_into([imgs[i]], outs[i], sizes[i], 90)
        torch.cuda.synchronize()
        for i in range(12):
            n = int(sizes[i].item())
            assert n == len(refs[i]) and outs[i][0, :n].cpu().numpy().tobytes() == refs[i], f"call {i}"
    finally:
        for h in handles:
            h.close()


def test_refusals(evam, O, gpu, pp):
    import torch

    N = evam.native
    rng = np.random.default_rng(19)
    imgs = upload(evam, [O.random_frame(rng, O.NV12, 32, 32, pitch_align=64)], gpu)
    sizes = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(evam.PreProcError) as e:  # smaller than the header plus EOI
        pp.encode_jpeg_into(imgs, torch.zeros((1, HEADER + 1), dtype=torch.uint8, device=gpu), sizes, 95)
    assert e.value.status == N.ERR_INVALID_ARG
    arr = (N.EvamImage * 1).from_buffer_copy(imgs[0].c_bytes())
    out = torch.zeros((1, 4096), dtype=torch.uint8, device=gpu)
    for q in (-1, 101):
        assert pp._lib.evam_pp_encode_jpeg(pp._h, arr, 1, q, ctypes.c_void_p(out.data_ptr()), 4096,
                                           ctypes.c_void_p(sizes.data_ptr())) == N.ERR_INVALID_ARG
    assert pp._lib.evam_pp_encode_jpeg(pp._h, arr, 0, 95, ctypes.c_void_p(out.data_ptr()), 4096,
                                       ctypes.c_void_p(sizes.data_ptr())) == N.ERR_INVALID_ARG
    assert pp._lib.evam_pp_encode_jpeg(pp._h, arr, 1, 95, None, 4096,
                                       ctypes.c_void_p(sizes.data_ptr())) == N.ERR_INVALID_ARG
    arr[0].pitch[0] = 40  # evam_pp_run's source validation, with its code
    assert pp._lib.evam_pp_encode_jpeg(pp._h, arr, 1, 95, ctypes.c_void_p(out.data_ptr()), 4096,
                                       ctypes.c_void_p(sizes.data_ptr())) == N.ERR_ALIGNMENT


# ---- pipeline server ---------------------------------------------------------------------------------------------
@pytest.fixture
def server(evam, tmp_path):
    ps = evam.pipeline_server
    mdir = make_model_tree(str(tmp_path / "models"), {
        "det_alias": {"det_ver": (64, 64, {"json_schema_version": "2.0.0", "input_preproc": [],
                                           "output_postproc": [{"labels": ["bg", "car"]}]})}})
    yield ps, mdir
    ps.PipelineServer.stop()


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_pipeline_publisher_jpeg(evam, O, gpu, server, runner):
    """Publisher mode with {"type": "jpeg", "level": 95}: every published frame is the reference file and the meta
    carries the two keys; without "encoding" the same pipeline publishes raw bytes."""
    import torch

    ps, mdir = server
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir, "runner": runner})
    ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(
        lambda t: torch.full((t.shape[0], 1, 7), -1.0), (64, 64), name="det"))
    rng = np.random.default_rng(23)
    frames = [O.random_frame(rng, O.NV12, 66, 50, pattern="gradient" if i & 1 else "uniform") for i in range(4)]
    src = {"type": "frames", "frames": [{"fourcc": f.fourcc, "width": f.width, "height": f.height,
                                          "planes": f.planes} for f in frames]}
    for enc in ({"type": "jpeg", "level": 95}, None):
        qout = queue.Queue()
        dst = {"type": "application", "output": qout, "mode": "publisher"}
        if enc:
            dst["encoding"] = enc
        p = ps.PipelineServer.pipeline("detect", "hip")
        p.start(source=src, destination={"metadata": dst})
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
        got = []
        while (x := qout.get(timeout=5)) is not None:
            got.append(x)
        assert qout.empty() and len(got) == 4
        for i, (meta, data) in enumerate(got):
            assert isinstance(data, bytes)
            assert (meta["height"], meta["width"], meta["channels"]) == (50, 66, 3)
            assert re.fullmatch(r"[A-Z0-9]{10}", meta["img_handle"])
            bgr = O.np_to_bgr(frames[i], 0, 0, 66, 50)
            if enc:
                assert (meta["encoding_type"], meta["encoding_level"]) == ("jpeg", 95)
                assert data == jpeg_ref.encode(bgr, 95)[0], f"frame {i}"
            else:
                assert "encoding_type" not in meta and "encoding_level" not in meta
                assert data == bgr.tobytes(), f"frame {i}"
