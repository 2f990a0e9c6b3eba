"""JPEG encoding, host side: the numpy restatement of libjpeg (tests/jpeg_ref.py) pinned byte for byte to the files
libjpeg-turbo wrote (tests/golden/jpeg, through Pillow; tests/golden/jpeg/generate.py), the library's host helpers
against the same files, the refusals that need no device, and the pipeline server's "encoding" option with a stand-in
pre-processor. The kernels are covered by tests/test_gpu_jpeg.py and tests/test_gpu_jpeg_sweep.py."""
import glob
import io
import os
import queue

import numpy as np
import pytest
import torch

import jpeg_ref
from jpeg_content import CUT_FRAMES, content, cut_strides
from test_pipeline_runner import StubPP, register, stubbed  # noqa: F401  (stubbed: fixture)
from test_pipeline_server import PIPES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")


def golden_cases():
    inputs = np.load(os.path.join(GOLDEN, "inputs.npz"))
    out = []
    for name in inputs.files:
        with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
            out.append((name, inputs[name], int(name.rsplit("_q", 1)[1]), f.read()))
    return out


CASES = golden_cases()


def test_golden_set_is_complete():
    assert len(CASES) == len(glob.glob(os.path.join(GOLDEN, "*.jpg"))) >= 21
    sizes = {(im.shape[1], im.shape[0]) for _, im, _, _ in CASES}
    assert {(1, 1), (8, 8), (16, 16), (18, 18), (24, 40), (26, 10), (17, 9), (23, 25), (33, 47), (50, 34),
            (200, 120)} <= sizes
    for axis in (0, 1):
        assert {0, 1, 2, 8, 9, 10} <= {s[axis] % 16 for s in sizes}
    assert {1, 10, 50, 75, 95, 100} <= {q for _, _, q, _ in CASES}


@pytest.mark.parametrize("name,img,q,ref", CASES, ids=[c[0] for c in CASES])
def test_ref_equals_golden(name, img, q, ref):
    got, stats = jpeg_ref.encode(img, q)
    assert got == ref
    assert set(stats) == {"zrl", "stuffed", "max_category", "dummy_blocks", "min_block_bits", "max_dc_category",
                          "max_zrl_run", "no_eob_blocks"}


def test_ref_stats_see_the_hard_parts():
    """The properties tests/test_gpu_jpeg.py asserts before it trusts a case, on the same contents."""
    by = {name: jpeg_ref.encode(img, q)[1] for name, img, q, _ in CASES}
    assert by["const_48x32_q95"]["min_block_bits"] <= 6
    assert by["checker_48x32_q10"]["zrl"] > 0
    assert by["sat_50x34_q100"]["max_category"] >= 10 and by["sat_50x34_q100"]["stuffed"] > 0
    assert by["noise_18x18_q10"]["dummy_blocks"] == 7 and by["grad_16x16_q95"]["dummy_blocks"] == 0


def test_ref_stats_of_the_sweep_contents():
    """What tests/test_gpu_jpeg_sweep.py asserts before it trusts a case, on the reference alone: DC category 11,
    three ZRL codes in front of one coefficient, blocks that end without an EOB, quality 0 as quality 1, the file
    that outgrows encode_jpeg's default slot, and cuts that fall behind a stuffed 0xFF. The counts are additions to
    ``encode``'s stats, so the golden files must still reproduce."""
    for name, img, q, ref in CASES:
        assert jpeg_ref.encode(img, q)[0] == ref, name
    _, st = jpeg_ref.encode(content("blocks", 48, 32), 100)
    assert st["max_dc_category"] == 11 == st["max_category"]
    _, st = jpeg_ref.encode(content("lowchecker", 48, 32), 10)
    # coefficient 63 is the only AC coefficient of those 24 blocks: 62 zeros = 3 ZRL + a run of 14, and no EOB
    assert st["max_zrl_run"] == 3 and st["no_eob_blocks"] == 24 and st["zrl"] == 72 and st["max_category"] == 1
    f1, st = jpeg_ref.encode(content("checker", 48, 32), 1)
    assert st["max_zrl_run"] == 2
    assert jpeg_ref.encode(content("checker", 48, 32), 0)[0] == f1
    f, st = jpeg_ref.encode(content("sat", 50, 34, 3), 100)
    assert st["no_eob_blocks"] == 51 and st["dummy_blocks"] == 13 and st["max_dc_category"] == 10
    assert len(f) == 5573 > 1024 + 64 * 48
    assert len(jpeg_ref.encode(content("const", 50, 34), 100)[0]) <= 1024 + 64 * 48
    # a plain scan: no ZRL, every block ends with an EOB
    _, st = jpeg_ref.encode(content("const", 48, 32), 95)
    assert (st["max_zrl_run"], st["no_eob_blocks"], st["zrl"]) == (0, 0, 0)
    stuffed_cuts = 0
    for kind, w, h, seed, q in CUT_FRAMES:
        f, _ = jpeg_ref.encode(content(kind, w, h, seed), q)
        assert f[-2:] == b"\xFF\xD9" and len(f) > 625 + 3
        stuffed_cuts += sum(f[s - 1] == 0xFF and f[s] == 0x00 for s in cut_strides(len(f)) if s < len(f) - 1)
    assert stuffed_cuts >= 2


def test_ref_equals_fresh_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2024)
    for _ in range(40):
        w, h, q = int(rng.integers(1, 65)), int(rng.integers(1, 65)), int(rng.integers(1, 101))
        kind = int(rng.integers(0, 3))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if kind == 1:
            img = (img >> 7) * np.uint8(255)
        elif kind == 2:
            img = (img // 32 + np.arange(w, dtype=np.uint8)[None, :, None] * 3).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, "JPEG", quality=q, subsampling=2)
        assert jpeg_ref.encode(img, q)[0] == buf.getvalue(), (w, h, q, kind)


@pytest.mark.parametrize("sampling", ["420", "422", "444", "grey"])
def test_ref_samplings_and_restarts_equal_fresh_pillow(sampling):
    """Every file the decoder accepts that ``encode`` writes: each sampling x restart interval in {0, 1, 5, MCUs per
    row} x three contents x qualities 10, 75, 100 x two odd sizes, the whole file equal to Pillow's (DRI included)."""
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for w, h in ((37, 23), (50, 33)):
        per_row = jpeg_ref.mcu_grid(w, h, sampling)[1]
        for restart in (0, 1, 5, per_row):
            for kind in ("noise", "sat", "grad"):
                for q in (10, 75, 100):
                    img = content(kind, w, h, seed=n)
                    buf = io.BytesIO()
                    if sampling == "grey":
                        im, args = Image.fromarray(np.ascontiguousarray(img[..., 1])), {}
                    else:
                        im = Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
                        args = {"subsampling": {"444": 0, "422": 1, "420": 2}[sampling]}
                    im.save(buf, "JPEG", quality=q, restart_marker_blocks=restart, **args)
                    got, _ = jpeg_ref.encode(img, q, sampling=sampling, restart=restart)
                    assert got == buf.getvalue(), (w, h, restart, kind, q)
                    assert (b"\xFF\xDD\x00\x04" in got[:700]) == (restart > 0)
                    n += 1
    assert n == 72
    assert jpeg_ref.encode(img, 75)[0] == jpeg_ref.encode(img, 75, sampling="420", restart=0)[0]


@pytest.mark.parametrize("name,img,q,ref", CASES, ids=[c[0] for c in CASES])
def test_header_and_bound(evam, name, img, q, ref):
    h, w = img.shape[:2]
    assert evam.native.JPEG_HEADER_LEN == jpeg_ref.HEADER_LEN == 623
    assert evam.jpeg_header(w, h, q) == ref[:623]
    n_blocks = 6 * (-(-w // 16)) * (-(-h // 16))
    analytic = 623 + 2 + 2 * (n_blocks * (11 + 11 + 63 * (16 + 10)) // 8)
    assert evam.jpeg_bound(w, h) >= analytic >= len(ref)


def test_header_quality_zero_and_refusals(evam):
    N = evam.native
    assert evam.jpeg_header(32, 16, 0) == evam.jpeg_header(32, 16, 1) == jpeg_ref.header(32, 16, 1)
    for args in ((32, 16, 101), (32, 16, -1), (0, 16, 50), (32, 40000, 50)):
        with pytest.raises(evam.PreProcError) as e:
            evam.jpeg_header(*args)
        assert e.value.status == N.ERR_INVALID_ARG
    with pytest.raises(evam.PreProcError):
        evam.jpeg_bound(0, 5)
    lib = N.load_library()
    assert lib.evam_pp_jpeg_bound(-1, 5) == 0
    import ctypes

    n = ctypes.c_size_t()
    small = (ctypes.c_uint8 * 100)()
    assert lib.evam_pp_jpeg_header(32, 16, 50, small, 100, ctypes.byref(n)) == N.ERR_INVALID_ARG and n.value == 623
    assert {"evam_pp_jpeg_header", "evam_pp_encode_jpeg"} <= set(N.EXPORTED_SYMBOLS)
    assert N.EXPORTED_SYMBOLS_SIZE_T == ("evam_pp_jpeg_bound",)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "evam_pp.h")).read()
    for name in ("evam_pp_jpeg_header", "evam_pp_jpeg_bound", "evam_pp_encode_jpeg"):
        assert hasattr(lib, name) and f" {name}(" in header
    assert N.KERNEL_JPEG == 128 and "EVAM_KERNEL_JPEG = 128" in open(
        os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "evam_pp.h")).read()


def host_image(pre, w, h):
    planes = [torch.zeros((h, 128), dtype=torch.uint8), torch.zeros((h // 2, 128), dtype=torch.uint8)]
    return pre.Image(pre.FOURCC_BY_NAME["NV12"], w, h, planes)


def test_encode_refusals_need_no_device(evam):
    """Empty list, mixed sizes, quality 101 and -1 are refused before anything touches a device: the object here was
    never bound to one."""
    pre, N = evam.preproc, evam.native
    pp = object.__new__(pre.HipPreProcessor)
    a, b = host_image(pre, 64, 32), host_image(pre, 32, 32)
    for srcs, q in (([], 95), ([a, b], 95), ([a], 101), ([a], -1), ([a], 95.0), ([a], True)):
        for call in (lambda: pp.encode_jpeg(srcs, q), lambda: pp.encode_jpeg_into(srcs, None, None, q)):
            with pytest.raises(evam.PreProcError) as e:
                call()
            assert e.value.status == N.ERR_INVALID_ARG


def test_encoding_option_parsing(evam):
    ps, N = evam.pipeline_server, evam.native
    pub = {"type": "application", "output": queue.Queue(), "mode": "publisher"}
    assert ps.publisher_encoding(None) is None and ps.publisher_encoding({}) is None
    assert ps.publisher_encoding({"metadata": pub}) is None
    for level in (0, 95, 100):
        assert ps.publisher_encoding({"metadata": {**pub, "encoding": {"type": "jpeg", "level": level}}}) == ("jpeg", level)
    assert ps.publisher_encoding({**pub, "encoding": {"type": "jpeg", "level": 7}}) == ("jpeg", 7)
    bad = [({"type": "png", "level": 3}, N.ERR_UNSUPPORTED), ({"type": "webp", "level": 3}, N.ERR_UNSUPPORTED),
           ({"type": "JPEG", "level": 3}, N.ERR_UNSUPPORTED), ({"type": "jpeg", "level": 101}, N.ERR_INVALID_ARG),
           ({"type": "jpeg", "level": -1}, N.ERR_INVALID_ARG), ({"type": "jpeg", "level": "95"}, N.ERR_INVALID_ARG),
           ({"type": "jpeg"}, N.ERR_INVALID_ARG), ("jpeg", N.ERR_INVALID_ARG)]
    for enc, status in bad:
        with pytest.raises(evam.PreProcError) as e:
            ps.publisher_encoding({"metadata": {**pub, "encoding": enc}})
        assert e.value.status == status, enc
    with pytest.raises(evam.PreProcError) as e:  # encoded frames exist in publisher mode only
        ps.publisher_encoding({"metadata": {"type": "application", "output": queue.Queue(), "mode": "frames",
                                            "encoding": {"type": "jpeg", "level": 95}}})
    assert e.value.status == N.ERR_INVALID_ARG


def test_publisher_message_encoding(evam):
    P = evam.postproc
    fr = P.FrameResult(66, 50, 4, "cam0")
    plain, _ = P.publisher_message(fr, b"x", caps="c", img_handle="H")
    assert list(plain) == ["height", "width", "channels", "caps", "img_handle", "gva_meta"]
    assert P.publisher_meta(fr, "c", "H") == plain == P.publisher_meta(fr, "c", "H", None)
    meta, frame = P.publisher_message(fr, b"file", caps="c", img_handle="H", encoding=("jpeg", 95))
    assert frame == b"file"
    assert list(meta) == list(plain) + ["encoding_type", "encoding_level"]
    assert (meta["encoding_type"], meta["encoding_level"]) == ("jpeg", 95)
    assert {k: meta[k] for k in plain} == plain


class EncodeStub(StubPP):
    """StubPP plus the two export calls: frame i's "file" names its luma value and the quality."""

    calls = []

    def export_bgr(self, srcs, out=None, color_space="BGR"):
        imgs = list(srcs)
        EncodeStub.calls.append(("raw", len(imgs)))
        return torch.stack([torch.full((im.height, im.width, 3), int(im.planes[0][0, 0]), dtype=torch.uint8)
                            for im in imgs])

    def encode_jpeg(self, srcs, quality=95):
        imgs = list(srcs)
        EncodeStub.calls.append(("jpeg", len(imgs)))
        return [b"JPEG %d q%d" % (int(im.planes[0][0, 0]), quality) for im in imgs]


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_publisher_destination_encoding(stubbed, monkeypatch, runner):  # noqa: F811
    ps, pre, mdir = stubbed
    monkeypatch.setattr(pre, "HipPreProcessor", EncodeStub)
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir, "runner": runner})
    register(ps)
    W, H, n = 66, 50, 5
    imgs = []
    for i in range(n):
        planes = [torch.full((H, 128), 10 + i, dtype=torch.uint8), torch.zeros((H // 2, 128), dtype=torch.uint8)]
        imgs.append(pre.Image(pre.FOURCC_BY_NAME["NV12"], W, H, planes))

    def run(dst_extra):
        EncodeStub.calls = []
        qout = queue.Queue()
        p = ps.PipelineServer.pipeline("detect", "hip")
        p.start(source={"type": "frames", "frames": imgs},
                destination={"metadata": {"type": "application", "output": qout, "mode": "publisher", **dst_extra}},
                parameters={"detection-properties": {"batch-size": 2}})
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
        got = []
        while (x := qout.get(timeout=5)) is not None:
            got.append(x)
        assert qout.empty() and len(got) == n
        return got

    got = run({"encoding": {"type": "jpeg", "level": 80}})
    assert {k for k, _ in EncodeStub.calls} == {"jpeg"} and sum(c for _, c in EncodeStub.calls) == n
    for i, (meta, frame) in enumerate(got):
        assert frame == b"JPEG %d q80" % (10 + i)
        assert (meta["encoding_type"], meta["encoding_level"]) == ("jpeg", 80)
        assert (meta["height"], meta["width"], meta["channels"]) == (H, W, 3)
    got = run({})
    assert {k for k, _ in EncodeStub.calls} == {"raw"}
    for i, (meta, frame) in enumerate(got):
        assert frame == bytes([10 + i]) * (H * W * 3)
        assert "encoding_type" not in meta and "encoding_level" not in meta

    # refused when the pipeline starts, before any frame runs
    for enc, status in (({"type": "png", "level": 3}, -2), ({"type": "jpeg", "level": 101}, -1)):
        EncodeStub.calls = []
        p = ps.PipelineServer.pipeline("detect", "hip")
        with pytest.raises(pre.PreProcError) as e:
            p.start(source={"type": "frames", "frames": imgs},
                    destination={"metadata": {"type": "application", "output": queue.Queue(), "mode": "publisher",
                                              "encoding": enc}})
        assert e.value.status == status and EncodeStub.calls == []
