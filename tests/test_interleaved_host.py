"""Interleaved (NHWC) output on the host side: the ABI's layout field, the layout decision for torch tensors, the
publisher message, and the pipeline server's ``"publisher"`` destination with a stand-in pre-processor (the kernels
are covered by tests/test_gpu_interleaved.py)."""
import ctypes
import os
import queue
import re

import pytest
import torch

from test_pipeline_runner import StubPP, register, stubbed  # noqa: F401  (stubbed: fixture)
from test_pipeline_server import PIPES

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "evam_pp.h")


def test_header_matches_native(evam):
    N = evam.native
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+EVAM_PP_ABI_VERSION\s+(\d+)", text).group(1)) == N.ABI_VERSION == 3
    assert int(re.search(r"EVAM_LAYOUT_NCHW\s*=\s*(\d+)", text).group(1)) == N.LAYOUT_NCHW == 0
    assert int(re.search(r"EVAM_LAYOUT_NHWC\s*=\s*(\d+)", text).group(1)) == N.LAYOUT_NHWC == 1
    body = re.search(r"typedef struct evam_tensor \{(.*?)\} evam_tensor;", text, re.S).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [f[0] for f in N.EvamTensor._fields_]


def test_tensor_struct_layout(evam):
    N = evam.native
    assert ctypes.sizeof(N.EvamTensor) == 40 == N.STRUCT_SIZES[N.EvamTensor]
    assert N.EvamTensor.layout.offset == 32 and N.EvamTensor.reserved.offset == 36
    assert N.EvamTensor().layout == N.LAYOUT_NCHW  # a zero-initialised struct is planar


def test_layout_decision(evam):
    N = evam.native
    planar = torch.zeros((2, 3, 5, 7))
    assert evam.tensor_layout(planar) == N.LAYOUT_NCHW
    cl = torch.zeros((2, 3, 5, 7)).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and evam.tensor_layout(cl) == N.LAYOUT_NHWC
    assert evam.tensor_layout(torch.zeros((2, 5, 7, 3), dtype=torch.uint8).permute(0, 3, 1, 2)) == N.LAYOUT_NHWC
    assert evam.tensor_layout(cl[1:]) == N.LAYOUT_NHWC
    # both formats coincide: planar, as before
    assert evam.tensor_layout(torch.zeros((2, 3, 1, 1)).contiguous(memory_format=torch.channels_last)) == N.LAYOUT_NCHW
    for bad in (planar[:, :, :, ::2], cl[:, :, ::2], planar[:, :, 1:], torch.zeros((2, 4, 5, 7)), torch.zeros((3, 5, 7))):
        with pytest.raises(evam.PreProcError) as e:
            evam.tensor_layout(bad)
        assert e.value.status == N.ERR_INVALID_ARG


def test_publisher_message(evam):
    P = evam.postproc
    fr = P.FrameResult(66, 50, 4, "cam0")
    frame = bytes(50 * 66 * 3)
    meta, got = P.publisher_message(fr, frame)
    assert got is frame
    assert set(meta) == {"height", "width", "channels", "caps", "img_handle", "gva_meta"}
    assert (meta["height"], meta["width"], meta["channels"]) == (50, 66, 3)
    assert meta["caps"] == "video/x-raw, format=(string)BGR, width=(int)66, height=(int)50"
    assert re.fullmatch(r"[A-Z0-9]{10}", meta["img_handle"])
    meta2, _ = P.publisher_message(fr, frame, caps="x", img_handle="ABCDEFGH12")
    assert meta2["caps"] == "x" and meta2["img_handle"] == "ABCDEFGH12"


class ExportStub(StubPP):
    """StubPP plus export_bgr: frame i's image is H x W x 3 bytes of the value its luma plane starts with."""

    exports = []

    def export_bgr(self, srcs, out=None, color_space="BGR"):
        imgs = list(srcs)
        ExportStub.exports.append(len(imgs))
        return torch.stack([torch.full((im.height, im.width, 3), int(im.planes[0][0, 0]), dtype=torch.uint8)
                            for im in imgs])


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_publisher_destination(stubbed, monkeypatch, runner):  # noqa: F811
    ps, pre, mdir = stubbed
    monkeypatch.setattr(pre, "HipPreProcessor", ExportStub)
    ExportStub.exports = []
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir, "runner": runner})
    register(ps)
    W, H, n = 66, 50, 5
    imgs = []
    for i in range(n):
        planes = [torch.full((H, 128), 10 + i, dtype=torch.uint8), torch.zeros((H // 2, 128), dtype=torch.uint8)]
        imgs.append(pre.Image(pre.FOURCC_BY_NAME["NV12"], W, H, planes))
    qout = queue.Queue()
    p = ps.PipelineServer.pipeline("detect", "hip")
    p.start(source={"type": "frames", "frames": imgs},
            destination={"metadata": {"type": "application", "output": qout, "mode": "publisher"}},
            parameters={"detection-properties": {"batch-size": 2}})
    st = p.wait(60)
    assert st["state"] == "COMPLETED", st
    got = []
    while (x := qout.get(timeout=5)) is not None:
        got.append(x)
    assert qout.empty()  # the end marker came last
    assert len(got) == n and sum(ExportStub.exports) == n
    for i, (meta, frame) in enumerate(got):
        assert isinstance(frame, bytes) and len(frame) == H * W * 3
        assert frame == bytes([10 + i]) * (H * W * 3)  # frame order
        assert (meta["height"], meta["width"], meta["channels"]) == (H, W, 3)
        assert meta["caps"] == f"video/x-raw, format=(string)BGR, width=(int){W}, height=(int){H}"
        assert re.fullmatch(r"[A-Z0-9]{10}", meta["img_handle"]) and "gva_meta" in meta
