"""GPU parity of 16-bit (fp16 / bf16) output tensors, bit-exact: every expected value is the oracle's fp32 output
narrowed once with ``torch.from_numpy(ref).to(torch.float16 | torch.bfloat16)`` and compared as int16, with no
mismatching element allowed.

Pixel parity uses only the two normalisations whose 16-bit table keeps 256 distinct values per channel in both types
(tests/test_half_host.py checks that): the ImageNet one (NORM) and none (0..255), so a wrong u8 value cannot hide
behind the rounding. Every output has a guard slot of 7 at each end and the call starts at slot_offset 1."""
import ctypes
import dataclasses
import zlib

import numpy as np
import pytest

from test_gpu_parity import FORMATS, fc, random_case, run_oracle, upload
from test_pipeline_server import PIPES, make_model_tree

pytestmark = pytest.mark.gpu

NORM = {"range": (0.0, 1.0), "mean": (0.406, 0.456, 0.485), "std": (0.225, 0.224, 0.229)}
NONE = {"range": None, "mean": None, "std": None}
PREC = {"f16": "FP16", "bf16": "BF16"}
HALVES = ["f16", "bf16"]


def tdt(torch, h):
    return {"f16": torch.float16, "bf16": torch.bfloat16}[h]


def half_full(torch, shape, h, device, nhwc=False, value=7):
    out = torch.empty(shape, dtype=tdt(torch, h), device=device,
                      memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    out.fill_(value)
    return out


def narrow_bits(torch, ref32, h):
    """The oracle's fp32 array narrowed by torch, as an int16 CPU tensor."""
    return torch.from_numpy(np.ascontiguousarray(ref32)).to(tdt(torch, h)).view(torch.int16)


def same_bits(torch, got, want_bits, what):
    """got (a 16-bit tensor of any device / layout) equals want_bits (int16, logical NCHW order) bit for bit."""
    g = got.detach().cpu().contiguous().view(torch.int16)
    if torch.equal(g, want_bits):
        return
    bad = (g != want_bits).nonzero()
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f"{what}: {len(bad)} mismatches of {g.numel()}; first at {i}: got "
                         f"{int(g[i]) & 0xFFFF:#06x} ref {int(want_bits[i]) & 0xFFFF:#06x}")


def check(evam, torch, O, coracle, gpu, pp, frames, dst, h, info, rois=None, nhwc=False, imgs=None, what=""):
    """One call at slot_offset 1 into n + 2 slots of 7: the whole tensor, guards included, against the narrowed oracle."""
    n = len(rois) if rois else len(frames)
    shape = (n + 2, 3, dst[1], dst[0])
    out = half_full(torch, shape, h, gpu, nhwc)
    pp.convert(imgs or upload(evam, frames, gpu), out, info, rois=[evam.Roi(*r) for r in rois] if rois else None,
               slot_offset=1)
    torch.cuda.synchronize()
    k = pp.stats().kernels
    ref, _ = run_oracle(O, coracle, frames, shape, "f32", info, rois=rois, slot_offset=1)
    assert (ref[0] == 7).all() and (ref[-1] == 7).all()
    same_bits(torch, out, narrow_bits(torch, ref, h), f"{what} {h} {'nhwc' if nhwc else 'nchw'}")
    return k


@pytest.fixture(scope="module")
def pp(evam, gpu):
    p = evam.HipPreProcessor(device=0)
    yield p
    p.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("src,dst", [((64, 48), (512, 512)), ((66, 50), (33, 17)), ((96, 64), (96, 64)),
                                     ((64, 48), (1, 37)), ((64, 48), (1, 1)), ((2, 2), (40, 3)),
                                     ((200, 120), (300, 70)), ((640, 360), (520, 200))])
@pytest.mark.parametrize("h", HALVES)
def test_full_frame(evam, O, coracle, gpu, pp, fmt, src, dst, h):
    """3 full frames, BGR (normalised) and RGB (0..255), planar and channels-last: the wave kernel (512 x 512 upscale),
    66-byte rows (33 x 17: every second row starts at an address = 2 mod 4), the identity, rows narrower than a lane's
    pixels, a 2 x 2 source, and 520 x 200 (a last tile 8 columns wide; one output row in five shares a source row with
    the next, so the planner hands this 1.8x downscale to the wave kernel as it does for fp32: the strip kernel at two
    pixels per lane is test_strip_kernel_counts' 640-wide shape)."""
    import torch

    N = evam.native
    rng = np.random.default_rng(zlib.crc32(repr((fmt, src, dst)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), src[0], src[1], pattern=p) for p in ("uniform", "gradient", "uniform")]
    imgs = upload(evam, frames, gpu)
    for color, norm in (("BGR", NORM), ("RGB", {})):
        info = evam.PreProcInfo(color_space=color, precision=PREC[h], **norm)
        for nhwc in (False, True):
            k = check(evam, torch, O, coracle, gpu, pp, frames, dst, h, info, nhwc=nhwc, imgs=imgs,
                      what=f"{fmt} {src}->{dst} {color}")
            if nhwc and dst != (1, 1):  # (at H = W = 1 both layouts coincide and the tensor counts as planar)
                assert k == N.KERNEL_GENERIC, k  # interleaved 16-bit output is the generic kernel's
            elif (src, dst) == ((64, 48), (512, 512)):
                assert k == N.KERNEL_WAVE, k


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("h", HALVES)
@pytest.mark.parametrize("placement", ["top_left", "center"])
def test_letterbox(evam, O, coracle, gpu, pp, fmt, h, placement):
    """aspect-ratio into 300 x 120 (padding columns) and 72 x 72 (padding rows), a distinct fill per channel that goes
    through the table."""
    import torch

    rng = np.random.default_rng(zlib.crc32(repr((fmt, placement)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), 200, 120) for _ in range(3)]
    imgs = upload(evam, frames, gpu)
    for color, norm in (("BGR", {}), ("RGB", NORM)):
        info = evam.PreProcInfo(resize="aspect-ratio", placement=placement, fill=(4, 5, 6), color_space=color,
                                precision=PREC[h], **norm)
        for dst in ((300, 120), (72, 72)):
            for nhwc in (False, True):
                check(evam, torch, O, coracle, gpu, pp, frames, dst, h, info, nhwc=nhwc, imgs=imgs,
                      what=f"letterbox {fmt} {placement} {color} -> {dst}")


@pytest.mark.parametrize("fmt", ["BGRX", "NV12"])
@pytest.mark.parametrize("h", HALVES)
def test_aspect_central_crop(evam, O, coracle, gpu, pp, fmt, h):
    import torch

    rng = np.random.default_rng(4)
    frames = [O.random_frame(rng, fc(O, fmt), 768, 432) for _ in range(2)]
    info = evam.PreProcInfo(resize="aspect-ratio", crop="central", precision=PREC[h], **NORM)
    for nhwc in (False, True):
        check(evam, torch, O, coracle, gpu, pp, frames, (224, 224), h, info, nhwc=nhwc, what=f"central crop {fmt}")


STRIP_COUNTS = [1, 2, 3, 5, 8, 13, 21, 34, 64, 65, 129]


@pytest.mark.parametrize("fmt,src,dst", [("NV12", (1200, 640), (512, 272)), ("I420", (1200, 640), (512, 272)),
                                         ("NV12", (3520, 436), (640, 216)), ("BGRX", (480, 1116), (256, 544))])
@pytest.mark.parametrize("h", HALVES)
def test_strip_kernel_counts(evam, O, coracle, gpu, fmt, src, dst, h):
    """The strip kernel (paired taps; 3520 -> 640: unpaired; BGRx) over item counts, 3 distinct frames repeated: the
    family is asserted, and the n items and both guard slots are compared on the device."""
    import torch

    N = evam.native
    (W, H), (DW, DH) = src, dst
    rng = np.random.default_rng(zlib.crc32(repr((fmt, src, dst)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), W, H, pattern=p) for p in ("uniform", "gradient", "uniform")]
    imgs = upload(evam, frames, gpu)
    info = evam.PreProcInfo(precision=PREC[h], **NORM)
    ref, _ = run_oracle(O, coracle, frames, (3, 3, DH, DW), "f32", info)
    ref_dev = narrow_bits(torch, ref, h).to(gpu)
    p = evam.HipPreProcessor(device=0)
    try:
        for n in STRIP_COUNTS:
            out = half_full(torch, (n + 2, 3, DH, DW), h, gpu)
            p.convert([imgs[i % 3] for i in range(n)], out, info, slot_offset=1)
            assert p.stats().kernels == N.KERNEL_STRIP, (n, p.stats().kernels)
            got = out.view(torch.int16)
            want = ref_dev[torch.arange(n, device=gpu) % 3]
            if not torch.equal(got[1:n + 1], want):
                i = int((got[1:n + 1] != want).flatten(1).any(1).nonzero()[0])
                same_bits(torch, out[1 + i], ref_dev[i % 3].cpu(), f"{fmt} {src}->{dst} {h} x {n}: item {i}")
            assert bool((out[0] == 7).all()) and bool((out[n + 1] == 7).all()), f"x {n}: a guard slot was written"
            del out
    finally:
        p.close()


@pytest.mark.parametrize("h", HALVES)
def test_strip_c2_shape(evam, O, coracle, gpu, pp, h):
    """2 x NV12 1920 x 1080 -> 512 x 512 normalised: the headline shape, on the strip kernel."""
    import torch

    rng = np.random.default_rng(0)
    frames = [O.random_frame(rng, O.NV12, 1920, 1080, pattern=p) for p in ("uniform", "gradient")]
    info = evam.PreProcInfo(precision=PREC[h], **NORM)
    k = check(evam, torch, O, coracle, gpu, pp, frames, (512, 512), h, info, what="C2 shape")
    assert k == evam.native.KERNEL_STRIP, k


def parity_rois(rng, W, H):
    """The 104 ROIs of test_gpu_parity.test_roi_batch (the same draws after two frames from ``rng``)."""
    rois = []
    for si in range(2):
        for _ in range(50):
            w = int(rng.integers(3, 200))
            h = int(rng.integers(3, 150))
            x = int(rng.integers(-20, W - 2))
            y = int(rng.integers(-20, H - 2))
            w, h = max(w, 3 - x), max(h, 3 - y)
            rois.append((si, x, y, w, h))
    return rois + [(0, 0, 0, W, H), (1, W - 3, H - 3, 10, 10), (0, 1, 1, 1, 1), (1, 5, 7, 9, 11)]


@pytest.mark.parametrize("fmt", ["NV12", "BGRX"])
@pytest.mark.parametrize("h", HALVES)
def test_roi_batch(evam, O, coracle, gpu, pp, fmt, h):
    """104 ROIs (edge, odd and partly-outside rects, mixed geometry) -> 72 x 72 on the ROI kernel."""
    import torch

    rng = np.random.default_rng(11)
    W, H = 320, 240
    frames = [O.random_frame(rng, fc(O, fmt), W, H) for _ in range(2)]
    rois = parity_rois(rng, W, H)
    assert len(rois) == 104
    for color, norm in (("RGB", NORM), ("BGR", {})):
        info = evam.PreProcInfo(color_space=color, precision=PREC[h], **norm)
        k = check(evam, torch, O, coracle, gpu, pp, frames, (72, 72), h, info, rois=rois, what=f"roi batch {fmt} {color}")
        assert k == evam.native.KERNEL_ROI, k


@pytest.mark.parametrize("h", HALVES)
@pytest.mark.parametrize("nhwc", [False, True])
def test_explicit_slots(evam, O, coracle, gpu, pp, h, nhwc):
    """slots=[...]: a permuted table with gaps into 33 x 17 slots; unwritten slots keep 7."""
    import torch

    rng = np.random.default_rng(21)
    frames = [O.random_frame(rng, O.NV12, 120, 64, pattern="gradient" if i % 2 else "uniform") for i in range(5)]
    slots = [9, 0, 17, 4, 12]
    out = half_full(torch, (19, 3, 17, 33), h, gpu, nhwc)
    info = evam.PreProcInfo(color_space="RGB", precision=PREC[h], **NORM)
    pp.convert(upload(evam, frames, gpu), out, info, slots=slots)
    torch.cuda.synchronize()
    ref5, _ = run_oracle(O, coracle, frames, (5, 3, 17, 33), "f32", info)
    ref = np.full((19, 3, 17, 33), 7, np.float32)
    ref[slots] = ref5
    same_bits(torch, out, narrow_bits(torch, ref, h), f"explicit slots {h}")


@pytest.mark.parametrize("h", HALVES)
def test_clip_ring_stride(evam, O, coracle, gpu, pp, h):
    """A [2*16+1, 3, 24, 40] ring written at slot_offset t, slot_stride 16 for t = 0..2."""
    import torch

    rng = np.random.default_rng(8)
    shape = (2 * 16 + 1, 3, 24, 40)
    out = half_full(torch, shape, h, gpu)
    ref = np.full(shape, 7, np.float32)
    info = evam.PreProcInfo(resize="aspect-ratio", crop="central", precision=PREC[h], **NORM)
    for t in range(3):
        frames = [O.random_frame(rng, O.BGRX, 96, 54) for _ in range(2)]
        pp.convert(upload(evam, frames, gpu), out, info, slot_offset=t, slot_stride=16)
        part, _ = run_oracle(O, coracle, frames, shape, "f32", info, slot_offset=t, slot_stride=16)
        for s in (t, 16 + t):
            ref[s] = part[s]
    torch.cuda.synchronize()
    same_bits(torch, out, narrow_bits(torch, ref, h), f"ring {h}")


def test_stats_bytes(evam, O, gpu):
    """dst_bytes counts 2-byte elements; src_bytes is that of the fp32 call."""
    import torch

    N = evam.native
    rng = np.random.default_rng(2)
    imgs = upload(evam, [O.random_frame(rng, O.NV12, 160, 90) for _ in range(2)], gpu)
    p = evam.HipPreProcessor(device=0)
    try:
        p.set_option(N.OPT_STATS, 1)
        p.convert(imgs, torch.empty((2, 3, 512, 512), dtype=torch.float32, device=gpu), evam.PreProcInfo(**NORM))
        s32 = p.stats()
        assert s32.dst_bytes == 2 * 3 * 512 * 512 * 4 and s32.src_bytes > 0
        p.convert(imgs, torch.empty((2, 3, 512, 512), dtype=torch.float16, device=gpu),
                  evam.PreProcInfo(precision="FP16", **NORM))
        s16 = p.stats()
        torch.cuda.synchronize()
        assert s16.dst_bytes == 3_145_728 and s16.src_bytes == s32.src_bytes and s16.n_items == 2
    finally:
        p.close()


def test_errors_and_two_byte_base(evam, O, coracle, gpu, pp):
    import torch

    N = evam.native
    rng = np.random.default_rng(31)
    frames = [O.random_frame(rng, O.NV12, 66, 50) for _ in range(2)]
    imgs = upload(evam, frames, gpu)
    batch = evam.ImageBatch(imgs)
    # out_dtype = 4 through the C ABI
    out = torch.zeros((2, 3, 8, 16), dtype=torch.float16, device=gpu)
    t = N.EvamTensor()
    t.data, t.n, t.c, t.h, t.w, t.slot_offset, t.slot_stride = out.data_ptr(), 2, 3, 8, 16, 0, 1
    cfg = evam.PreProcInfo().to_c(4)
    rc = pp._lib.evam_pp_run(pp._h, batch.c_array, 2, None, 2, ctypes.byref(cfg), ctypes.byref(t), None)
    assert rc == N.ERR_UNSUPPORTED and b"out_dtype" in pp._lib.evam_pp_last_error()
    # std == 0 is rejected for the 16-bit types as for fp32
    cfg = evam.PreProcInfo(mean=(0, 0, 0), std=(1.0, 0.0, 1.0)).to_c(N.DTYPE_BF16)
    rc = pp._lib.evam_pp_run(pp._h, batch.c_array, 2, None, 2, ctypes.byref(cfg), ctypes.byref(t), None)
    assert rc == N.ERR_INVALID_ARG and b"std[1]" in pp._lib.evam_pp_last_error()
    # a float16 tensor without the precision stated
    for info in (None, evam.PreProcInfo(**NORM), evam.PreProcInfo(precision="BF16")):
        with pytest.raises(evam.PreProcError) as e:
            pp.convert(imgs, out, info)
        assert e.value.status == N.ERR_UNSUPPORTED and "precision" in str(e.value)
    with pytest.raises(evam.PreProcError) as e:
        pp.convert(imgs, torch.zeros((2, 3, 8, 16), device=gpu), evam.PreProcInfo(precision="FP16"))
    assert e.value.status == N.ERR_INVALID_ARG
    assert bool((out == 0).all())
    # a base that is 2-byte but not 4-byte aligned: a view starting one element into a 4-byte-aligned buffer
    n_el = 2 * 3 * 17 * 33
    ref, _ = run_oracle(O, coracle, frames, (2, 3, 17, 33), "f32", evam.PreProcInfo(**NORM))
    for h in HALVES:
        info = evam.PreProcInfo(precision=PREC[h], **NORM)
        for nhwc in (False, True):
            flat = torch.full((n_el + 4,), 7, dtype=tdt(torch, h), device=gpu)
            assert flat.data_ptr() % 4 == 0
            body = flat[1:1 + n_el]
            view = body.view(2, 17, 33, 3).permute(0, 3, 1, 2) if nhwc else body.view(2, 3, 17, 33)
            assert view.data_ptr() % 4 == 2
            pp.convert(imgs, view, info)
            torch.cuda.synchronize()
            same_bits(torch, view, narrow_bits(torch, ref, h), f"2-byte base {h} nhwc={nhwc}")
            assert float(flat[0]) == 7 and bool((flat[1 + n_el:] == 7).all())


@pytest.mark.parametrize("seed", range(24))
def test_random_configurations(evam, O, coracle, gpu, pp, seed):
    """test_gpu_parity's seeded random calls with the dtype forced to fp16 / bf16 and the normalisation replaced by one
    of the two parity normalisations; every third one channels-last. One more slot at the end keeps 7."""
    import torch

    fmt, frames, shape, _, info, rois, offset, stride = random_case(evam, O, np.random.default_rng(7000 + seed))
    h = HALVES[seed % 2]
    norm = NORM if (seed // 2) % 2 == 0 else NONE
    info = dataclasses.replace(info, precision=PREC[h], **norm)
    nhwc = seed % 3 == 2
    shape = (shape[0] + 1,) + tuple(shape[1:])
    what = f"seed {seed}: {fmt} {[(f.width, f.height) for f in frames]} -> {shape} {h} {info} " \
           f"{'%d rois' % len(rois) if rois else 'frames'} offset {offset} stride {stride} nhwc={nhwc}"
    out = half_full(torch, shape, h, gpu, nhwc)
    pp.convert(upload(evam, frames, gpu), out, info, rois=[evam.Roi(*r) for r in rois] if rois else None,
               slot_offset=offset, slot_stride=stride)
    torch.cuda.synchronize()
    ref, _ = run_oracle(O, coracle, frames, shape, "f32", info, rois=rois, slot_offset=offset, slot_stride=stride)
    assert (ref[-1] == 7).all()
    same_bits(torch, out, narrow_bits(torch, ref, h), what)


# ---- pipeline server ---------------------------------------------------------------------------------------------
@pytest.fixture
def server(evam, tmp_path):
    ps = evam.pipeline_server
    mdir = make_model_tree(str(tmp_path / "models"), {
        "det_alias": {"det_ver": (64, 64, {"json_schema_version": "2.0.0", "input_preproc": [],
                                           "output_postproc": [{"labels": ["bg", "car"]}]})}})
    yield ps, mdir
    ps.PipelineServer.stop()


def test_pipeline_f16_model(evam, O, coracle, gpu, server):
    """InferenceModel(out_dtype="f16"): the model callable receives a torch.float16 blob, written by the kernels, equal
    to the narrowed oracle tensor."""
    import torch

    ps, mdir = server
    seen = []

    def fn(t):
        seen.append((t.dtype, t.is_contiguous(), t.cpu().clone()))
        return torch.full((t.shape[0], 1, 7), -1.0)

    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir})
    ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(fn, (64, 64), name="det", out_dtype="f16"))
    rng = np.random.default_rng(3)
    frames = [O.random_frame(rng, O.NV12, 66, 50) for _ in range(3)]
    src = {"type": "frames", "frames": [{"fourcc": f.fourcc, "width": f.width, "height": f.height,
                                         "planes": f.planes} for f in frames]}
    p = ps.PipelineServer.pipeline("detect", "hip")
    p.start(source=src, destination={})
    st = p.wait(60)
    assert st["state"] == "COMPLETED", st
    assert seen and all(dt == torch.float16 and c for dt, c, _ in seen)
    got = torch.cat([t for _, _, t in seen])
    ref, _ = run_oracle(O, coracle, frames, (3, 3, 64, 64), "f32", evam.PreProcInfo())
    assert got.shape == (3, 3, 64, 64)
    same_bits(torch, got, narrow_bits(torch, ref, "f16"), "pipeline f16 blob")
