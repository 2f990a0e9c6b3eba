"""GPU JPEG decoding to raw 4:2:0 planes (evam_pp_decode_jpeg_planes), byte for byte.

The references are the fixtures' stored Pillow (libjpeg-turbo) planes and ``evam_pp_decode_jpeg_planes_host``, the host
twin that shares the kernel's row tasks and clipped stores and that tests/test_jpeg_planes_host.py pins to Pillow.
Every output lies inside one buffer of noise that is compared whole, so a byte written outside the pixel bytes shows.
Nothing here imports Pillow."""
import queue

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_planes_cases as PC
from test_pipeline_server import PIPES, make_model_tree

pytestmark = pytest.mark.gpu

FORMATS = ("NV12", "I420")
S_BITS = C.source_constant("kJdecSubBits")
T_SUBS = C.source_constant("kJdecChunk")


@pytest.fixture(scope="module")
def pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


def device_decode(evam, gpu, pp, files, surface):
    """(the surface's buffer after the decode, the statuses)."""
    import torch

    buf, imgs = surface.device_images(evam, torch, gpu)
    status = torch.full((len(files),), 77, dtype=torch.int32, device=gpu)
    pp.decode_jpeg_into(files, imgs, status)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), status.cpu().numpy()


def host_planes(evam, files, fmt):
    """The host twin's compact planes of every file, and its statuses."""
    N = evam.native
    return N.decode_jpeg_planes_host(files, N.FOURCC_NV12 if fmt == "NV12" else N.FOURCC_I420)


def check_twin(evam, gpu, pp, files, fmt, kinds, what, seed=0):
    """Decode on the device into a surface of ``kinds``: the whole buffer equals the noise with the host twin's
    pixel bytes pasted in, and every status is 0."""
    i = evam.native.jpeg_info_struct(files[0])
    ref, ref_status = host_planes(evam, files, fmt)
    s = PC.Surface(fmt, i.width, i.height, kinds, seed)
    got, status = device_decode(evam, gpu, pp, files, s)
    assert status.tolist() == ref_status.tolist() == [0] * len(files), what
    diff = PC.first_difference(got, s.expected(ref))
    assert not diff, f"{what} {fmt} {kinds}: {diff}"


@pytest.mark.parametrize("fmt", FORMATS)
def test_fixtures_equal_pillow_and_the_twin(evam, gpu, pp, fmt):
    N = evam.native
    for k, (name, (f, ycc)) in enumerate(PC.fixtures().items()):
        h, w = ycc[0].shape
        s = PC.Surface(fmt, w, h, [PC.KINDS[k % len(PC.KINDS)]], seed=k)
        got, status = device_decode(evam, gpu, pp, [f], s)
        assert status.tolist() == [0], name
        diff = PC.first_difference(got, s.expected([PC.planes_of(ycc, fmt)]))
        assert not diff, f"{name}: {diff}"
        twin, twin_status = host_planes(evam, [f], fmt)
        assert twin_status.tolist() == [0] and not PC.first_difference(got, s.expected(twin)), name
    st = pp.stats()
    assert st.kernels == N.KERNEL_JPEG_DEC and st.n_launches == 5


def nv12_images(evam, O, gpu, n, w, h, seed):
    rng = np.random.default_rng(seed)
    frames = [O.random_frame(rng, O.NV12, w, h, pitch_align=64, pattern="gradient" if i % 3 == 1 else "uniform")
              for i in range(n)]
    return [evam.Image.from_host(f.fourcc, f.width, f.height, f.planes, device=gpu) for f in frames]


@pytest.mark.parametrize("h", range(2, 35, 2))
def test_edge_residues(evam, O, gpu, pp, h):
    """Every even W in 2..34 at this height (all residues of the 16x16 MCU: 2x2 has byte stores only, 16x16 no clip,
    24x8 a luma block wholly outside, 10x10 five chroma pixels): files of encode_jpeg of random NV12 frames, two per
    call, against the host twin, the buffer compared whole."""
    for w in range(2, 35, 2):
        files = pp.encode_jpeg(nv12_images(evam, O, gpu, 2, w, h, 1000 * h + w), 95)
        check_twin(evam, gpu, pp, files, FORMATS[(w + h) // 2 % 2], ["unequal", "base16"], f"{w}x{h}", seed=w)


@pytest.mark.parametrize("fmt", FORMATS)
def test_layouts(evam, gpu, pp, fmt):
    """Three files per call, each out[i] in another layout kind; afterwards the noise is intact."""
    fx = PC.fixtures()
    for size in ("10x10", "30x46", "64x48"):
        files = [fx[f"grad_{size}_q90"][0], fx[f"sat_{size}_q100"][0], fx[f"grad_{size}_q90"][0]]
        for k in range(len(PC.KINDS)):
            kinds = [PC.KINDS[(k + j) % len(PC.KINDS)] for j in range(3)]
            check_twin(evam, gpu, pp, files, fmt, kinds, size, seed=k)


@pytest.mark.parametrize("fmt", FORMATS)
def test_1080p(evam, O, gpu, pp, fmt):
    """The bottom MCU row is half outside the frame, and the scan is longer than one chunk of evam_jdec_sync."""
    files = pp.encode_jpeg(nv12_images(evam, O, gpu, 1, 1920, 1080, 1080), 90)
    assert len(files[0]) * 8 > 2 * S_BITS * T_SUBS and 1080 % 16 == 8
    check_twin(evam, gpu, pp, files, fmt, ["unequal"], "1920x1080")


@pytest.mark.parametrize("fmt", FORMATS)
def test_restart_intervals_and_long_thin_frames(evam, O, gpu, pp, fmt):
    f, ycc = PC.fixtures()["rstrow_320x180_q75"]
    assert evam.jpeg_info(f).restart_interval == 20
    s = PC.Surface(fmt, 320, 180, ["window", "reversed"], seed=5)
    got, status = device_decode(evam, gpu, pp, [f, f], s)
    assert status.tolist() == [0, 0]
    assert not PC.first_difference(got, s.expected([PC.planes_of(ycc, fmt)] * 2))
    for w, h in ((4096, 16), (16, 4096)):
        files = pp.encode_jpeg(nv12_images(evam, O, gpu, 2, w, h, w), 90)
        check_twin(evam, gpu, pp, files, fmt, ["base16", "window"], f"{w}x{h}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_damaged_file_between_two_good_ones(evam, gpu, pp, fmt):
    N = evam.native
    fx = PC.fixtures()
    a, b = fx["dec/noise_64x48_420"], fx["grad_64x48_q90"]
    bad = C.damaged_scans()[1][1]
    assert len({a[0], bad, b[0]}) == 3
    s = PC.Surface(fmt, 64, 48, ["window", "reversed", "unequal"], seed=7)
    got, status = device_decode(evam, gpu, pp, [a[0], bad, b[0]], s)
    _, twin_status = host_planes(evam, [a[0], bad, b[0]], fmt)
    assert status.tolist() == twin_status.tolist() == [0, N.ERR_INVALID_ARG, 0]
    assert s.outside_intact(got)
    want = s.expected([PC.planes_of(a[1], fmt), s.extract(got, 1), PC.planes_of(b[1], fmt)])
    assert not PC.first_difference(got, want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_damaged_scans(evam, gpu, pp, fmt):
    """The fixed damaged scans that are even-sized 4:2:0 files: the status agrees with the host twin and nothing
    outside the file's pixel bytes is written."""
    N = evam.native
    n = 0
    for k, (name, f, must_fail) in enumerate(C.damaged_scans()):
        if not evam.jpeg_planes_ok(evam.jpeg_info(f)):
            continue
        s = PC.Surface(fmt, 64, 48, [PC.KINDS[k % len(PC.KINDS)]], seed=k)
        got, status = device_decode(evam, gpu, pp, [f], s)
        _, want = host_planes(evam, [f], fmt)
        assert status[0] in (0, N.ERR_INVALID_ARG) and (status[0] != 0) == (want[0] != 0), (name, status, want)
        assert status[0] != 0 or not must_fail, name
        assert s.outside_intact(got), name
        n += 1
    assert n >= 10


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_then_convert_without_a_synchronisation(evam, O, coracle, gpu, pp, fmt):
    """decode_jpeg(files, fmt) and convert on one handle, nothing in between: a full-frame downscale and a small ROI
    batch equal the oracle run on the host twin's planes."""
    import torch

    N = evam.native
    fc = N.FOURCC_NV12 if fmt == "NV12" else N.FOURCC_I420
    files = pp.encode_jpeg(nv12_images(evam, O, gpu, 3, 320, 180, 11), 90)
    rois = [(0, 10, 10, 100, 60), (1, 0, 0, 320, 180), (2, 200, 100, 120, 80), (0, 33, 17, 51, 39)]
    full = torch.zeros((3, 3, 72, 128), dtype=torch.uint8, device=gpu)
    crops = torch.zeros((4, 3, 32, 32), dtype=torch.uint8, device=gpu)
    imgs = pp.decode_jpeg(files, fmt)
    pp.convert(imgs, full)
    pp.convert(imgs, crops, rois=[evam.Roi(*r) for r in rois])
    torch.cuda.synchronize()
    assert [(im.fourcc, im.width, im.height) for im in imgs] == [(fc, 320, 180)] * 3
    planes, status = host_planes(evam, files, fmt)
    assert status.tolist() == [0, 0, 0]
    frames = [O.HostFrame(O.NV12 if fmt == "NV12" else O.I420, 320, 180, p) for p in planes]
    ref_full, ref_crops = np.zeros((3, 3, 72, 128), np.uint8), np.zeros((4, 3, 32, 32), np.uint8)
    for i, f in enumerate(frames):
        coracle.preprocess_item(f, None, ref_full, i)
    for i, (k, x, y, w, h) in enumerate(rois):
        coracle.preprocess_item(frames[k], (x, y, w, h), ref_crops, i)
    assert np.array_equal(full.cpu().numpy(), ref_full)
    assert np.array_equal(crops.cpu().numpy(), ref_crops)


def test_fallback(evam, gpu, pp):
    """A 4:4:4 and an odd-sized file among 4:2:0 files come back as BGRX, equal to decode_jpeg's default; the others
    come back as planes."""
    N = evam.native
    fx, pfx = C.fixtures(), PC.fixtures()
    names = ["grad_64x48_q90", "noise_64x48_444", "sat_10x10_q100", "rst1_33x17_420", "sat_64x48_q100"]
    files = [pfx[k][0] if k in pfx else fx[k][0] for k in names]
    default = pp.decode_jpeg(files)
    for fmt, fc in (("NV12", N.FOURCC_NV12), ("I420", N.FOURCC_I420)):
        imgs = pp.decode_jpeg(files, fmt, fallback="BGRX")
        assert [im.fourcc for im in imgs] == [fc, N.FOURCC_BGRX, fc, N.FOURCC_BGRX, fc]
        for k in (1, 3):
            w, h = imgs[k].width, imgs[k].height
            assert (w, h) == (default[k].width, default[k].height)
            assert np.array_equal(imgs[k].planes[0].cpu().numpy()[:, :4 * w], default[k].planes[0].cpu().numpy()[:, :4 * w])
            assert np.array_equal(imgs[k].planes[0].cpu().numpy()[:, :4 * w].reshape(h, w, 4)[..., :3], fx[names[k]][1])
        for k in (0, 2, 4):
            for got, want in zip(imgs[k].planes, PC.planes_of(pfx[names[k]][1], fmt)):
                assert np.array_equal(got.cpu().numpy()[:, :want.shape[1]], want), (fmt, names[k])
        with pytest.raises(evam.PreProcError, match=r"files\[1\]") as e:
            pp.decode_jpeg(files, fmt)
        assert e.value.status == N.ERR_UNSUPPORTED


# ---- pipeline server ---------------------------------------------------------------------------------------------
@pytest.fixture
def server(evam, tmp_path):
    ps = evam.pipeline_server
    mdir = make_model_tree(str(tmp_path / "models"), {
        "det_alias": {"det_ver": (64, 64, {"json_schema_version": "2.0.0", "input_preproc": [],
                                           "output_postproc": [{"labels": ["bg", "car"]}]})}})
    yield ps, mdir
    ps.PipelineServer.stop()


def run_pipeline(ps, frames, seen, **source):
    import torch

    def detector(t):
        seen.append(t.detach().cpu().numpy().copy())
        out = torch.full((t.shape[0], 1, 7), -1.0)
        out[:, 0] = torch.tensor([0, 1, 0.9, 0.25, 0.25, 0.5, 0.75])
        return out

    ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
    qout = queue.Queue()
    p = ps.PipelineServer.pipeline("detect", "hip")
    p.start(source={"type": "frames", "frames": frames, **source},
            destination={"metadata": {"type": "application", "output": qout, "mode": "json"}})
    st = p.wait(60)
    lines = []
    while (x := qout.get(timeout=5)) is not None:
        lines.append(x)
    return st, lines


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_pipeline_jpeg_format_i420(evam, gpu, pp, server, runner):
    """A detect pipeline with "jpeg_format": "I420": the detector's tensors equal those of the same frames submitted
    as host I420 frames (the host twin's planes), and a 4:4:4 file in the stream gives the tensor of the default BGRX
    route."""
    ps, mdir = server
    N = evam.native
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir, "runner": runner})
    fx, pfx = C.fixtures(), PC.fixtures()
    files = [fx["noise_64x48_420"][0], pfx["grad_64x48_q90"][0], fx["noise_64x48_444"][0], pfx["rstrow_64x48_q90"][0]]
    a_seen, b_seen, c_seen = [], [], []
    st, a_lines = run_pipeline(ps, list(files), a_seen, jpeg_format="I420")
    assert st["state"] == "COMPLETED", st
    twins = []
    for k, f in enumerate(files):
        if k == 2:
            twins.append(pp.decode_jpeg([f])[0])
        else:
            planes, status = host_planes(evam, [f], "I420")
            assert status.tolist() == [0]
            twins.append({"fourcc": N.FOURCC_I420, "width": 64, "height": 48, "planes": planes[0],
                          "timestamp": k})  # a dict item carries its own timestamp; a file's is its frame index
    st, b_lines = run_pipeline(ps, twins, b_seen)
    assert st["state"] == "COMPLETED", st
    assert len(a_lines) == 4 and a_lines == b_lines
    a, b = np.concatenate(a_seen), np.concatenate(b_seen)
    assert a.shape[0] == 4 and np.array_equal(a, b)
    st, _ = run_pipeline(ps, list(files), c_seen)  # the default route: BGRX for every file
    assert st["state"] == "COMPLETED", st
    c = np.concatenate(c_seen)
    assert np.array_equal(a[2], c[2])
    assert not np.array_equal(a[0], c[0])  # raw planes and libjpeg's default decode differ by design
    with pytest.raises(evam.PreProcError, match="jpeg_format"):
        run_pipeline(ps, [files[0]], [], jpeg_format="RGB")
