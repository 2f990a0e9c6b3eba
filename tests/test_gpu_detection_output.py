"""SSD DetectionOutput on the GPU: ``evam_pp_detection_output`` (``HipPreProcessor.detection_output``) bit for bit
against its host twin on every case of ``tests/detout_cases.py``, and a detector that returns raw heads driven through
the pipeline server's host path, its ``"device_rois"`` path and the tracked chain. The largest case has 4099 priors;
the pipeline frames are 352x198."""
import ctypes
import functools
import json
import queue

import numpy as np
import pytest

import detout_cases as DC
from test_pipeline_server import PIPES, model_dir, ps  # noqa: F401  (fixtures of the pipeline-server tests)
from test_pipeline_tracking import TRACK_PIPES

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def attrs_of(cfg):
    return {("background_label_id" if k == "background_label" else k): v for k, v in cfg.items()}


@functools.lru_cache(maxsize=None)
def host_result(name):
    """The host helper's blob and counts of a case: computed once, shared, never changed."""
    import __graft_entry__ as g

    evam = g.import_package()
    c = DC.case(name)
    out, counts = evam.detection_output_host(c["loc"], c["conf"], c["priors"], attrs_of(c["cfg"]))
    out.setflags(write=False)
    counts.setflags(write=False)
    return out, counts


def upload(torch, gpu, c):
    return tuple(torch.from_numpy(np.ascontiguousarray(c[k])).to(gpu) for k in ("loc", "conf", "priors"))


def run_device(evam, torch, gpu, pp, c, heads=None, with_counts=True):
    """``(blob, counts or None)`` of a case on the device, written between sentinel guard rows that must survive."""
    loc, conf, priors = heads if heads is not None else upload(torch, gpu, c)
    n, k = loc.shape[0], c["cfg"]["keep_top_k"]
    buf = torch.full((n * k + 2, 7), SENTINEL, dtype=torch.float32, device=gpu)
    out = buf[1:-1].view(n, k, 7)
    cbuf = torch.full((n + 2,), -7, dtype=torch.int32, device=gpu)
    got = pp.detection_output(loc, conf, priors, attrs_of(c["cfg"]), out=out, counts=cbuf[1:-1] if with_counts else None)
    assert got is out
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[0] == SENTINEL).all() and (b[-1] == SENTINEL).all(), "a guard row of out was written"
    cb = cbuf.cpu().numpy()
    assert cb[0] == -7 and cb[-1] == -7, "a guard element of counts was written"
    if not with_counts:
        assert (cb == -7).all()
    return b[1:-1].reshape(n, k, 7), (cb[1:-1].view(np.uint32) if with_counts else None)


def assert_equal(name, got, counts, want, wcounts):
    if counts is not None:
        assert counts.tolist() == wcounts.tolist(), f"{name}: counts"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        n, r, _ = bad[0]
        raise AssertionError(f"{name}: {len(bad)} elements differ, first at image {n} row {r}: device {got[n, r].tolist()} "
                             f"host {want[n, r].tolist()}")


@pytest.fixture(scope="module")
def pp(evam, gpu):
    p = evam.HipPreProcessor(device=0)
    yield p
    p.close()


@pytest.mark.parametrize("name", DC.case_names())
def test_device_equals_host(evam, gpu, pp, name):
    import torch

    got, counts = run_device(evam, torch, gpu, pp, DC.case(name))
    assert_equal(name, got, counts, *host_result(name))
    st = pp.stats()
    assert st.kernels == evam.native.KERNEL_DETOUT and st.n_launches == 2 and st.n_items == got.shape[0]


def test_counts_none(evam, gpu, pp):
    import torch

    for name in ("total_above_k", "base"):
        got, counts = run_device(evam, torch, gpu, pp, DC.case(name), with_counts=False)
        assert counts is None
        assert_equal(name, got, None, *host_result(name))


def test_half_precision_heads_are_cast(evam, gpu, pp):
    import torch

    c = DC.case("base")
    loc, conf, priors = upload(torch, gpu, c)
    out = pp.detection_output(loc.half(), conf.bfloat16(), priors, attrs_of(c["cfg"]))
    want, _ = evam.detection_output_host(loc.half().float().cpu().numpy(), conf.bfloat16().float().cpu().numpy(),
                                         c["priors"], attrs_of(c["cfg"]))
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_two_handles_in_flight(evam, gpu):
    import torch

    names = ["dense_1024", "C=21"]
    cases = [DC.case(n) for n in names]
    heads = [upload(torch, gpu, c) for c in cases]
    streams = [torch.cuda.Stream(device=gpu) for _ in names]
    pps = [evam.HipPreProcessor(device=0, stream=s) for s in streams]
    try:
        torch.cuda.synchronize()
        outs = []
        for _ in range(2):  # both handles busy at once, twice (the second round reuses their scratch)
            outs = [p.detection_output(*h, attrs_of(c["cfg"])) for p, h, c in zip(pps, heads, cases)]
        for s in streams:
            s.synchronize()
        for name, o in zip(names, outs):
            assert_equal(name, o.cpu().numpy(), None, *host_result(name))
    finally:
        for p in pps:
            p.close()


def test_scratch_growth(evam, gpu):
    import torch

    with evam.HipPreProcessor(device=0) as p:
        for name in ("one", "dense_1024_ties", "one", "N=33", "dense_1024", "chain"):
            got, counts = run_device(evam, torch, gpu, p, DC.case(name))
            assert_equal(name, got, counts, *host_result(name))


def test_non_contiguous_and_wrong_inputs_are_refused(evam, gpu, pp):
    import torch

    N = evam.native
    c = DC.case("base")
    loc, conf, priors = upload(torch, gpu, c)
    a = attrs_of(c["cfg"])
    with pytest.raises(evam.PreProcError, match="not contiguous") as e:
        pp.detection_output(loc.t().contiguous().t(), conf, priors, a)
    assert e.value.status == N.ERR_INVALID_ARG
    with pytest.raises(evam.PreProcError, match="float32"):
        pp.detection_output(loc.double(), conf, priors, a)
    with pytest.raises(evam.PreProcError, match="cuda"):
        pp.detection_output(loc.cpu(), conf, priors, a)
    with pytest.raises(evam.PreProcError, match="conf"):
        pp.detection_output(loc, conf[:, :-1].contiguous(), priors, a)
    with pytest.raises(evam.PreProcError, match="priors"):
        pp.detection_output(loc, conf, priors[:, :-4].contiguous(), a)
    with pytest.raises(evam.PreProcError, match="out must"):
        pp.detection_output(loc, conf, priors, a, out=torch.empty((3, 7, 7), device=gpu))


def test_invalid_calls_launch_nothing(evam, gpu, pp):
    """Every limit of the header, through the C entry point with valid device pointers: the status, the argument named,
    and an output that still holds its sentinel."""
    import torch

    N = evam.native
    lib = evam.load_library()
    c = DC.case("one")
    loc, conf, priors = upload(torch, gpu, c)
    out = torch.full((1, 8, 7), SENTINEL, dtype=torch.float32, device=gpu)
    good = dict(num_classes=3, background_label=0, top_k=8, keep_top_k=8, confidence_threshold=0.25, nms_threshold=0.5)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(n=1, p=3, h=pp._h, loc_=loc, out_=out, **over):
        f = dict(good, **over)
        cfg = N.EvamDetoutCfg(f["num_classes"], f["background_label"], f["top_k"], f["keep_top_k"],
                              f["confidence_threshold"], f["nms_threshold"])
        rc = lib.evam_pp_detection_output(h, None if loc_ is None else ptr(loc_), ptr(conf), ptr(priors), n, p,
                                          ctypes.byref(cfg), None if out_ is None else ptr(out_), None)
        return rc, lib.evam_pp_last_error().decode()

    bad = [(dict(n=0), "n "), (dict(n=65536), "n "), (dict(p=0), "p "), (dict(p=2 ** 30), "p "),
           (dict(num_classes=1), "num_classes"), (dict(num_classes=257), "num_classes"),
           (dict(background_label=3), "background_label"), (dict(background_label=-2), "background_label"),
           (dict(top_k=0), "top_k"), (dict(top_k=-1), "top_k"), (dict(top_k=1025), "top_k"),
           (dict(keep_top_k=0), "keep_top_k"), (dict(keep_top_k=-1), "keep_top_k"), (dict(keep_top_k=1025), "keep_top_k"),
           (dict(confidence_threshold=-0.5), "confidence_threshold"), (dict(confidence_threshold=float("nan")), "confidence_threshold"),
           (dict(confidence_threshold=float("inf")), "confidence_threshold"), (dict(nms_threshold=float("nan")), "nms_threshold"),
           (dict(nms_threshold=float("-inf")), "nms_threshold"), (dict(loc_=None), "loc"), (dict(out_=None), "out"),
           (dict(h=None), "handle")]
    for over, word in bad:
        rc, msg = call(**over)
        assert rc == N.ERR_INVALID_ARG and word in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all(), "a refused call wrote its output"
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == host_result("one")[0].tobytes()


# ---- end to end: a detector that returns raw heads ----------------------------------------------------------------------

GRID, E2E_C, E2E_FRAMES = 8, 3, 12
E2E_ATTRS = dict(num_classes=E2E_C, background_label_id=0, top_k=20, keep_top_k=10, confidence_threshold=0.3,
                 nms_threshold=0.45, code_type="caffe.PriorBoxParameter.CENTER_SIZE", share_location=True)


def grid_priors():
    pr = np.zeros((2, GRID * GRID, 4), np.float32)
    for i in range(GRID):
        for j in range(GRID):
            cx, cy = (j + 0.5) / GRID, (i + 0.5) / GRID
            pr[0, i * GRID + j] = (cx - 0.1, cy - 0.1, cx + 0.1, cy + 0.1)
    pr[1] = DC.VAR
    return pr.reshape(2, -1)


def planted_heads(rng, n_frames):
    """Heads of n_frames images: per image up to 5 planted boxes (label 1 ``car`` or 2 ``person``), each encoded on an
    even prior and, a little shifted and with a lower score, on the prior next to it."""
    pr = grid_priors().reshape(2, -1, 4)
    P = pr.shape[1]
    loc = np.zeros((n_frames, P, 4), np.float32)
    conf = np.zeros((n_frames, P, E2E_C), np.float32)
    conf[:, :, 0] = 1.0
    planted = 0

    def encode(box, p):
        x0, y0, x1, y1 = pr[0, p]
        pw, ph, pcx, pcy = x1 - x0, y1 - y0, (x0 + x1) / 2, (y0 + y1) / 2
        bw, bh, bcx, bcy = box[2] - box[0], box[3] - box[1], (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
        v = pr[1, p]
        return ((bcx - pcx) / (v[0] * pw), (bcy - pcy) / (v[1] * ph), np.log(bw / pw) / v[2], np.log(bh / ph) / v[3])

    for f in range(n_frames):
        for p in rng.choice(P // 2, int(rng.integers(1, 6)), replace=False) * 2:
            x0, y0 = rng.uniform(0.0, 0.6, 2)
            w, h = rng.uniform(0.1, 0.4, 2)
            label, score = int(rng.integers(1, 3)), float(rng.choice([0.9, 0.7]))
            loc[f, p] = encode((x0, y0, x0 + w, y0 + h), p)
            conf[f, p] = 0
            conf[f, p, label], conf[f, p, 0] = score, 1 - score
            loc[f, p + 1] = encode((x0 + 0.01, y0 + 0.01, x0 + w + 0.01, y0 + h + 0.01), p + 1)
            conf[f, p + 1] = 0
            conf[f, p + 1, label], conf[f, p + 1, 0] = score * 0.8, 1 - score * 0.8
            planted += 1
    return loc.reshape(n_frames, -1), conf.reshape(n_frames, -1), planted


def run_heads_pipeline(ps, evam, model_dir, tracked, frames, heads, twin, options):  # noqa: F811
    """(JSON lines, the classifier's inputs, fused_batches) of detect (-> track) -> classify over ``frames`` with a
    detector that returns the raw ``heads`` of the frames it is handed, or (``twin``) the blob the host helper computes
    from the same heads."""
    import torch

    loc, conf = heads
    priors = grid_priors()
    cls_in, seen = [], [0]

    def raw_detector(t):
        n = t.shape[0]
        sl = slice(seen[0], seen[0] + n)
        seen[0] += n
        return {"loc": torch.from_numpy(loc[sl]).to(t.device), "conf": torch.from_numpy(conf[sl]).to(t.device)}

    def twin_detector(t):
        n = t.shape[0]
        sl = slice(seen[0], seen[0] + n)
        seen[0] += n
        blob, _ = evam.detection_output_host(loc[sl], conf[sl], priors, E2E_ATTRS)
        return torch.from_numpy(blob).to(t.device)

    def classifier(t):
        cls_in.append(t.detach().float().cpu().numpy().copy())
        m = t[:, 0, 3, 5] * 0.5 + t[:, 2, 20, 11] * 0.25
        return {"color": torch.stack([1 - m, m], 1)}

    det = (ps.InferenceModel(twin_detector, (64, 64), name="det") if twin else
           ps.InferenceModel(raw_detector, (64, 64), name="det", detection_output=dict(E2E_ATTRS, priors=priors)))
    ps.PipelineServer.start(dict({"pipeline_dir": TRACK_PIPES if tracked else PIPES, "model_dir": model_dir,
                                  "runner": "device", "batch_max": 4}, **options))
    try:
        ps.PipelineServer.register_model("det_alias/det_ver", det)
        ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(classifier, (24, 24), name="cls"))
        qin, qout = queue.Queue(), queue.Queue()
        for f in frames:
            qin.put({"fourcc": f.fourcc, "width": f.width, "height": f.height, "planes": f.planes})
        qin.put(None)
        p = ps.PipelineServer.pipeline("detect_track_classify" if tracked else "detect_classify", "hip")
        p.start(source={"type": "application", "input": qin},
                destination={"metadata": {"type": "application", "output": qout, "mode": "json"}},
                parameters={"reclassify-interval": 1} if tracked else {"detection-properties": {"pre-process-backend": "hip"}})
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
        lines = []
        while (x := qout.get(timeout=5)) is not None:
            lines.append(json.loads(x))
        return lines, cls_in, [dict(e) for e in ps.PipelineServer.hub(0).fused_batches]
    finally:
        ps.PipelineServer.stop()


@pytest.mark.parametrize("mode", ["host", "device_rois", "tracked_device_rois"])
def test_pipeline_raw_heads(ps, evam, model_dir, gpu, O, coracle, mode):  # noqa: F811
    rng = np.random.default_rng(77)
    frames = [O.random_frame(rng, O.NV12, 352, 198, pattern="gradient" if k % 3 == 0 else "uniform")
              for k in range(E2E_FRAMES)]
    loc, conf, planted = planted_heads(rng, E2E_FRAMES)
    options = {} if mode == "host" else {"device_rois": True, "device_rois_cap": 40}
    tracked = mode.startswith("tracked")
    twin_lines, _, _ = run_heads_pipeline(ps, evam, model_dir, tracked, frames, (loc, conf), True, options)
    lines, cls_in, fused = run_heads_pipeline(ps, evam, model_dir, tracked, frames, (loc, conf), False, options)
    assert len(lines) == E2E_FRAMES and lines == twin_lines, "the published regions differ from the twin model's"
    n_obj = sum(len(d.get("objects", [])) for d in lines)
    assert planted // 2 < n_obj <= planted, (n_obj, planted)  # NMS removed every duplicate
    if mode != "host":
        assert fused and all(e["fused"] and e["reason"] is None for e in fused), fused
    crops = [(k, o["x"], o["y"], o["w"], o["h"]) for k, d in enumerate(lines) for o in d.get("objects", [])
             if "color" in o]
    assert len(crops) > 5
    if mode == "host":
        got = np.concatenate(cls_in)
    else:
        assert sum(e["count"] for e in fused) == len(crops) and len(cls_in) == len(fused)
        got = np.concatenate([t[:e["count"]] for t, e in zip(cls_in, fused)])
    assert len(got) == len(crops)
    ref = np.zeros(got.shape, np.float32)
    lut1 = O.np_norm_lut(1, (0.0, 1.0))
    for i, (k, x, y, w, h) in enumerate(crops):
        coracle.preprocess_item(frames[k], (x, y, w, h), ref, i, color_rgb=True, lut=lut1)
    bad = [i for i in range(len(crops)) if not np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32))]
    assert not bad, f"classifier rows differ: {[(i, crops[i]) for i in bad[:5]]}"
