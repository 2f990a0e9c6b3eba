"""SSD DetectionOutput on the host (no GPU): ``evam_pp_detection_output_host`` bit for bit against the float32
restatement of the rule in ``tests/detout_ref.py``, its survivors against the float64 reference on the cases decided
with margin, the targeted cases against hand-written expectations, ``evam_pp_expf`` against float64 ``exp``, every
refusal of the limits, and the Python surface (``DetectionOutputConfig``, ``InferenceModel(detection_output=...)``)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import detout_cases as DC
import detout_ref as R
from test_pipeline_server import PIPES, model_dir, ps  # noqa: F401  (fixtures of the pipeline-server tests)

F = np.float32
MAX_SKIPPED_SHARE = 0.10  # of the random cases, by the float64 check


def attrs_of(cfg):
    return {("background_label_id" if k == "background_label" else k): v for k, v in cfg.items()}


def host(evam, c):
    return evam.detection_output_host(c["loc"], c["conf"], c["priors"], attrs_of(c["cfg"]))


@functools.lru_cache(maxsize=None)
def bits_reference(name):
    c = DC.case(name)
    return R.detection_output_bits(c["loc"], c["conf"], c["priors"], c["cfg"])


@pytest.mark.parametrize("name", DC.case_names())
def test_host_equals_bit_reference(evam, name):
    got, counts = host(evam, DC.case(name))
    want, wcounts = bits_reference(name)
    assert counts.tolist() == wcounts.tolist()
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        n, r, _ = bad[0]
        raise AssertionError(f"{len(bad)} elements differ, first at image {n} row {r}: {got[n, r].tolist()} vs "
                             f"{want[n, r].tolist()}")
    # the whole block is defined: every row from the count on is (-1, 0, 0, 0, 0, 0, 0)
    for n in range(got.shape[0]):
        tail = got[n, int(counts[n]):]
        assert (tail[:, 0] == -1).all() and not tail[:, 1:].any() and not np.signbit(tail[:, 1:]).any()


@pytest.mark.parametrize("name", DC.case_names(("targeted",)))
def test_targeted_expectations(evam, name):
    c = DC.case(name)
    got, counts = host(evam, c)
    want, wcounts = DC.expected_blob(c)
    assert counts.tolist() == wcounts.tolist()
    assert got.tobytes() == want.tobytes(), (got[:, :int(counts.max()) + 1].tolist(), c["expect"])


def test_survivors_equal_float64_reference(evam):
    """On the cases the float64 reference decides with margin, the survivors (image, class, score) are its survivors; it
    may skip at most a tenth of the random cases."""
    skipped, n_random, checked = 0, 0, 0
    for c in DC.all_cases():
        if c["kind"] not in ("random", "sweep"):
            continue
        surv, margin = R.detection_output_f64(c["loc"], c["conf"], c["priors"], c["cfg"])
        if c["kind"] == "random":
            n_random += 1
            skipped += not margin
        if not margin:
            continue
        got, counts = host(evam, c)
        C = c["cfg"]["num_classes"]
        conf = c["conf"].reshape(c["conf"].shape[0], -1, C)
        want = sorted((n, cl, conf[n, p, cl].view(np.uint32).item()) for n, cl, p in surv)
        assert sorted(R.blob_rows(got, counts)) == want, c["name"]
        assert len(surv) == int(counts.sum())
        checked += 1
    print(f"float64 check: {checked} cases checked, {skipped} of {n_random} random cases skipped")
    assert n_random >= 20 and skipped <= MAX_SKIPPED_SHARE * n_random, (skipped, n_random)


def test_expf(evam):
    lib = evam.load_library()
    f = lib.evam_pp_expf
    assert f(0.0) == 1.0 and f(-0.0) == 1.0
    assert math.isnan(f(float("nan")))
    assert f(float("inf")) == math.inf and f(89.5) == math.inf and f(1e30) == math.inf
    assert f(float("-inf")) == 0.0 and f(-104.5) == 0.0 and f(-1e30) == 0.0
    assert f(-103.0) == float(np.float32(math.exp(-103.0)))  # subnormal, rounded once
    assert f(88.0) == float(np.float32(math.exp(88.0))) or abs(f(88.0) / math.exp(88.0) - 1) < 3e-7
    # a strided subset of [-20, 20]: every 2^15-th float32 of each sign, and the neighbourhood of the reduction's borders
    top = np.float32(20.0).view(np.uint32).item()
    u = np.arange(0, top + 1, 1 << 15, dtype=np.uint32)
    xs = np.concatenate([-(u.view(F)[::-1]), u.view(F), np.float32([20.0, -20.0])])
    borders = (np.arange(-28, 29)[:, None] + 0.5) * math.log(2) + np.arange(-8, 9)[None, :] * 1e-6
    xs = np.sort(np.concatenate([xs, borders.astype(F).ravel()]))
    xs = xs[(xs >= -20) & (xs <= 20)]
    got = np.array([f(float(x)) for x in xs], F)
    assert got.tobytes() == R.expf_bits(xs).tobytes(), "the library and the Python restatement differ"
    want64 = np.exp(xs.astype(np.float64))
    ulp = np.spacing(want64.astype(F)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want64) / ulp
    print(f"evam_pp_expf: {len(xs)} points, max error {err.max():.4f} ulp at x = {xs[err.argmax()]!r}")
    assert err.max() <= 2.0
    assert (np.diff(got) >= 0).all(), "not monotone"


def test_blob_feeds_the_roi_calls(evam):
    """The blob is what evam_pp_ssd_rois_host and parse_ssd_batch read: both give the same rects."""
    import device_rois_cases as RC

    c = DC.case("C=21")
    blob, counts = host(evam, c)
    sizes = [(352, 198), (320, 180), (64, 48)][:blob.shape[0]]
    b = RC.Batch(blob, sizes, None, RC.TENSOR, 0.5, None)
    want = RC.python_rois(evam, b)  # parse_ssd_batch -> detections_to_regions -> roi_inside
    got, total = RC.host_rois(evam, b)
    assert total == len(want) and total > 10
    assert [tuple(r) for r in got.tolist()] == want


REFUSALS = [
    (dict(n=0), "n "), (dict(n=65536), "n "), (dict(p=0), "p "), (dict(p=2 ** 30), "p "),
    (dict(num_classes=1), "num_classes"), (dict(num_classes=257), "num_classes"),
    (dict(background_label=3), "background_label"), (dict(background_label=-2), "background_label"),
    (dict(top_k=0), "top_k"), (dict(top_k=-1), "top_k"), (dict(top_k=1025), "top_k"),
    (dict(keep_top_k=0), "keep_top_k"), (dict(keep_top_k=-1), "keep_top_k"), (dict(keep_top_k=1025), "keep_top_k"),
    (dict(confidence_threshold=-0.5), "confidence_threshold"), (dict(confidence_threshold=float("nan")), "confidence_threshold"),
    (dict(confidence_threshold=float("inf")), "confidence_threshold"), (dict(nms_threshold=float("nan")), "nms_threshold"),
    (dict(nms_threshold=float("inf")), "nms_threshold"), (dict(loc=None), "loc"), (dict(conf=None), "conf"),
    (dict(priors=None), "priors"), (dict(out=None), "out"), (dict(cfg=None), "cfg"),
]


@pytest.mark.parametrize("over,word", REFUSALS, ids=[f"{next(iter(o))}={next(iter(o.values()))}" for o, _ in REFUSALS])
def test_refusals(evam, over, word):
    N = evam.native
    lib = evam.load_library()
    c = DC.case("one")
    arrays = dict(loc=c["loc"], conf=c["conf"], priors=c["priors"], out=np.full((1, 8, 7), 7.0, F))
    f = dict(num_classes=3, background_label=0, top_k=8, keep_top_k=8, confidence_threshold=0.25, nms_threshold=0.5,
             n=1, p=3, cfg=True, **arrays)
    f.update(over)
    cfg = N.EvamDetoutCfg(f["num_classes"], f["background_label"], f["top_k"], f["keep_top_k"], f["confidence_threshold"],
                          f["nms_threshold"])
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.evam_pp_detection_output_host(ptr(f["loc"]), ptr(f["conf"]), ptr(f["priors"]), f["n"], f["p"],
                                           ctypes.byref(cfg) if f["cfg"] else None, ptr(f["out"]), None)
    msg = lib.evam_pp_last_error().decode()
    assert rc == N.ERR_INVALID_ARG and word in msg and "evam_pp_detection_output_host" in msg, (rc, msg)
    assert (arrays["out"] == 7.0).all()


def test_counts_are_optional(evam):
    lib = evam.load_library()
    c = DC.case("total_above_k")
    cfg = evam.DetectionOutputConfig.from_attributes(attrs_of(c["cfg"])).to_c()
    out = np.zeros((2, 2, 7), F)
    assert lib.evam_pp_detection_output_host(c["loc"].ctypes.data, c["conf"].ctypes.data, c["priors"].ctypes.data, 2, 4,
                                             ctypes.byref(cfg), out.ctypes.data, None) == 0
    assert out.tobytes() == DC.expected_blob(c)[0].tobytes()


def test_config_from_attributes(evam):
    N = evam.native
    ok = dict(num_classes=21, keep_top_k=[200], top_k=400, background_label_id=0, confidence_threshold=0.01,
              nms_threshold=0.45, code_type="caffe.PriorBoxParameter.CENTER_SIZE", share_location="true", normalized=True,
              variance_encoded_in_target=False, clip_before_nms=False, clip_after_nms="false", decrease_label_id=0,
              input_height=1, input_width=1)
    cfg = evam.DetectionOutputConfig.from_attributes(ok)
    assert (cfg.num_classes, cfg.keep_top_k, cfg.top_k, cfg.background_label) == (21, 200, 400, 0)
    c = cfg.to_c()
    assert ctypes.sizeof(c) == 24 and abs(c.nms_threshold - 0.45) < 1e-7
    d = evam.DetectionOutputConfig.from_attributes(dict(num_classes=2, keep_top_k=5))
    assert (d.top_k, d.background_label, d.confidence_threshold, d.nms_threshold) == (400, 0, 0.01, 0.45)
    unsupported = [dict(code_type="caffe.PriorBoxParameter.CORNER"), dict(share_location=False), dict(normalized=False),
                   dict(variance_encoded_in_target=True), dict(clip_before_nms=True), dict(clip_after_nms=True),
                   dict(decrease_label_id=True), dict(top_k=-1), dict(keep_top_k=-1), dict(keep_top_k=[200, 100])]
    for over in unsupported:
        with pytest.raises(evam.PreProcError) as e:
            evam.DetectionOutputConfig.from_attributes(dict(ok, **over))
        assert e.value.status == N.ERR_UNSUPPORTED and next(iter(over)) in str(e.value), (over, str(e.value))
    invalid = [dict(num_classes=1), dict(num_classes=300), dict(top_k=0), dict(top_k=2000), dict(keep_top_k=0),
               dict(background_label_id=21), dict(confidence_threshold=-1), dict(confidence_threshold=float("nan")),
               dict(nms_threshold=float("inf")), dict(num_classes="many"), dict(no_such_attribute=1)]
    for over in invalid:
        with pytest.raises(evam.PreProcError) as e:
            evam.DetectionOutputConfig.from_attributes(dict(ok, **over))
        assert e.value.status == N.ERR_INVALID_ARG, (over, str(e.value))
    for missing in ("num_classes", "keep_top_k"):
        with pytest.raises(evam.PreProcError, match=missing):
            evam.DetectionOutputConfig.from_attributes({k: v for k, v in ok.items() if k != missing})
    with pytest.raises(evam.PreProcError):
        evam.detection_output_host(np.zeros((1, 8), F), np.zeros((1, 5), F), np.zeros((2, 8), F), dict(num_classes=2, keep_top_k=1))


def test_inference_model_refused_at_start(ps, evam, model_dir):  # noqa: F811
    """A detector whose detection_output the rule does not serve is refused when the pipeline starts; the field's
    default leaves the model as it was."""
    import queue

    assert ps.InferenceModel(None, (64, 64)).detection_output is None
    priors = np.zeros((2, 8), F)
    good = dict(num_classes=3, keep_top_k=10, priors=priors)
    bad = [(dict(good, code_type="CORNER"), evam.native.ERR_UNSUPPORTED, "code_type"),
           (dict(good, top_k=-1), evam.native.ERR_UNSUPPORTED, "top_k"),
           (dict(num_classes=3, keep_top_k=10), evam.native.ERR_INVALID_ARG, "priors"),
           (dict(good, priors=np.zeros((2, 7), F)), evam.native.ERR_INVALID_ARG, "priors"),
           (dict(good, keep_top_k=5000), evam.native.ERR_INVALID_ARG, "keep_top_k")]
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": model_dir, "runner": "device"})
    try:
        ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(lambda t: t, (24, 24), name="cls"))
        for spec, status, word in bad:
            ps.PipelineServer.register_model("det_alias/det_ver",
                                             ps.InferenceModel(lambda t: t, (64, 64), name="det", detection_output=spec))
            p = ps.PipelineServer.pipeline("detect_classify", "hip")
            with pytest.raises(evam.PreProcError) as e:
                p.start(source={"type": "application", "input": queue.Queue()},
                        destination={"metadata": {"type": "application", "output": queue.Queue(), "mode": "json"}})
            assert e.value.status == status and word in str(e.value), str(e.value)
        spec = ps.detection_output_spec(ps.InferenceModel(None, (64, 64), detection_output=good))
        assert spec[0].keep_top_k == 10 and spec[1].shape == (2, 8)
    finally:
        ps.PipelineServer.stop()
