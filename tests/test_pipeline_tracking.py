"""gvatrack in a running pipeline (CPU: the HIP pre-processor is the recording stub of test_pipeline_runner, the tracker
itself runs on the host): the ids both JSON shapes publish equal ``tests/track_ref.py`` on the stub detector's boxes,
``reclassify-interval`` sends a persistent object to the classifier on every N-th frame only, and the tracking types
that need image features are refused when the pipeline starts. Both runners."""
import json
import os
import queue

import pytest
import torch

import track_ref as R
from test_pipeline_runner import StubPP, frames, stubbed  # noqa: F401  (fixture)
from test_pipeline_server import PIPES, REF_PIPES, make_model_tree, model_dir  # noqa: F401  (fixture)

W, H = 64, 48
N_FRAMES = 12
# the gvatrack template lives beside tests/pipelines, whose exact contents test_pipeline_server pins
TRACK_PIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pipelines_tracking")


def boxes_at(f):
    """The stub detector's rows of frame f: (label, confidence, x0, y0, x1, y1), normalised."""
    rows = [(1, 0.9, (4 + f) / W, 8 / H, (24 + f) / W, 28 / H),          # a car that drifts right: one id throughout
            (0, 0.8, 40 / W, 4 / H, 60 / W, 20 / H)]                      # label "bg": tracked, never classified
    if 2 <= f <= 5:
        rows.insert(1, (1, 0.7, 30 / W, 30 / H, 44 / W, 46 / H))         # a second car for four frames
    if f >= 9:
        rows.append((1, 0.7, 30 / W, 30 / H, 44 / W, 46 / H))            # ... and where it stood, later: a new id
    rows.append((1, 0.6, 0.5, 0.5, 0.5, 0.9))                             # zero width: roi_inside rejects it, id 0
    return rows


def register(ps, sent):
    state = {"frame": 0}

    def detector(t):
        out = torch.full((t.shape[0], 8, 7), -1.0)
        for i in range(t.shape[0]):
            for j, (label, conf, *box) in enumerate(boxes_at(state["frame"])):
                out[i, j] = torch.tensor([0, label, conf, *box])
            state["frame"] += 1
        return out

    def classifier(t):
        sent.append(t.shape[0])
        return {"color": torch.stack([torch.zeros(t.shape[0]), torch.ones(t.shape[0])], 1)}

    ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
    ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(classifier, (24, 24), name="cls"))


def reference(evam, max_lost, classify_label=1, reclassify=1):
    """Per frame: (ids of all regions in order, due flags), by track_ref on the regions the host path builds."""
    P, roi_inside = evam.postproc, evam.pipeline_server.roi_inside
    trk = R.Tracker(max_lost)
    out = []
    for f in range(N_FRAMES):
        rects = [P.roi_rect(tuple(float(torch.tensor(v, dtype=torch.float32)) for v in row[2:]), W, H)
                 for row in boxes_at(f)]
        labels = [row[0] for row in boxes_at(f)]
        keep = [i for i, r in enumerate(rects) if roi_inside(*r, W, H)]
        ids, due = trk.step(f, [rects[i] for i in keep], [labels[i] for i in keep], [classify_label], reclassify)
        full, full_due = [0] * len(rects), [False] * len(rects)
        for i, a, d in zip(keep, ids, due):
            full[i], full_due[i] = a, d
        out.append((full, full_due))
    return out


def run(ps, pre, mdir, runner, params, sent):
    ps.PipelineServer.start({"pipeline_dir": TRACK_PIPES, "model_dir": mdir, "runner": runner})
    register(ps, sent)
    qout = queue.Queue()
    p = ps.PipelineServer.pipeline("detect_track_classify", "hip")
    p.start(source={"type": "frames", "frames": frames(pre, N_FRAMES, W, H)},
            destination={"metadata": {"type": "application", "output": qout, "mode": "frames"}}, parameters=params)
    st = p.wait(60)
    assert st["state"] == "COMPLETED", st
    results = []
    while (x := qout.get(timeout=5)) is not None:
        results.append(x[1])
    assert len(results) == N_FRAMES
    return results


@pytest.mark.parametrize("runner", ["device", "threads"])
@pytest.mark.parametrize("tracking_type,max_lost", [(None, 8), ("zero-term-imageless", 0)])
def test_ids_in_both_json_shapes(stubbed, evam, runner, tracking_type, max_lost):
    ps, pre, mdir = stubbed
    P = evam.postproc
    params = {"detection-properties": {"batch-size": 3}, "tracking-device": "GPU"}
    if tracking_type:
        params["tracking-type"] = tracking_type
    results = run(ps, pre, mdir, runner, params, [])
    want = reference(evam, max_lost)
    seen = set()
    for f, fr in enumerate(results):
        ids = want[f][0]
        conv = json.loads(P.gvametaconvert_json(fr))
        assert [o.get("id", 0) for o in conv["objects"]] == ids, f
        assert all(("id" in o) == bool(i) for o, i in zip(conv["objects"], ids))
        assert [g["object_id"] for g in P.publisher_meta(fr)["gva_meta"]] == ids, f
        assert ids[0] == 1 and ids[-1] == 0          # the drifting car keeps id 1; the degenerate box has none
        seen.update(ids)
    # the second car's two appearances, four and more frames apart: one id with max_lost 8, two with 0
    assert results[9].regions[2].object_id == (results[2].regions[1].object_id if max_lost == 8 else 4)
    assert seen == ({0, 1, 2, 3} if max_lost == 8 else {0, 1, 2, 3, 4})


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_reclassify_interval_on_tracked_objects(stubbed, evam, runner):
    ps, pre, mdir = stubbed
    sent = []
    results = run(ps, pre, mdir, runner, {"reclassify-interval": 3}, sent)
    want = reference(evam, 8, reclassify=3)
    # the classifier sees exactly the due regions (a call may hold several frames of the stream)
    assert sum(sent) == sum(sum(d) for _, d in want), sent
    assert [f for f, (_, d) in enumerate(want) if d[0]] == [0, 3, 6, 9]      # the persistent car: every third frame
    assert sum(sent) < sum(sum(1 for r in fr.regions if r.label == "car" and r.w > 0) for fr in results)
    for f, fr in enumerate(results):
        car = fr.regions[0]
        assert car.object_id == 1
        assert [t.name for t in car.tensors] == ["detection", "color"], f      # results attached on every frame
        assert [t.name for t in fr.regions[-1].tensors] == ["detection"]       # degenerate: never classified


@pytest.mark.parametrize("runner", ["device", "threads"])
@pytest.mark.parametrize("kind", ["zero-term", "short-term"])
def test_tracking_types_that_need_image_features_are_refused(stubbed, evam, runner, kind):
    ps, pre, mdir = stubbed
    ps.PipelineServer.start({"pipeline_dir": TRACK_PIPES, "model_dir": mdir, "runner": runner})
    register(ps, [])
    p = ps.PipelineServer.pipeline("detect_track_classify", "hip")
    with pytest.raises(evam.native.PreProcError) as e:
        p.start(source={"type": "frames", "frames": frames(pre, 2, W, H)}, destination={},
                parameters={"tracking-type": kind})
    assert e.value.status == evam.native.ERR_UNSUPPORTED and "image features" in str(e.value)


def test_detector_interval_frames_are_not_tracked(stubbed, evam):
    """On a frame the detector skipped, tracks are neither aged nor emitted: with inference-interval 2 and max_lost 0
    the car still keeps its id over the detector's frames."""
    ps, pre, mdir = stubbed
    results = run(ps, pre, mdir, "device", {"inference-interval": 2, "tracking-type": "zero-term-imageless"}, [])
    for f, fr in enumerate(results):
        if f % 2:
            assert not fr.regions
        else:
            assert fr.regions[0].object_id == 1, f


@pytest.mark.skipif(not os.path.isdir(REF_PIPES), reason="reference templates only in the build container")
@pytest.mark.parametrize("name", ["person_vehicle_bike", "object_line_crossing"])
def test_reference_tracking_templates_publish_ids(evam, monkeypatch, tmp_path, name):
    """The reference's two ``gvadetect ! gvatrack ! gvaclassify`` templates start as they are and publish ids."""
    ps, pre = evam.pipeline_server, evam.preproc
    monkeypatch.setattr(pre, "HipPreProcessor", StubPP)
    monkeypatch.setattr(ps._InferenceStage, "_tensor",
                        lambda self, n: torch.zeros((n, 3, self.model.input_size[1], self.model.input_size[0])))
    monkeypatch.setenv("DETECTION_DEVICE", "GPU")
    monkeypatch.setenv("CLASSIFICATION_DEVICE", "GPU")
    mdir = make_model_tree(str(tmp_path / "models"), {
        "object_detection": {"person_vehicle_bike": (64, 64, {"input_preproc": [],
                                                              "output_postproc": [{"labels": ["person", "vehicle"]}]})},
        "object_classification": {"vehicle_attributes": (24, 24, {"input_preproc": [], "output_postproc": [
            {"layer_name": "color", "attribute_name": "color", "labels": ["dark", "light"], "method": "max"}]})}})
    try:
        ps.PipelineServer.start({"pipeline_dir": REF_PIPES, "model_dir": mdir})
        state = {"frame": 0}

        def detector(t):
            out = torch.full((t.shape[0], 8, 7), -1.0)
            for i in range(t.shape[0]):
                for j, (label, conf, *box) in enumerate(boxes_at(state["frame"])):
                    out[i, j] = torch.tensor([0, label, conf, *box])
                state["frame"] += 1
            return out

        ps.PipelineServer.register_model("object_detection/person_vehicle_bike",
                                         ps.InferenceModel(detector, (64, 64), name="det"))
        ps.PipelineServer.register_model("object_classification/vehicle_attributes", ps.InferenceModel(
            lambda t: {"color": torch.stack([torch.zeros(t.shape[0]), torch.ones(t.shape[0])], 1)}, (24, 24), name="cls"))
        qout = queue.Queue()
        p = ps.PipelineServer.pipeline("object_tracking", name)
        p.start(source={"type": "frames", "frames": frames(pre, N_FRAMES, W, H)},
                destination={"metadata": {"type": "application", "output": qout, "mode": "json"}},
                parameters={"tracking-type": "short-term-imageless", "reclassify-interval": 2})
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
        lines = []
        while (x := qout.get(timeout=5)) is not None:
            lines.append(json.loads(x))
        assert len(lines) == N_FRAMES
        assert all(d["objects"][0]["id"] == 1 and d["objects"][0]["color"]["label"] == "light" for d in lines)
        assert {o.get("id", 0) for d in lines for o in d["objects"]} == {0, 1, 2, 3}
    finally:
        ps.PipelineServer.stop()


# ---- GPU: the fused detect -> track -> classify chain of server option "device_rois" ------------------------------------

GW, GH, G_FRAMES = 352, 198, 24


def drifting_boxes(rng):
    """Per frame: [label, conf, x0, y0, x1, y1] rows of objects that drift a few pixels per frame, appear and vanish;
    label 1 is ``car`` (the classified class), 2 is ``person``. Every box lies inside the frame."""
    objs, frames_ = [], []
    for f in range(G_FRAMES):
        objs = [o for o in objs if rng.random() > 0.08]
        while len(objs) < 7 and (f == 0 or rng.random() < 0.5):
            w, h = int(rng.integers(20, 90)), int(rng.integers(20, 80))
            objs.append([int(rng.integers(1, 3)), int(rng.integers(0, GW - w - 40)), int(rng.integers(0, GH - h - 40)), w, h,
                         int(rng.integers(-1, 2)), int(rng.integers(-1, 2))])
        rows = []
        for o in objs:
            o[1] = min(max(o[1] + o[5], 0), GW - o[3])
            o[2] = min(max(o[2] + o[6], 0), GH - o[4])
            if rng.random() > 0.15:  # a missed detection now and then: the track ages and comes back
                rows.append([float(o[0]), 0.9, o[1] / GW, o[2] / GH, (o[1] + o[3]) / GW, (o[2] + o[4]) / GH])
        frames_.append(rows[:10])
    return frames_


def run_tracked(ps, model_dir, frames_, boxes, options, params, detector_on_device=True):
    """(JSON lines, the classifier's input tensors in call order, fused_batches, batches) of the detect -> track ->
    classify template under the device runner."""
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

    ps.PipelineServer.start(dict({"pipeline_dir": TRACK_PIPES, "model_dir": model_dir, "runner": "device", "batch_max": 4},
                                 **options))
    try:
        ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
        ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(classifier, (24, 24), name="cls"))
        qin, qout = queue.Queue(), queue.Queue()
        for f in frames_:
            qin.put({"fourcc": f.fourcc, "width": f.width, "height": f.height, "planes": f.planes})
        qin.put(None)
        p = ps.PipelineServer.pipeline("detect_track_classify", "hip")
        p.start(source={"type": "application", "input": qin},
                destination={"metadata": {"type": "application", "output": qout, "mode": "json"}}, parameters=params)
        st = p.wait(60)
        assert st["state"] == "COMPLETED", st
        lines = []
        while (x := qout.get(timeout=5)) is not None:
            lines.append(json.loads(x))
        hub = ps.PipelineServer.hub(0)
        return lines, cls_in, [dict(e) for e in hub.fused_batches], list(hub.batches)
    finally:
        ps.PipelineServer.stop()


def reference_of_lines(lines, reclassify):
    """track_ref over the boxes the JSON reports: (ids per frame, the due crops [(frame, x, y, w, h)] in order)."""
    trk = R.Tracker(8)
    ids, crops = [], []
    for k, d in enumerate(lines):
        objs = d.get("objects", [])
        a, due = trk.step(k, [(o["x"], o["y"], o["w"], o["h"]) for o in objs],
                          [o["detection"]["label_id"] for o in objs], [1], reclassify)
        ids.append(a)
        crops += [(k, o["x"], o["y"], o["w"], o["h"]) for o, is_due in zip(objs, due) if is_due]
    return ids, crops


@pytest.mark.gpu
def test_fused_tracked_chain_equals_host_path(evam, gpu, O, coracle, model_dir):  # noqa: F811
    import numpy as np

    ps, mdir = evam.pipeline_server, model_dir
    rng = np.random.default_rng(77)
    frames_ = [O.random_frame(rng, O.NV12, GW, GH, pattern="gradient" if k % 3 == 0 else "uniform")
               for k in range(G_FRAMES)]
    boxes = drifting_boxes(rng)
    lut1 = O.np_norm_lut(1, (0.0, 1.0))
    totals = {}
    for reclassify in (1, 4):
        params = {"reclassify-interval": reclassify}
        off_lines, off_in, off_fused, off_batches = run_tracked(ps, mdir, frames_, boxes, {}, params)
        assert len(off_lines) == G_FRAMES and off_fused == []
        ids, crops = reference_of_lines(off_lines, reclassify)
        assert [[o.get("id", 0) for o in d.get("objects", [])] for d in off_lines] == ids
        assert max(max(a, default=0) for a in ids) >= 8 and all(0 not in a for a in ids)
        assert sum(len(t) for t in off_in) == len(crops)      # the host path classifies exactly the due regions
        totals[reclassify] = len(crops)
        for inflight in (1, 3):
            on_lines, on_in, fused, batches = run_tracked(ps, mdir, frames_, boxes,
                                                         {"device_rois": True, "device_rois_cap": 40, "inflight": inflight},
                                                         params)
            what = f"reclassify {reclassify}, inflight {inflight}"
            assert on_lines == off_lines, f"{what}: the JSON lines differ with device_rois on"
            assert len(fused) == G_FRAMES // 4 and all(e["fused"] and e["reason"] is None for e in fused), what
            assert {b[0][0] for b in batches} == {"detect+classify"}, what
            assert sum(e["count"] for e in fused) == len(crops), what
            # every classifier input row below a batch's count is the oracle's crop of a due region, in order
            got = np.concatenate([t[:e["count"]] for t, e in zip(on_in, fused)])
            ref = np.zeros(got.shape, np.float32)
            for i, (k, x, y, w, h) in enumerate(crops):
                coracle.preprocess_item(frames_[k], (x, y, w, h), ref, i, color_rgb=True, lut=lut1)
            bad = [i for i in range(len(crops)) if not np.array_equal(got[i].view(np.uint32), ref[i].view(np.uint32))]
            assert not bad, f"{what}: classifier rows differ: {[(i, crops[i]) for i in bad[:5]]}"
            if inflight == 3:  # ticks overlap: some batch was launched before the one before it completed
                assert any(b["launched"] < a["completed"] for a, b in zip(fused, fused[1:])), fused
        # a cap below a tick's due count: the regions beyond it take the host path, the JSON is equal
        over_lines, _, over, _ = run_tracked(ps, mdir, frames_, boxes, {"device_rois": True, "device_rois_cap": 2}, params)
        assert over_lines == off_lines and any(e["count"] > 2 for e in over) and all(e["fused"] for e in over)
    assert 0 < totals[4] < totals[1]
    # a detector that answers on the CPU: the stream is tracked on the host from its first tick, recorded as such
    cpu_lines, _, cpu, _ = run_tracked(ps, mdir, frames_, boxes, {"device_rois": True}, {"reclassify-interval": 4},
                                       detector_on_device=False)
    assert cpu_lines == off_lines and cpu and all(not e["fused"] and "device" in e["reason"] for e in cpu)


@pytest.mark.gpu
def test_reclassify_interval_without_tracker_is_fused(evam, gpu, O, model_dir):  # noqa: F811
    """detect -> classify with a reclassify-interval and no gvatrack: every region has id 0, so the interval gates
    nothing and the batch runs fused, as with interval 1."""
    import numpy as np

    ps, mdir = evam.pipeline_server, model_dir
    rng = np.random.default_rng(5)
    frames_ = [O.random_frame(rng, O.NV12, GW, GH, pattern="uniform") for _ in range(8)]
    boxes = drifting_boxes(rng)[:8]

    def run(options):
        seen = [0]

        def detector(t):
            out = torch.full((t.shape[0], 10, 7), -1.0)
            for i in range(t.shape[0]):
                for j, r in enumerate(boxes[seen[0] + i]):
                    out[i, j] = torch.tensor([0.0] + r)
            seen[0] += t.shape[0]
            return out.to(t.device)

        ps.PipelineServer.start(dict({"pipeline_dir": PIPES, "model_dir": mdir, "runner": "device", "batch_max": 4},
                                     **options))
        try:
            ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
            ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(
                lambda t: {"color": torch.stack([1 - t[:, 0, 3, 5], t[:, 0, 3, 5]], 1)}, (24, 24), name="cls"))
            qout = queue.Queue()
            p = ps.PipelineServer.pipeline("detect_classify", "hip")
            p.start(source={"type": "frames", "frames": [
                        {"fourcc": f.fourcc, "width": f.width, "height": f.height, "planes": f.planes} for f in frames_]},
                    destination={"metadata": {"type": "application", "output": qout, "mode": "json"}},
                    parameters={"classification-properties": {"reclassify-interval": 5}})
            assert p.wait(60)["state"] == "COMPLETED"
            lines = []
            while (x := qout.get(timeout=5)) is not None:
                lines.append(x)
            return lines, [dict(e) for e in ps.PipelineServer.hub(0).fused_batches]
        finally:
            ps.PipelineServer.stop()

    off, none = run({})
    on, fused = run({"device_rois": True, "device_rois_cap": 40})
    assert on == off and none == [] and len(fused) == 2 and all(e["fused"] for e in fused)


# Boxes that every frame of every stream gets (label, conf, x0, y0, x1, y1): the detector below cannot tell whose frame
# it sees, and does not have to. Two cars and a person that stand still: each keeps its id, and the classifier's
# result depends on the frame's pixels only.
STILL = [[1.0, 0.9, 0.10, 0.10, 0.40, 0.50], [2.0, 0.9, 0.50, 0.20, 0.80, 0.70], [1.0, 0.9, 0.30, 0.55, 0.60, 0.95]]


def run_streams(ps, model_dir, streams, options):
    """``streams``: [(frames, request parameters)] on one server, device runner, fed frame by frame in turn so that
    their ticks coincide. Returns (JSON lines per stream, fused_batches, batches)."""
    def detector(t):
        out = torch.full((t.shape[0], 10, 7), -1.0)
        for j, r in enumerate(STILL):
            out[:, j] = torch.tensor([0.0] + r)
        return out.to(t.device)

    def classifier(t):
        m = t[:, 0, 3, 5] * 0.5 + t[:, 2, 20, 11] * 0.25  # element-wise: a row's result does not depend on the batch
        return {"color": torch.stack([1 - m, m], 1)}

    ps.PipelineServer.start(dict({"pipeline_dir": TRACK_PIPES, "model_dir": model_dir, "runner": "device"}, **options))
    try:
        ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
        ps.PipelineServer.register_model("cls_alias/cls_ver", ps.InferenceModel(classifier, (24, 24), name="cls"))
        qs, pipes = [], []
        for _, params in streams:
            qin, qout = queue.Queue(), queue.Queue()
            p = ps.PipelineServer.pipeline("detect_track_classify", "hip")
            p.start(source={"type": "application", "input": qin},
                    destination={"metadata": {"type": "application", "output": qout, "mode": "json"}}, parameters=params)
            qs.append((qin, qout))
            pipes.append(p)
        for k in range(max(len(fr) for fr, _ in streams)):
            for (fr, _), (qin, _) in zip(streams, qs):
                if k < len(fr):
                    f = fr[k]
                    qin.put({"fourcc": f.fourcc, "width": f.width, "height": f.height, "planes": f.planes})
        for qin, _ in qs:
            qin.put(None)
        out = []
        for p, (_, qout) in zip(pipes, qs):
            st = p.wait(60)
            assert st["state"] == "COMPLETED", st
            lines = []
            while (x := qout.get(timeout=5)) is not None:
                lines.append(json.loads(x))
            out.append(lines)
        hub = ps.PipelineServer.hub(0)
        return out, [dict(e) for e in hub.fused_batches], list(hub.batches)
    finally:
        ps.PipelineServer.stop()


@pytest.mark.gpu
def test_streams_with_different_reclassify_intervals_on_one_server(evam, gpu, O, model_dir):  # noqa: F811
    """``reclassify-interval`` is a request parameter: streams of one template with intervals 1, 4 and 4 share a
    server. A fused batch's device gate runs with one interval, so only streams of one interval share a batch."""
    import numpy as np

    ps = evam.pipeline_server
    rng = np.random.default_rng(3)
    streams = [([O.random_frame(rng, O.NV12, GW, GH, pattern="uniform") for _ in range(16)],
                {"reclassify-interval": iv}) for iv in (1, 4, 4)]
    opts = {"batch_max": 12, "batch_target": 3, "batch_wait_ms": 100.0}
    off, none, _ = run_streams(ps, model_dir, streams, opts)
    on, fused, batches = run_streams(ps, model_dir, streams, dict(opts, device_rois=True, device_rois_cap=40))
    assert none == [] and fused and all(e["fused"] and e["reason"] is None for e in fused)
    for s, (a, b) in enumerate(zip(off, on)):
        assert len(a) == 16 and a == b, f"stream {s}: the JSON lines differ with device_rois on"
        assert all([o.get("id") for o in d["objects"]] == [1, 2, 3] for d in a), s
    keys = {b[0] for b in batches}
    assert all(k[0] == "detect+classify" for k in keys)
    assert {k[-1] for k in keys} == {1, 4}, "one batch key per reclassify-interval"
    assert any(b[2] == 2 for b in batches if b[0][-1] == 4), "the two interval-4 streams never shared a batch"
    assert all(b[2] == 1 for b in batches if b[0][-1] == 1)
    # what the device gate let through: both cars on every frame at interval 1, on every fourth at interval 4
    assert sum(e["count"] for e in fused) == 2 * 16 + 2 * (2 * 4)


@pytest.mark.gpu
def test_device_tracked_stream_with_detector_interval(evam, gpu, O, model_dir):  # noqa: F811
    """A device-tracked stream whose detector runs on every second frame, one frame per tick: the ticks that hold
    only a skipped frame are no step for the tracker and must pass."""
    import numpy as np

    ps = evam.pipeline_server
    rng = np.random.default_rng(4)
    params = {"detection-properties": {"inference-interval": 2}, "reclassify-interval": 3}
    streams = [([O.random_frame(rng, O.NV12, GW, GH, pattern="uniform") for _ in range(13)], params)]
    off, none, _ = run_streams(ps, model_dir, streams, {"batch_max": 1})
    on, fused, _ = run_streams(ps, model_dir, streams, {"batch_max": 1, "device_rois": True, "device_rois_cap": 8})
    assert none == [] and on == off
    assert len(fused) == 7 and all(e["fused"] for e in fused)          # frames 0, 2, .. 12, one per tick
    assert [e["count"] for e in fused] == [2, 0, 2, 0, 2, 0, 2]        # frames 0, 4, 8, 12: 3 or more frames apart
    for f, d in enumerate(off[0]):
        assert ("objects" in d) == (f % 2 == 0)
        if f % 2 == 0:
            assert [o.get("id") for o in d["objects"]] == [1, 2, 3]
