"""bench.py's command line: a plain run is lean (set-up, warm-up, the timed steps, the line), `--full` adds the
secondary measurements, `--dump-outputs DIR` writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "latency", "host_us_per_call")


def test_dump_output_whole_and_sampled(tmp_path, monkeypatch):
    """A tensor within the limit is written whole as float32 (u8 widened exactly); a larger one as the elements at
    seeded flat indices, the same in every call, drawn from the tensor itself."""
    import torch

    t = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7) * 0.37
    meta = bench.dump_output(torch, t, str(tmp_path / "whole.npy"))
    a = np.load(tmp_path / "whole.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 5, 7) and not meta["sampled"]
    assert np.array_equal(a, t.numpy())
    u = (torch.arange(210) % 251).to(torch.uint8).reshape(2, 105)
    bench.dump_output(torch, u, str(tmp_path / "u8.npy"))
    b = np.load(tmp_path / "u8.npy")
    assert b.dtype == np.float32 and np.array_equal(b, u.numpy().astype(np.float32))

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 100)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ELEMS", 64)
    for name in ("s1.npy", "s2.npy"):
        meta = bench.dump_output(torch, t, str(tmp_path / name))
    s1, s2 = np.load(tmp_path / "s1.npy"), np.load(tmp_path / "s2.npy")
    assert meta["sampled"] and meta["of_shape"] == [2, 3, 5, 7]
    assert s1.dtype == np.float32 and s1.shape == (64,) and np.array_equal(s1, s2)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, t.numel(), size=64, dtype=np.int64))
    assert np.array_equal(s1, t.numpy().reshape(-1)[idx])
    assert s1.nbytes <= 4 * 100


def test_dump_sample_fits_the_limit():
    assert bench.DUMP_SAMPLE_ELEMS * 4 <= bench.DUMP_LIMIT_BYTES <= 64 * 10**6


def test_bench_help_names_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(evam, gpu, tmp_path):
    """A plain `bench.py --config c1_b1 --steps 4 --warmup 1 --dump-outputs DIR`: the line has the headline fields and
    none of the --full blocks, and DIR/output.npy is, bit for bit, what the library computes from the frame set of
    step 3 (pool set 3 of 64: bench's seed 1234 + 7919 * 3)."""
    import torch

    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "EVAM_BENCH_PG")}
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1_b1", "--steps", "4",
                        "--warmup", "1", "--dump-outputs", str(d)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 4 and res["warmup"] == 1 and res["unit"] == "frames/s" and res["higher_is_better"] is True
    assert res["value"] > 0 and res["ms_per_step"] > 0 and res["dtype"] == "u8"
    # one frame per step: value and ms_per_step are the same wall clock (ms_per_step is rounded to 1e-4 ms, 1 % of
    # a 10 us step, which is less than four launches and a synchronize take)
    assert res["value"] == pytest.approx(1e3 / res["ms_per_step"], rel=2e-2)
    assert not any(k in res for k in FULL_ONLY) and res["cpu_baseline"] is None
    assert res["config"]["pool_sets"] == 64
    assert os.listdir(d) == ["output.npy"] and res["outputs"]["file"] == "output.npy" and not res["outputs"]["sampled"]
    got = np.load(d / "output.npy")
    assert got.dtype == np.float32 and got.shape == (1, 3, 512, 512)

    wl = bench.WORKLOADS["c1_b1"]
    imgs = bench.device_frames(evam, torch, wl, 1, gpu, seed=1234 + 7919 * 3)
    out = torch.full((1, 3, 512, 512), 7, dtype=torch.uint8, device=gpu)
    pp = evam.HipPreProcessor(device=0)
    pp.convert(evam.ImageBatch(imgs), out, bench.make_info(evam, wl))
    torch.cuda.synchronize()
    pp.close()
    assert np.array_equal(got, out.cpu().numpy().astype(np.float32))
