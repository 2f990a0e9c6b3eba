"""The SSD DetectionOutput rule (csrc/evam_detout.h) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Builds tests/native/detout_check.cpp as a stand-alone program with ``-fsanitize=address,undefined
-fno-sanitize-recover=all -ffp-contract=off`` and runs it on every case of ``tests/detout_cases.py``: the heads, the
priors, each image's rows and the counts in exactly-sized heap allocations, its blobs and counts compared bit for bit
with the float32 reference of ``tests/detout_ref.py``. Nothing is loaded into Python.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import detout_cases as DC
import detout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("detout_check") / "detout_check"
    subprocess.run(["g++", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "detout_check.cpp"), "-o", str(path)], check=True)
    return path


def test_rule_under_asan_ubsan(exe, tmp_path):
    cases = DC.all_cases()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            cfg = c["cfg"]
            N = c["loc"].shape[0]
            P = c["loc"].shape[1] // 4
            f.write(struct.pack("6i2f", N, P, cfg["num_classes"], cfg["background_label"], cfg["top_k"],
                                cfg["keep_top_k"], cfg["confidence_threshold"], cfg["nms_threshold"]))
            for k in ("loc", "conf", "priors"):
                f.write(np.ascontiguousarray(c[k], np.float32).tobytes())
    # verify_asan_link_order=0: the environment may preload its own library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert f"detout_check: {len(cases)} cases" in r.stdout and "all checks passed" in r.stdout
    raw = dst.read_bytes()
    off = 0
    for c in cases:
        want, wcounts = R.detection_output_bits(c["loc"], c["conf"], c["priors"], c["cfg"])
        nb = want.nbytes
        assert raw[off:off + nb] == want.tobytes(), c["name"]
        off += nb
        assert np.frombuffer(raw, np.uint32, len(wcounts), off).tolist() == wcounts.tolist(), c["name"]
        off += 4 * len(wcounts)
    (m,) = struct.unpack_from("i", raw, off)
    pairs = np.frombuffer(raw, np.float32, 2 * m, off + 4).reshape(m, 2)
    assert off + 4 + 8 * m == len(raw) and m >= 10
    assert pairs[:, 1].tobytes() == R.expf_bits(pairs[:, 0]).tobytes()
