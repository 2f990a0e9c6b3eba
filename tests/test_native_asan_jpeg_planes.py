"""The raw-plane output of the JPEG decoder under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Builds tests/native/jpeg_planes_check.cpp — jdec_planes_host, jdec_planes_row and jdec_store_clipped of
csrc/evam_jpeg_dec.h, the row tasks and the clipped stores the kernel shares — as a stand-alone program with
``-fsanitize=address,undefined -fno-sanitize-recover=all`` and runs it on every plane fixture (the sizes 2x2, 10x10 and
24x8 among them), on the damaged scans that are even-sized 4:2:0 files and on 5,000 seeded random damaged scans. The
output planes are exactly-sized heap blocks whose last row ends with its pixels, so a store behind a row's pixels or
below the last row is a heap overflow. Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

import jpeg_dec_cases as C
import jpeg_planes_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_jpeg_planes_under_asan_ubsan(tmp_path):
    exe = tmp_path / "jpeg_planes_check"
    subprocess.run(["g++", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "jpeg_planes_check.cpp"), "-o", str(exe), "-lm"], check=True)
    good = sorted(os.path.join(PC.PLANES_DIR, f) for f in os.listdir(PC.PLANES_DIR) if f.endswith(".jpg"))
    good += [os.path.join(d, f) for d in (C.DEC_DIR, C.ENC_DIR) for f in sorted(os.listdir(d))
             if f.endswith(".jpg") and PC.header_420_even(open(os.path.join(d, f), "rb").read())]
    assert len(good) == len(PC.fixtures()) == 44
    damaged = []
    for name, data, _ in C.damaged_scans():
        if PC.header_420_even(data):
            path = tmp_path / (name + ".jpg")
            path.write_bytes(data)
            damaged.append(str(path))
    assert len(damaged) >= 10
    # verify_asan_link_order=0: the environment may preload its own library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), *good, "--damaged", *damaged], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout
    assert f"{len(good) + len(damaged)} files (0 skipped), 5000 random damaged scans" in r.stdout
