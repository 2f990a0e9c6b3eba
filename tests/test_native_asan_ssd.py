"""The detection-row arithmetic of ``evam_pp_ssd_rois`` under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Builds tests/native/ssd_rois_check.cpp — ``ssd_row_rect`` of csrc/evam_geom.h, the function the host helper and the
kernels share — as a stand-alone program with ``-fsanitize=address,undefined -fno-sanitize-recover=all`` and runs it:
rows, transforms and label lists in exactly-sized allocations, values that include NaN, infinities and labels outside
int32, every accepted rect checked against the host path's rules.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ssd_row_rect_under_asan_ubsan(tmp_path):
    exe = tmp_path / "ssd_rois_check"
    subprocess.run(["g++", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "ssd_rois_check.cpp"), "-o", str(exe), "-lm"], check=True)
    # verify_asan_link_order=0: the environment may preload its own library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout
