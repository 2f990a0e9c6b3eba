"""The JPEG decoder's shared arithmetic under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Builds tests/native/jpeg_dec_check.cpp — the header parse, the sub-sequence decoder driven exactly as the kernels
drive it (same sub-sequence and chunk sizes, rounds to convergence, the slot table, the write pass), the IDCT and the
colour stage of csrc/evam_jpeg_dec.h — as a stand-alone program with ``-fsanitize=address,undefined
-fno-sanitize-recover=all`` and runs it on every fixture, on the fixed list of 16 damaged scans, on one good file of
each kind tests/test_gpu_jpeg_dec_sweep.py decodes and on its five damaged restart files, and on 20,000 seeded random
damaged scans. Every one must end with a status, inside exactly-sized heap buffers, within the round bound, and
equal to the sequential decode. Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

import jpeg_dec_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_jpeg_decoder_under_asan_ubsan(tmp_path):
    exe = tmp_path / "jpeg_dec_check"
    subprocess.run(["g++", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "jpeg_dec_check.cpp"), "-o", str(exe), "-lm"], check=True)
    good = sorted(os.path.join(C.DEC_DIR, f) for f in os.listdir(C.DEC_DIR) if f.endswith(".jpg"))
    good += sorted(os.path.join(C.ENC_DIR, f) for f in os.listdir(C.ENC_DIR) if f.endswith(".jpg"))
    damaged, bad = [], []
    for name, data, must_fail in C.damaged_scans():
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        (bad if must_fail else damaged).append(str(path))
    assert len(damaged) + len(bad) == 16
    # the files of tests/test_gpu_jpeg_dec_sweep.py: one good file of each kind, and its damaged restart files
    sweep = {"residue_422_rst1": C.residue_files("422", 1, 9, [17])[0][1][1],
             "long_blocks_444_rst3": C.long_block_file(40, 24, True, seed=3, sampling="444", restart=3)[0]}
    long_files = {"long_intervals_grey": C.long_interval_file("grey")[0], "wide_422": C.wide_and_tall_files("422")[0][1],
                  "tall_444": C.wide_and_tall_files("444")[1][1]}
    long_files.update({f"cut_pairs_{s}": C.cut_pairs_file(s) for s in C.SAMPLINGS})
    long_files.update({what.replace(" ", "_"): f for what, f, _ in C.many_interval_files()})
    good_only = []
    for files, names in ((sweep, good), (long_files, good_only)):
        for name, data in files.items():
            path = tmp_path / (name + ".jpg")
            path.write_bytes(data)
            names.append(str(path))
    for name, data, must_fail in C.damaged_restart_scans():
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        assert must_fail
        bad.append(str(path))
    assert len(bad) + len(damaged) == 21
    # verify_asan_link_order=0: the environment may preload its own library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), *good, "--good-only", *good_only, "--damaged", *damaged, "--expect-bad", *bad],
                       capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout
    assert "20000 random damaged scans" in r.stdout and "(1 refused)" in r.stdout
