"""The gvatrack rule (csrc/evam_track.h) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Builds tests/native/track_check.cpp as a stand-alone program with ``-fsanitize=address,undefined
-fno-sanitize-recover=all`` and runs it on the random sequences of ``tests/track_ref.py``: the state and every frame's
detection, label, id and due arrays in exactly-sized heap allocations, its ids, due flags and final states compared
with the Python reference. Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_track_rule_under_asan_ubsan(tmp_path):
    exe = tmp_path / "track_check"
    subprocess.run(["g++", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "track_check.cpp"), "-o", str(exe)], check=True)
    seqs = R.random_sequences(7)
    max_lost, classify, reclassify = 2, [0, 2], 3
    lines = [f"{len(seqs)} {max_lost} 0.3 {len(classify)} {' '.join(map(str, classify))} {reclassify}"]
    for frames in seqs:
        lines.append(str(len(frames)))
        for f, (boxes, labels) in enumerate(frames):
            lines.append(f"{f} {len(boxes)}")
            lines += [f"{int(l)} {b[0]} {b[1]} {b[2]} {b[3]}" for b, l in zip(boxes, labels)]
    src, dst = tmp_path / "in.txt", tmp_path / "out.txt"
    src.write_text("\n".join(lines) + "\n")
    # verify_asan_link_order=0: the environment may preload its own library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout
    want, states, ev = R.run_reference(seqs, max_lost, 0.3, classify, reclassify)
    assert ev.ties and ev.exhausted and ev.over_d, vars(ev)
    got = iter(dst.read_text().splitlines())
    for s, frames in enumerate(want):
        for f, (ids, due) in enumerate(frames):
            a, b = next(got).split("|")
            assert [int(v) for v in a.split()] == ids, (s, f)
            assert [bool(int(v)) for v in b.split()] == due, (s, f)
        assert next(got) == f"state {states[s][0]}"
        for t in range(R.T):
            assert tuple(int(v) for v in next(got).split()) == states[s][1][t], (s, t)
