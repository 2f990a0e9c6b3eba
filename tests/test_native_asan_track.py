"""The gvatrack rule (csrc/evam_track.h) under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

Builds tests/native/track_check.cpp as a stand-alone program with ``-fsanitize=address,undefined
-fno-sanitize-recover=all`` and runs it on the inputs of ``tests/track_ref.py`` (the random sequences, the 128-round
chain, one sequence of extreme boxes with frame indices up to 0xFFFFFFFE): the state and every frame's detection,
label, id and due arrays in exactly-sized heap allocations, its ids, due flags and final states compared with the
Python reference. The program steps the first stream a second time with a NULL due pointer and compares, and writes
the key of every pair of a grid of extreme boxes, compared here with ``track_ref.pair_key``. Nothing is loaded into
Python.
"""
import os
import shutil
import subprocess

import pytest

import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-ffp-contract=off"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("track_check") / "track_check"
    subprocess.run(["g++", *SAN, "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "track_check.cpp"), "-o", str(path)], check=True)
    return path


def run_program(exe, tmp_path, seqs, frame_indices, max_lost, iou, classify, reclassify):
    """The program on ``seqs``; its per-frame ids and due flags and final states compared with the reference. Returns
    ``(the reference's Events, the output lines behind the states)``."""
    n_set = -2 if classify is None else -1 if classify == "all" else len(classify)
    lines = [f"{len(seqs)} {max_lost} {iou!r} {n_set} {' '.join(map(str, classify if n_set > 0 else []))} {reclassify}"]
    for s, frames in enumerate(seqs):
        lines.append(str(len(frames)))
        for f, (boxes, labels) in enumerate(frames):
            lines.append(f"{frame_indices[s][f]} {len(boxes)}")
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
    assert f" {len(seqs[0])} steps with a NULL due pointer" in r.stdout
    want, states, ev = R.run_reference(seqs, max_lost, iou, classify, reclassify, frame_indices=frame_indices)
    got = iter(dst.read_text().splitlines())
    for s, frames in enumerate(want):
        for f, (ids, due) in enumerate(frames):
            a, b = next(got).split("|")
            assert [int(v) for v in a.split()] == ids, (s, f)
            assert [bool(int(v)) for v in b.split()] == due, (s, f)
        assert next(got) == f"state {states[s][0]}"
        for t in range(R.T):
            assert tuple(int(v) for v in next(got).split()) == states[s][1][t], (s, t)
    return ev, list(got)


def test_track_rule_under_asan_ubsan(exe, tmp_path):
    seqs = R.random_sequences(7)
    ev, rest = run_program(exe, tmp_path, seqs, [range(len(fr)) for fr in seqs], 2, 0.3, [0, 2], 3)
    assert ev.ties and ev.exhausted and ev.over_d, vars(ev)
    # the keys of the extreme pairs: equal to the reference's, not only in range
    assert len(rest) == len(R.EXTREME_FIELDS) ** 4
    some = 0
    for line in rest:
        tag, *v = line.split()
        v = [int(x) for x in v]
        assert tag == "key" and len(v) == 9
        want = R.pair_key(v[0:4], v[4:8])
        assert v[8] == (-1 if want is None else want), line
        some += want is not None and 0 < want < 65536
    assert some > 100, "hardly a pair of the grid overlaps in part"


def test_chain_under_asan_ubsan(exe, tmp_path):
    frames, ids = R.chain_frames(128, seed=9)
    ev, _ = run_program(exe, tmp_path, [frames], [[3, 4]], 8, 0.3, "all", 2)
    assert ev.rounds >= 128


def test_extreme_sequence_under_asan_ubsan(exe, tmp_path):
    seqs, fi = R.extreme_sequences(21, 2, 30)
    ev, _ = run_program(exe, tmp_path, seqs, fi, 2, 0.0, [-2**31, 0], 2**31 - 1)
    assert ev.ties and ev.exhausted and ev.over_d, vars(ev)
    assert fi[0][-1] == R.LAST_FRAME
