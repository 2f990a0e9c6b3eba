"""GPU JPEG decoding beyond 4:2:0 without restart intervals: every sampling at every size residue, restart intervals
at sizes where the carries of evam_jdec_unstuff, the slot arithmetic of evam_jdec_sync / evam_jdec_write and the
interval sums of evam_jdec_dc matter, frames wider than one workgroup of evam_jdec_colour, seeded random calls, and
damaged restart files.

Every file is written at test time by tests/jpeg_ref.py (pinned to Pillow's files byte for byte in
tests/test_jpeg_host.py) or by ``jpeg_dec_cases.long_block_file``. The reference is the host twin, which
tests/test_jpeg_dec_host.py and tests/test_jpeg_planes_host.py pin to Pillow on these very files. Every precondition
is asserted on the file's bytes before the GPU is touched, and every kernel constant is read from the source. Nothing
here imports Pillow."""
import os

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_planes_cases as PC
import jpeg_ref
from jpeg_content import KINDS, content
from test_gpu_jpeg_dec import assert_equal, check_twin, device_decode, host
from test_gpu_jpeg_planes import check_twin as check_planes_twin, host_planes

pytestmark = pytest.mark.gpu

S_BITS = C.source_constant("kJdecSubBits")
SUB_BYTES = S_BITS // 8
T_SUBS = C.source_constant("kJdecChunk")
DC_THREADS = C.source_constant("kJdecDcThreads", "evam_jpeg_dec_kernels.h")
PASS = C.PASS
CHUNK_BYTES = S_BITS * T_SUBS // 8


@pytest.fixture(scope="module")
def pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


def fourcc_of(evam, k):
    return evam.native.FOURCC_BGR if k % 2 == 0 else evam.native.FOURCC_BGRX


# ---- residue grids ------------------------------------------------------------------------------------------------

def residue_row(evam, gpu, pp, sampling, restart, h):
    widths, heights = C.RESIDUE_GRIDS[sampling]
    assert h in heights
    rows = C.residue_files(sampling, restart, h, widths)
    for w, files in rows:
        for f in files:
            i = evam.jpeg_info(f)
            assert (i.width, i.height, i.restart_interval) == (w, h, restart)
            mr, mc, _ = jpeg_ref.mcu_grid(w, h, sampling)
            assert len(C.rst_markers(f)) == (-(-mr * mc // restart) - 1 if restart else 0)
    for w, files in rows:
        check_twin(evam, gpu, pp, files, f"{sampling} restart {restart} {w}x{h}", fourcc_of(evam, w + h))


@pytest.mark.parametrize("restart", [0, 1])
@pytest.mark.parametrize("h", range(1, 18))
def test_444_residue_grid(evam, gpu, pp, h, restart):
    """W in 1..17 at this height, two files of one size per call: jdec_block_pos of the 8x8 MCU at every residue, no
    up-sampling. With ``restart`` 1 every MCU is an interval; the 1x1 file has a DRI and no marker."""
    residue_row(evam, gpu, pp, "444", restart, h)


@pytest.mark.parametrize("restart", [0, 1])
@pytest.mark.parametrize("h", range(1, 18))
def test_grey_residue_grid(evam, gpu, pp, h, restart):
    residue_row(evam, gpu, pp, "grey", restart, h)


@pytest.mark.parametrize("restart", [0, 1])
@pytest.mark.parametrize("h", range(1, 18))
def test_422_residue_grid(evam, gpu, pp, h, restart):
    """W in 1..33: h2v1_fancy_upsample at every width residue of the 16x8 MCU, and at W <= 4 the replication rule of
    a down-sampled width of 1 or 2."""
    residue_row(evam, gpu, pp, "422", restart, h)


@pytest.mark.parametrize("h", range(1, 34))
def test_420_residue_grid_with_restarts(evam, gpu, pp, h):
    """test_420_residue_grid's sizes with a marker behind every MCU."""
    residue_row(evam, gpu, pp, "420", 1, h)


# ---- unstuff carries and cut pairs --------------------------------------------------------------------------------

def test_cut_pairs_preconditions():
    """What the four cut-pairs files have, from their raw scans alone. Asserted of each: longer than two passes, a
    marker wholly in the third pass, markers cycling RST0..7, and the literal properties of CUT_SEEDS. Asserted of
    the four together (no seed below 200 gives one file all of it, see CUT_SEEDS): markers at all 16 residues mod
    kJdecUnstuffBytes, a marker and an FF 00 pair whose FF is the last byte of a pass, RST7 passed twice."""
    union = {"residues": set(), "marker_cut": 0, "pair_cut": 0, "wraps": 0}
    for sampling in C.SAMPLINGS:
        f = C.cut_pairs_file(sampling)
        p = C.cut_pairs_properties(f)
        seed, residues, marker_cut, pair_cut, wraps = C.CUT_SEEDS[sampling]
        assert p["len"] > 2 * PASS + 1 and p["third_pass"] and p["in_sequence"], (sampling, p)
        assert (p["residues"], p["marker_cut"], p["pair_cut"], p["wraps"]) == (residues, marker_cut, pair_cut, wraps)
        union["residues"] |= {k % C.UNSTUFF_BYTES for k, _ in C.rst_markers(f)}
        union["marker_cut"] += len(marker_cut)
        union["pair_cut"] += len(pair_cut)
        union["wraps"] = max(union["wraps"], wraps)
    assert len(union["residues"]) == C.UNSTUFF_BYTES == 16
    assert union["marker_cut"] >= 1 and union["pair_cut"] >= 1 and union["wraps"] >= 2
    p = C.cut_pairs_properties(C.cut_pairs_file("grey"))
    assert p["residues"] == 16 and p["wraps"] >= 2  # one file alone has these two


@pytest.mark.parametrize("sampling", C.SAMPLINGS)
def test_cut_pairs(evam, gpu, pp, sampling):
    """Saturated noise at quality 100 with a marker behind every MCU, three passes of evam_jdec_unstuff: the carries
    ``kept`` / ``rst`` across passes, first[] written in later passes, pairs cut by a thread's window and by a pass
    border. Alone, then with a short file of the same geometry (one pass) in between: one call, two pass counts."""
    f = C.cut_pairs_file(sampling)
    p = C.cut_pairs_properties(f)
    assert p["len"] > 2 * PASS + 1 and p["third_pass"] and (p["marker_cut"] or p["pair_cut"])
    w, mh = C.cut_pairs_width(sampling), C.mcu_size(sampling)[1]
    short = jpeg_ref.encode(content("const", w, mh), 100, sampling=sampling, restart=1)[0]
    s, e = C.scan_bounds(short)
    assert e - s < PASS and len(C.rst_markers(short)) == len(C.rst_markers(f))
    table = C.interval_table(f)
    assert any(a % SUB_BYTES for a in table[1:-1])  # slot0 = fb / kJdecSubBytes + k with fb off a boundary, k > 0
    check_twin(evam, gpu, pp, [f], f"cut pairs {sampling}", fourcc_of(evam, 1))
    check_twin(evam, gpu, pp, [f, short, f], f"cut pairs {sampling} with a short file", fourcc_of(evam, 0))
    if sampling == "420":
        for fmt in ("NV12", "I420"):
            check_planes_twin(evam, gpu, pp, [short, f], fmt, ["unequal", "window"], "cut pairs")


# ---- intervals longer than a chunk --------------------------------------------------------------------------------

def long_interval_case(sampling):
    f, restart, mcus = C.long_interval_file(sampling)
    table = C.interval_table(f)
    assert len(table) == 4 and len(C.rst_markers(f)) == 2
    sizes = np.diff(table)
    assert sizes[0] * 8 > S_BITS * T_SUBS and sizes[1] * 8 > S_BITS * T_SUBS and sizes[2] < min(sizes[:2])
    assert table[1] % SUB_BYTES != 0  # interval 1 starts off a sub-sequence boundary: blk0 != 0 and k > 0 there
    assert restart > DC_THREADS and restart % DC_THREADS != 0  # evam_jdec_dc: per > 1, the last lanes clipped
    assert 0 < mcus - 2 * restart < restart
    return f


def test_intervals_longer_than_a_chunk(evam, gpu, pp):
    """Grey saturated noise at quality 100, three intervals: 0 and 1 are each longer than S * T bits, so
    evam_jdec_sync's second chunk of interval 1 starts from carry_blk = blk0 + a count, and evam_jdec_dc sums more
    than kJdecDcThreads MCUs per interval, the last interval fewer than the others."""
    f = long_interval_case("grey")
    check_twin(evam, gpu, pp, [f], "long intervals", fourcc_of(evam, 1))
    g = bytes(C.long_interval_file("grey")[0])
    check_twin(evam, gpu, pp, [f, g], "long intervals, two files", fourcc_of(evam, 0))


@pytest.mark.parametrize("fmt", ["NV12", "I420"])
def test_intervals_longer_than_a_chunk_to_planes(evam, gpu, pp, fmt):
    f = long_interval_case("420")
    assert evam.jpeg_planes_ok(evam.jpeg_info(f))
    for kind in ("unequal", "window"):
        check_planes_twin(evam, gpu, pp, [f], fmt, [kind], "long intervals")


# ---- many intervals -----------------------------------------------------------------------------------------------

def test_many_intervals(evam, gpu, pp):
    """2,048 intervals of a few bytes each, and 293 of seven MCUs that do not divide the row of 64; BGRX. Then 256
    intervals of a 4:2:0 frame into NV12."""
    (w1, f1, _), (w7, f7, _), (w420, f420, _) = C.many_interval_files()
    t1, t7 = C.interval_table(f1), C.interval_table(f7)
    assert len(t1) == 2048 + 1 and len(t7) == -(-2048 // 7) + 1 and 64 % 7
    assert np.diff(t1).max() < 16 and np.diff(t1).min() >= 1
    assert len(C.interval_table(f420)) == 256 + 1
    check_twin(evam, gpu, pp, [f1], w1)
    check_twin(evam, gpu, pp, [f7], w7)
    check_planes_twin(evam, gpu, pp, [f420], "NV12", ["base16"], w420)


# ---- long blocks across a restart ---------------------------------------------------------------------------------

@pytest.mark.parametrize("restart", [1, 3])
@pytest.mark.parametrize("sampling", ["422", "444"])
def test_long_blocks_across_a_restart(evam, gpu, pp, sampling, restart):
    """test_blocks_longer_than_a_sub_sequence's files at 40x24 with restart intervals. Every block is longer than S,
    and in every interval some sub-sequence completes no block. With three MCUs per interval some block of every
    whole interval has symbols in three sub-sequences; one MCU is too short for that (its blocks start at most
    4 * 186 bits behind a sub-sequence boundary, and 838 are needed), so there it is asserted of no interval."""
    sym = 19
    f, ends = C.long_block_file(40, 24, True, seed=restart, sampling=sampling, restart=restart)
    mr, mc, bpm = jpeg_ref.mcu_grid(40, 24, sampling)
    table = C.interval_table(f)
    assert len(table) == -(-mr * mc // restart) + 1 and len(ends) == mr * mc * bpm
    ends = np.array(ends)
    assert np.diff(np.concatenate([[0], ends])).min() > S_BITS - 8  # the padding of an interval is not the block's
    spans = []
    for k in range(len(table) - 1):
        e = ends[k * restart * bpm:(k + 1) * restart * bpm] - table[k] * 8
        starts = np.concatenate([[0], e[:-1]])
        assert (e - starts).min() > S_BITS and e[-1] <= (table[k + 1] - table[k]) * 8
        last = e - sym
        assert (np.bincount(last // S_BITS) == 0).any(), k
        spans.append(bool((last // S_BITS - starts // S_BITS >= 2).any()))
    whole = (mr * mc) // restart
    assert all(spans[:whole]) if restart == 3 else not any(spans)
    check_twin(evam, gpu, pp, [f, f], f"long blocks {sampling} restart {restart}")


# ---- wide and tall frames -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampling", ["422", "444", "grey"])
def test_wide_and_tall_frames(evam, gpu, pp, sampling):
    """2 * 256 * kVec + 5 pixels wide (blockIdx.x of evam_jdec_colour reaches 2, the last workgroup holds five pixels)
    with a marker behind every MCU row, and 24 x 1,100; a gradient with noise at quality 85."""
    assert C.WIDE == 2 * 256 * C.source_constant("kVec", "evam_jpeg_dec_api.h") + 5
    for k, (what, f) in enumerate(C.wide_and_tall_files(sampling)):
        i = evam.jpeg_info(f)
        assert (i.width, i.height) in ((C.WIDE, 24), (24, 1100))
        if k == 0:
            assert i.restart_interval == -(-C.WIDE // C.mcu_size(sampling)[0]) and len(C.rst_markers(f)) >= 1
            s, e = C.scan_bounds(f)
            assert e - s > 2 * PASS  # a scan of several passes and sub-sequences
        check_twin(evam, gpu, pp, [f], f"{what} {sampling}", fourcc_of(evam, k + len(sampling)))


# ---- seeded random calls ------------------------------------------------------------------------------------------

FUZZ_SIZES = (1, 2, 8, 9, 16, 17)


def random_dec_case(rng):
    """One call: dict(files, out, pad, kinds, what). ``out`` is "BGR", "BGRX", "NV12" or "I420". Every draw is a file
    the decoder accepts."""
    sampling = C.SAMPLINGS[int(rng.choice(4, p=[0.19, 0.27, 0.27, 0.27]))]
    w, h = (int(rng.choice(FUZZ_SIZES)) if rng.random() < 0.3 else int(rng.integers(1, 201)) for _ in range(2))
    quality = int(rng.choice([1, 10, 50, 75, 95, 100]))
    mr, mc, _ = jpeg_ref.mcu_grid(w, h, sampling)
    restart = int([0, 1, 2, mc, int(rng.integers(1, mr * mc + 4))][int(rng.integers(5))])
    n = int(rng.integers(1, 5))
    kinds = [KINDS[int(rng.integers(len(KINDS)))] for _ in range(n)]
    seed = int(rng.integers(1 << 30))
    files = [jpeg_ref.encode(content(k, w, h, seed + i), quality, sampling=sampling, restart=restart)[0]
             for i, k in enumerate(kinds)]
    out = "BGR" if rng.random() < 0.5 else "BGRX"
    pad = int(rng.choice([0, 16, 48]))
    if sampling == "420" and w % 2 == 0 and h % 2 == 0 and rng.random() < 1 / 3:
        out = "NV12" if rng.random() < 0.5 else "I420"
    layout = [PC.KINDS[int(rng.integers(len(PC.KINDS)))] for _ in range(n)]
    return {"files": files, "out": out, "pad": pad, "layout": layout, "sampling": sampling,
            "what": f"{sampling} {w}x{h} q{quality} restart {restart} {kinds} {out} pad {pad}"}


def test_random_draws_cover_every_kind():
    """The draw alone, no GPU: 4:2:0 is at most a quarter of 400 cases, every sampling, output and restart kind
    occurs, and every file parses as what was drawn."""
    cases = [random_dec_case(np.random.default_rng(130000 + seed)) for seed in range(400)]
    share = sum(c["sampling"] == "420" for c in cases)
    assert 0 < share <= 100
    assert {c["sampling"] for c in cases} == set(C.SAMPLINGS)
    assert {c["out"] for c in cases} == {"BGR", "BGRX", "NV12", "I420"}
    assert {c["pad"] for c in cases} == {0, 16, 48} and {len(c["files"]) for c in cases} == {1, 2, 3, 4}


@pytest.fixture(scope="module")
def fuzz_pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVAM_FUZZ_JPEG_DEC_CASES", "48"))))
def test_random_jpeg_dec_calls(evam, gpu, fuzz_pp, seed):
    """Seeded random decode calls on one handle (its scratch and tables carry over): sampling, sizes 1..200 with the
    block and MCU borders over-weighted, quality, restart interval, 1..4 files of any content, BGR / BGRX at a padded
    pitch or, for even 4:2:0 files, NV12 / I420 in a random layout. Every status is 0, every byte the twin's."""
    N = evam.native
    c = random_dec_case(np.random.default_rng(130000 + seed))
    files, what = c["files"], c["what"]
    if c["out"] in ("NV12", "I420"):
        check_planes_twin(evam, gpu, fuzz_pp, files, c["out"], c["layout"], what, seed=seed)
        return
    fourcc = N.FOURCC_BGR if c["out"] == "BGR" else N.FOURCC_BGRX
    ref, ref_status = host(evam, files, fourcc)
    px, status, intact = device_decode(evam, gpu, fuzz_pp, files, fourcc, pad=c["pad"], guard=2, seed=seed)
    assert status.tolist() == ref_status.tolist() == [0] * len(files), what
    assert_equal(px, ref, what)
    assert intact, what


def test_random_calls_in_flight_on_three_streams(evam, gpu):
    """18 of the same draws on three handles and streams, synchronised once at the end."""
    import torch

    N = evam.native
    streams = [torch.cuda.Stream(device=gpu) for _ in range(3)]
    handles = [evam.HipPreProcessor(device=0, stream=s) for s in streams]
    calls = []
    for call in range(18):
        c = random_dec_case(np.random.default_rng(140000 + call))
        i = N.jpeg_info_struct(c["files"][0])
        n = len(c["files"])
        imgs = [evam.Image.alloc(c["out"], i.width, i.height, device=gpu) for _ in range(n)]
        calls.append((c, imgs, torch.full((n,), 77, dtype=torch.int32, device=gpu), i))
    torch.cuda.synchronize()  # the fills above ran on torch's stream
    for call, (c, imgs, status, i) in enumerate(calls):
        handles[call % 3].decode_jpeg_into(c["files"], imgs, status)
    torch.cuda.synchronize()
    for call, (c, imgs, status, i) in enumerate(calls):
        files, out = c["files"], c["out"]
        if out in ("NV12", "I420"):
            ref, ref_status = host_planes(evam, files, out)
        else:
            ref, ref_status = host(evam, files, N.FOURCC_BGR if out == "BGR" else N.FOURCC_BGRX)
        assert status.cpu().tolist() == ref_status.tolist() == [0] * len(files), c["what"]
        for k, im in enumerate(imgs):
            if out in ("NV12", "I420"):
                for got, want in zip(im.planes, ref[k]):
                    assert np.array_equal(got.cpu().numpy()[:, :want.shape[1]], want), (c["what"], k)
            else:
                bpp = ref.shape[-1]
                got = im.planes[0].cpu().numpy()[:, :i.width * bpp].reshape(i.height, i.width, bpp)
                assert_equal(got, ref[k], (c["what"], k))
    for h in handles:
        h.close()


# ---- damaged restart files ----------------------------------------------------------------------------------------

def test_damaged_restart_scans(evam, gpu, pp):
    """The five damaged restart files (the sanitizer program has passed on the same files, and the host twin ends
    each with a status): truncated inside the second pass, a marker out of sequence there, the marker on a pass
    border removed or turned into FF 00, one marker too many. Zero / non-zero status agrees with the host twin, a
    guard band of noise around the output stays intact, and the same handle then decodes a good restart file
    exactly."""
    N = evam.native
    good = C.cut_pairs_file("grey")
    ref, ref_status = host(evam, [good])
    assert ref_status.tolist() == [0]
    cases = C.damaged_restart_scans()
    assert len(cases) == 5
    for name, f, must_fail in cases:
        _, want = host(evam, [f])
        assert want[0] != 0 and must_fail, name
        px, status, intact = device_decode(evam, gpu, pp, [f], N.FOURCC_BGRX, pad=16, guard=4, seed=1)
        assert status[0] in (0, N.ERR_INVALID_ARG), name
        assert (status[0] != 0) == (want[0] != 0), (name, status, want)
        assert intact, name
        px, status, intact = device_decode(evam, gpu, pp, [good], N.FOURCC_BGRX, pad=16, guard=4, seed=2)
        assert status.tolist() == [0] and intact, name
        assert_equal(px, ref, f"good file after {name}")
