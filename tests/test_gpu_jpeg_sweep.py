"""GPU JPEG encoder beyond the fixed sizes of tests/test_gpu_jpeg.py: frames large enough for every pass count of
``evam_jpeg_scan2``, the bit packer's extremes (DC category 11, three ZRL codes in a row, blocks without an EOB), every
edge residue of small frames, every quality, the host paths of ``encode_jpeg`` (mixed overflow, ``_jpeg_need``
turnover, a ``dst_stride`` that cuts the file anywhere) and seeded random calls.

Every expected file is ``jpeg_ref.encode(oracle identity BGR of the frame, quality)[0]`` and every comparison is the
whole file and its length, byte for byte. What a content is chosen for is asserted on the reference's stats first
(tests/test_jpeg_host.py asserts the same without a device)."""
import os
import re

import numpy as np
import pytest

from jpeg_content import CUT_FRAMES, KINDS, content, cut_strides
from test_gpu_jpeg import bgr_frame, check, expected
from test_gpu_parity import fc, upload

pytestmark = pytest.mark.gpu

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "edge-video-analytics-microservice_amd", "csrc", "evam_jpeg_kernels.h")


@pytest.fixture(scope="module")
def pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


def same_file(got, ref, what):
    assert len(got) == len(ref), f"{what}: {len(got)} bytes, reference {len(ref)}"
    if got != ref:
        k = next(j for j in range(len(ref)) if got[j] != ref[j])
        raise AssertionError(f"{what}: first difference at byte {k} of {len(ref)}")


def default_slot(w, h):
    return 1024 + (-(-w // 16) * 16) * (-(-h // 16) * 16)


# ---- bit-packer extremes -----------------------------------------------------------------------------------------
def test_dc_category_11(evam, O, gpu, pp):
    """8x8 blocks alternately black and white at quality 100: DC differences of +-2040, the 11-bit category (the last
    entry of the DC tables, a 20-bit code + value)."""
    f = bgr_frame(O, content("blocks", 48, 32))
    _, st = expected(O, f, 100)
    assert st["max_dc_category"] == 11
    check(evam, O, gpu, pp, [f], 100, "black / white blocks")


def test_three_zrl_and_no_eob(evam, O, gpu, pp):
    """A per-pixel checkerboard of 88 / 168 at quality 10: coefficient 63 is the only AC coefficient of 24 blocks, so
    three ZRL codes precede it and the block ends without an EOB."""
    f = bgr_frame(O, content("lowchecker", 48, 32))
    _, st = expected(O, f, 10)
    assert st["max_zrl_run"] == 3 and st["no_eob_blocks"] == 24
    check(evam, O, gpu, pp, [f], 10, "low-amplitude checkerboard")


def test_two_zrl_quality_0_and_1(evam, O, gpu, pp):
    """The 0 / 255 checkerboard at the coarsest tables (most entries clamp to 255): two ZRL codes in a row, and
    quality 0 counts as quality 1."""
    f = bgr_frame(O, content("checker", 48, 32))
    ref1, st = expected(O, f, 1)
    assert st["max_zrl_run"] == 2
    assert expected(O, f, 0)[0] == ref1
    check(evam, O, gpu, pp, [f], 1, "checkerboard at quality 1")
    check(evam, O, gpu, pp, [f], 0, "checkerboard at quality 0")


def test_saturated_without_eob(evam, O, gpu, pp):
    """Saturated noise at quality 100: 51 of 72 blocks fill all 64 coefficients (no EOB) next to 13 dummy blocks, in
    a file past the default slot."""
    f = bgr_frame(O, content("sat", 50, 34, 3))
    ref, st = expected(O, f, 100)
    assert st["no_eob_blocks"] == 51 and len(ref) == 5573 > default_slot(50, 34)
    check(evam, O, gpu, pp, [f], 100, "saturated noise")


# ---- large frames: the passes of evam_jpeg_scan2 -----------------------------------------------------------------
def scan_groups(w, h):
    """Pack groups of a frame and the groups evam_jpeg_scan2 scans per pass, with the constants of the kernel source."""
    src = open(KERNELS).read()
    group = int(re.search(r"constexpr int kJpegGroup = (\d+);", src).group(1))
    per_pass = int(re.search(r"for \(int base = 0; base < g\.n_grp; base \+= (\d+)\)", src).group(1))
    n_blk = 6 * (-(-w // 16)) * (-(-h // 16))
    return -(-n_blk // group), per_pass


def large_frame(O, fmt, w, h, seed):
    if fmt in ("BGR", "BGRX"):
        return bgr_frame(O, content("grad", w, h), fmt, seed)
    return O.random_frame(np.random.default_rng(seed), fc(O, fmt), w, h, pitch_align=64, pattern="gradient")


@pytest.mark.parametrize("fmt,w,h,more_than,passes", [("BGR", 1184, 1184, 256, 2), ("NV12", 1920, 1080, 256, 2),
                                                      ("I420", 2560, 1440, 512, 3), ("BGRX", 3840, 2160, 1280, 6)],
                         ids=["1184x1184", "1080p", "1440p", "2160p"])
def test_large_frames(evam, O, gpu, pp, fmt, w, h, more_than, passes):
    """The smallest square frame whose last group lands in the second pass (257 groups), 1080p (383, a bottom row of
    dummy Y blocks), 1440p (675, three passes) and 2160p (1,519, six): the carry between passes, the zeroed shared
    words of later passes and evam_jpeg_finish's walk over a long stream."""
    n_grp, per_pass = scan_groups(w, h)
    assert n_grp > more_than and -(-n_grp // per_pass) == passes
    check(evam, O, gpu, pp, [large_frame(O, fmt, w, h, w)], 75, f"{fmt} {w}x{h}")


def test_large_frames_two_in_a_call(evam, O, gpu, pp):
    """Two different 1080p frames in one call: frame 1's gsum, total and stream at multi-pass size."""
    n_grp, per_pass = scan_groups(1920, 1080)
    assert n_grp > 256 and -(-n_grp // per_pass) == 2
    frames = [large_frame(O, "NV12", 1920, 1080, 21), large_frame(O, "NV12", 1920, 1080, 22)]
    assert expected(O, frames[0], 75)[0] != expected(O, frames[1], 75)[0]
    check(evam, O, gpu, pp, frames, 75, "2 x 1080p")


# ---- edge residues -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", range(1, 34))
def test_residues_bgr(evam, O, gpu, pp, w):
    """Every height 1..33 at this width (with the parameter: every W, H mod 16 at 1, 2 and 3 MCUs across and down):
    edge replication, repeated chroma rows, dummy blocks and their inherited DC."""
    for h in range(1, 34):
        check(evam, O, gpu, pp, [bgr_frame(O, content("noise", w, h, w * 64 + h), seed=h)], 90, f"BGR {w}x{h}")


@pytest.mark.parametrize("w", range(2, 35, 2))
@pytest.mark.parametrize("fmt", ["NV12", "I420"])
def test_residues_yuv(evam, O, gpu, pp, fmt, w):
    for h in range(2, 35, 2):
        rng = np.random.default_rng(w * 64 + h)
        check(evam, O, gpu, pp, [O.random_frame(rng, fc(O, fmt), w, h, pitch_align=16 << (h & 2))], 90,
              f"{fmt} {w}x{h}")


@pytest.mark.parametrize("size", [(4096, 16), (16, 4096)])
def test_long_thin_frames(evam, O, gpu, pp, size):
    """256 MCUs across and one down, and the reverse."""
    w, h = size
    check(evam, O, gpu, pp, [bgr_frame(O, content("noise", w, h, 5))], 90, f"BGR {w}x{h}")


def test_size_limit(evam, O, gpu, pp):
    """32,768 is the widest frame: the bound refuses 32,769, and a 32768 x 16 frame is exact. (Were the identity
    export to refuse that width, the encode has to fail with the status of the export itself.)"""
    lib = evam.native.load_library()
    assert lib.evam_pp_jpeg_bound(32768, 16) > 0 and lib.evam_pp_jpeg_bound(16, 32768) > 0
    assert lib.evam_pp_jpeg_bound(32769, 16) == 0 and lib.evam_pp_jpeg_bound(16, 32769) == 0
    f = bgr_frame(O, content("grad", 32768, 16))
    imgs = upload(evam, [f], gpu)
    try:
        pp.export_bgr(imgs)
    except evam.PreProcError as e:
        print(f"identity export of 32768x16 refused with status {e.status}")
        with pytest.raises(evam.PreProcError) as e2:
            pp.encode_jpeg(imgs, 75)
        assert e2.value.status == e.status
        return
    print("identity export of 32768x16 accepted")
    same_file(pp.encode_jpeg(imgs, 75)[0], expected(O, f, 75)[0], "BGR 32768x16")


# ---- quality -----------------------------------------------------------------------------------------------------
def test_quality_sweep(evam, O, gpu):
    """Every quality 0..100 in order on one handle, then shuffled: both branches of the quality scaling, the clamp to
    255, quality 0 as 1, and tables rebuilt when the quality alone changes."""
    frames = [bgr_frame(O, content("noise", 50, 34, 9)), bgr_frame(O, content("grad", 26, 10))]
    refs = [[expected(O, f, q)[0] for q in range(101)] for f in frames]
    imgs = [upload(evam, [f], gpu) for f in frames]
    order = list(range(101)) + [int(q) for q in np.random.default_rng(31).permutation(101)]
    with evam.HipPreProcessor(device=0) as h:
        got = [[h.encode_jpeg(im, q)[0] for im in imgs] for q in order]
    for q, files in zip(order, got):
        for k, name in enumerate(("noise 50x34", "gradient 26x10")):
            same_file(files[k], refs[k][q], f"{name} at quality {q}")
    for k in range(2):
        assert refs[k][0] == refs[k][1] and len(set(refs[k])) == 100


# ---- host paths of encode_jpeg / encode_jpeg_into ----------------------------------------------------------------
def test_mixed_overflow(evam, O, gpu):
    """const, sat, const, sat in one call: only frames 1 and 3 outgrow the default slot and are encoded again."""
    frames = [bgr_frame(O, content(k, 50, 34, 3 + i), seed=i) for i, k in enumerate(("const", "sat", "const", "sat"))]
    refs = [expected(O, f, 100)[0] for f in frames]
    assert [len(r) > default_slot(50, 34) for r in refs] == [False, True, False, True] and refs[1] != refs[3]
    imgs = upload(evam, frames, gpu)
    with evam.HipPreProcessor(device=0) as h:
        for call in range(2):
            got = h.encode_jpeg(imgs, 100)
            assert len(got) == 4
            for i in range(4):
                same_file(got[i], refs[i], f"call {call} frame {i}")


def test_need_turnover(evam, O, gpu):
    """17 sizes that each outgrow the default slot: the 16-entry table of learnt slot sizes is cleared and refilled,
    and the first size is still exact afterwards."""
    sizes = [(34 + 2 * i, 34 + (i % 3)) for i in range(17)]
    frames = [bgr_frame(O, content("sat", w, h, w), seed=w) for w, h in sizes]
    refs = [expected(O, f, 100)[0] for f in frames]
    assert len(set(sizes)) == 17 and all(len(r) > default_slot(w, h) for r, (w, h) in zip(refs, sizes))
    with evam.HipPreProcessor(device=0) as h:
        for k in list(range(17)) + [0]:
            same_file(h.encode_jpeg(upload(evam, [frames[k]], gpu), 100)[0], refs[k], "%dx%d" % sizes[k])
            assert sizes[k] in h._jpeg_need and len(h._jpeg_need) <= 16


@pytest.mark.parametrize("case", range(len(CUT_FRAMES)), ids=[c[0] for c in CUT_FRAMES])
def test_arbitrary_cut(evam, O, gpu, pp, case):
    """dst_stride cuts the file two bytes into the scan, inside the last bytes, at its length and one past it: the
    size is always the true length and nothing is written behind the slot; with room the file is whole. (Inside a slot
    that is too small the contents are unspecified.)"""
    import torch

    kind, w, h, seed, q = CUT_FRAMES[case]
    f = bgr_frame(O, content(kind, w, h, seed))
    ref = expected(O, f, q)[0]
    L, guard = len(ref), 256
    strides = cut_strides(L)
    assert case == 2 or any(ref[s - 1] == 0xFF and ref[s] == 0x00 for s in strides if s < L - 1)  # a stuffed 0xFF
    assert ref[L - 2] == 0xFF  # stride L - 1 ends between EOI's two bytes
    imgs = upload(evam, [f], gpu)
    bufs = [torch.full((s + guard,), 7, dtype=torch.uint8, device=gpu) for s in strides]
    sizes = torch.zeros(len(strides), dtype=torch.int32, device=gpu)
    for k, s in enumerate(strides):
        pp.encode_jpeg_into(imgs, bufs[k][:s].view(1, s), sizes[k:k + 1], q)
    torch.cuda.synchronize()
    assert sizes.cpu().tolist() == [L] * len(strides)
    for s, buf in zip(strides, bufs):
        got = buf.cpu().numpy()
        assert (got[s:] == 7).all(), f"stride {s}: bytes behind the slot were written"
        if s >= L:
            same_file(got[:L].tobytes(), ref, f"stride {s}")
            assert (got[L:] == 7).all(), f"stride {s}: bytes behind the file were written"


# ---- seeded random calls -----------------------------------------------------------------------------------------
def frame_of(O, rng, img, fmt):
    """A HostFrame of any format from an [H, W, 3] image, every pitch padded by a random multiple of 16 bytes of
    noise. 4:2:0 formats take Y from channel 1 and U, V from channels 0 and 2 of every other pixel: the expected file
    comes from the oracle's BGR of the frame, so only the kind of content matters."""
    h, w = img.shape[:2]

    def plane(a):
        rows, cols = a.shape
        p = rng.integers(0, 256, (rows, -(-cols // 16) * 16 + 16 * int(rng.integers(0, 4))), dtype=np.uint8)
        p[:, :cols] = a
        return p

    if fmt in ("BGR", "BGRX"):
        n = 3 if fmt == "BGR" else 4
        px = rng.integers(0, 256, (h, w, n), dtype=np.uint8)
        px[..., :3] = img
        return O.HostFrame(fc(O, fmt), w, h, [plane(px.reshape(h, w * n))])
    y, u, v = img[..., 1], img[::2, ::2, 0], img[::2, ::2, 2]
    if fmt == "NV12":
        return O.HostFrame(O.NV12, w, h, [plane(y), plane(np.stack([u, v], -1).reshape(h // 2, w))])
    return O.HostFrame(O.I420, w, h, [plane(y), plane(u), plane(v)])


def random_jpeg_case(O, rng, max_side=320, max_batch=5):
    """(format, frames of one size, quality, description)."""
    fmt = ("NV12", "I420", "BGR", "BGRX")[int(rng.integers(0, 4))]
    w, h = int(rng.integers(1, max_side + 1)), int(rng.integers(1, max_side + 1))
    if fmt in ("NV12", "I420"):
        w, h = w + (w & 1), h + (h & 1)
    quality = int(rng.choice((0, 1, 49, 50, 51, 100))) if rng.random() < 0.4 else int(rng.integers(0, 101))
    kinds = [KINDS[int(rng.integers(0, len(KINDS)))] for _ in range(int(rng.integers(1, max_batch + 1)))]
    frames = [frame_of(O, rng, content(k, w, h, int(rng.integers(0, 1 << 30))), fmt) for k in kinds]
    return fmt, frames, quality, f"{fmt} {w}x{h} quality {quality} {kinds}"


@pytest.mark.parametrize("pitches", [(16, 32), (48, 16)])
def test_i420_unequal_chroma_pitches(evam, O, gpu, pp, pitches):
    """An I420 frame whose U and V planes have different pitches, at a width that is no multiple of 4 (the interleaved
    identity export then takes the generic kernel): the generic kernel addressed V with U's row offsets. Found by
    test_random_jpeg_calls (seed 4); every other kernel family and every earlier test used equal chroma pitches."""
    w, h = 18, 18
    rng = np.random.default_rng(7)
    planes = [rng.integers(0, 256, (h, 32), dtype=np.uint8)] + \
             [rng.integers(0, 256, (h // 2, p), dtype=np.uint8) for p in pitches]
    f = O.HostFrame(O.I420, w, h, planes)
    imgs = upload(evam, [f], gpu)
    got = pp.export_bgr(imgs)
    assert pp.stats().kernels & evam.native.KERNEL_GENERIC
    assert np.array_equal(got.cpu().numpy()[0], O.np_to_bgr(f, 0, 0, w, h))
    check(evam, O, gpu, pp, [f], 90, f"I420 {w}x{h} chroma pitches {pitches}")


@pytest.fixture(scope="module")
def fuzz_pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVAM_FUZZ_JPEG_CASES", "48"))))
def test_random_jpeg_calls(evam, O, gpu, fuzz_pp, seed):
    """Seeded random encode_jpeg calls on one handle (tables, scratch, the copy guess and the learnt slot sizes carry
    over): format, sizes 1..320 with pitch padding, quality 0..100 with the branch points over-weighted, 1..5 frames
    of noise, saturated noise, gradient, constant, checkerboards, black / white blocks or two kinds side by side."""
    fmt, frames, quality, what = random_jpeg_case(O, np.random.default_rng(120000 + seed))
    files = fuzz_pp.encode_jpeg(upload(evam, frames, gpu), quality)
    assert len(files) == len(frames)
    for i, (f, got) in enumerate(zip(frames, files)):
        same_file(got, expected(O, f, quality)[0], f"seed {seed}: {what} frame {i}")


def test_random_jpeg_in_flight(evam, O, gpu):
    """Three handles on three streams, 18 random calls round-robin (every call its own size and quality) into slots of
    the largest file plus 64 bytes, one synchronisation at the end."""
    import torch

    rng = np.random.default_rng(130000)
    cases = [random_jpeg_case(O, rng, max_side=160, max_batch=2) for _ in range(18)]
    refs = [[expected(O, f, q)[0] for f in frames] for _, frames, q, _ in cases]
    imgs = [upload(evam, frames, gpu) for _, frames, _, _ in cases]
    outs = [torch.zeros((len(r), max(map(len, r)) + 64), dtype=torch.uint8, device=gpu) for r in refs]
    sizes = [torch.zeros(len(r), dtype=torch.int32, device=gpu) for r in refs]
    streams = [torch.cuda.Stream(device=gpu) for _ in range(3)]
    handles = [evam.HipPreProcessor(device=0, stream=s) for s in streams]
    torch.cuda.synchronize()  # uploads and fills ran on the default stream
    try:
        for k, (_, _, q, _) in enumerate(cases):
            handles[k % 3].encode_jpeg_into(imgs[k], outs[k], sizes[k], q)
        torch.cuda.synchronize()
        for k, (_, _, _, what) in enumerate(cases):
            lens = sizes[k].cpu().tolist()
            rows = outs[k].cpu().numpy()
            for i, ref in enumerate(refs[k]):
                assert lens[i] == len(ref), f"call {k}: {what} frame {i}: {lens[i]} bytes, reference {len(ref)}"
                same_file(rows[i, :lens[i]].tobytes(), ref, f"call {k}: {what} frame {i}")
    finally:
        for h in handles:
            h.close()
