"""GPU JPEG decoding of source frames, byte for byte.

The references are the fixtures' stored Pillow (libjpeg-turbo) pixels and ``evam_pp_decode_jpeg_host``, the host twin
that shares the kernels' arithmetic and that tests/test_jpeg_dec_host.py pins to Pillow. Nothing here imports Pillow.
The sub-sequence and chunk sizes the edge cases are built around are read from the kernel source."""
import queue

import numpy as np
import pytest

import jpeg_dec_cases as C
import jpeg_ref
from jpeg_content import content
from test_pipeline_server import PIPES, make_model_tree

pytestmark = pytest.mark.gpu

S_BITS = C.source_constant("kJdecSubBits")
T_SUBS = C.source_constant("kJdecChunk")


@pytest.fixture(scope="module")
def pp(evam, gpu):
    h = evam.HipPreProcessor(device=0)
    yield h
    h.close()


def host(evam, files, fourcc=None):
    """The host twin's [n, H, W, bpp] pixels and statuses."""
    N = evam.native
    fourcc = N.FOURCC_BGRX if fourcc is None else fourcc
    buf, pitch, status = N.decode_jpeg_host(files, fourcc)
    i = N.jpeg_info_struct(files[0])
    bpp = 3 if fourcc == N.FOURCC_BGR else 4
    return buf[:, :, :i.width * bpp].reshape(len(files), i.height, i.width, bpp), status


def device_decode(evam, gpu, pp, files, fourcc, pad=0, guard=0, seed=0):
    """Decode into images whose rows are padded by ``pad`` bytes and that lie ``guard`` rows apart inside one noise
    surface. Returns ([n, H, W, bpp] pixels, statuses, True when every byte outside the pixels kept its noise)."""
    import torch

    N = evam.native
    i = N.jpeg_info_struct(files[0])
    bpp = 3 if fourcc == N.FOURCC_BGR else 4
    n, row = len(files), i.width * bpp
    pitch = (row + 15) // 16 * 16 + pad
    rows = i.height + guard
    noise = np.random.default_rng(seed).integers(0, 256, (guard + n * rows, pitch), dtype=np.uint8)
    surf = torch.from_numpy(noise).to(gpu)
    imgs = [evam.Image(fourcc, i.width, i.height, [surf[guard + k * rows:guard + k * rows + i.height]]) for k in range(n)]
    status = torch.full((n,), 77, dtype=torch.int32, device=gpu)
    pp.decode_jpeg_into(files, imgs, status)
    torch.cuda.synchronize()
    got = surf.cpu().numpy()
    px = np.stack([got[guard + k * rows:guard + k * rows + i.height, :row].reshape(i.height, i.width, bpp)
                   for k in range(n)])
    mask = np.ones_like(noise, bool)
    for k in range(n):
        mask[guard + k * rows:guard + k * rows + i.height, :row] = False
    return px, status.cpu().numpy(), bool((got[mask] == noise[mask]).all())


def assert_equal(px, ref, what):
    assert px.shape == ref.shape, what
    bad = np.argwhere(px != ref)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first {bad[:3].tolist()}"


def check_twin(evam, gpu, pp, files, what, fourcc=None):
    N = evam.native
    fourcc = N.FOURCC_BGRX if fourcc is None else fourcc
    ref, ref_status = host(evam, files, fourcc)
    px, status, intact = device_decode(evam, gpu, pp, files, fourcc, pad=16, guard=1)
    assert status.tolist() == ref_status.tolist() == [0] * len(files), what
    assert_equal(px, ref, what)
    assert intact, what


@pytest.mark.parametrize("fmt", ["BGR", "BGRX"])
def test_fixtures_equal_pillow(evam, gpu, pp, fmt):
    """Every fixture, at pitches padded by 0, 16 and 48 bytes: the padding's noise survives, X is 255."""
    N = evam.native
    fourcc = N.FOURCC_BGR if fmt == "BGR" else N.FOURCC_BGRX
    for k, (name, (f, ref)) in enumerate(C.fixtures().items()):
        px, status, intact = device_decode(evam, gpu, pp, [f], fourcc, pad=(0, 16, 48)[k % 3], guard=2, seed=k)
        assert status.tolist() == [0], name
        assert_equal(px[0][..., :3], ref, name)
        if fmt == "BGRX":
            assert (px[..., 3] == 255).all(), name
        assert intact, name
    assert pp.stats().kernels == N.KERNEL_JPEG_DEC


def test_encoder_fixtures_equal_pillow(evam, gpu, pp):
    for name, (f, ref) in C.encoder_fixtures().items():
        px, status, intact = device_decode(evam, gpu, pp, [f], evam.native.FOURCC_BGR, pad=16, guard=1)
        assert status.tolist() == [0] and intact, name
        assert_equal(px[0], ref, name)


def scan_bits(f, stats):
    """Bits of the un-stuffed scan of a jpeg_ref.encode file."""
    s, e = C.scan_bounds(f)
    return (e - s - stats["stuffed"]) * 8


def test_one_pixel(evam, gpu, pp):
    """A scan shorter than one sub-sequence."""
    f, stats = jpeg_ref.encode(content("noise", 1, 1, 3), 90)
    assert scan_bits(f, stats) < S_BITS
    check_twin(evam, gpu, pp, [f], "1x1")


def test_chunk_borders(evam, gpu, pp):
    """Saturated noise at quality 100, one MCU row, widened one MCU at a time: the three consecutive files whose scans
    lie around S*T bits (the last sub-sequence of the first chunk, the first of the second), and one above 2*S*T
    bits. The content has blocks without EOB, which are the longest a scan holds."""
    border = S_BITS * T_SUBS
    per_mcu = scan_bits(*jpeg_ref.encode(content("sat", 64, 16, 1), 100)) // 4
    files, k = [], max(border // per_mcu - 3, 1)
    while True:
        f, stats = jpeg_ref.encode(content("sat", 16 * k, 16, 1), 100)
        files.append((scan_bits(f, stats), f, stats))
        if len(files) >= 2 and files[-2][0] > border:
            break
        k += 1
        assert k * 16 <= 32768
    near = files[-3:]
    assert near[0][0] <= border < near[1][0] < near[2][0], [b for b, _, _ in near]
    assert all(st["no_eob_blocks"] > 0 for _, _, st in near)
    for bits, f, _ in near:
        check_twin(evam, gpu, pp, [f], f"{bits} bits around S*T = {border}")
    f, stats = jpeg_ref.encode(content("sat", 16 * (2 * k + 4), 16, 2), 100)
    assert scan_bits(f, stats) > 2 * border
    check_twin(evam, gpu, pp, [f, f], "above 2*S*T bits")


@pytest.mark.parametrize("colour,chunks", [(False, 1), (True, 1), (False, 2), (True, 2)])
def test_blocks_longer_than_a_sub_sequence(evam, gpu, pp, colour, chunks):
    """Pixel content cannot give a block of S bits (saturated noise at quality 100 stays near 800), so these files are
    written from coefficients: every block holds 63 symbols of a 16-bit code and is longer than S. Asserted from the
    block ends: some sub-sequence completes no block (a zero in the block prefix sum, a record whose first block is
    its neighbour's), some block has symbols in three sub-sequences (three threads write it), and with two chunks
    both happen behind the chunk border as well. tests/test_jpeg_dec_host.py pins the builder's files to libjpeg."""
    sym = 19  # bits of every AC symbol; a block counts for the sub-sequence in which its last symbol starts
    if chunks == 1:
        w, h = 40, 24
    else:
        per_mcu = (6 if colour else 1) * 63 * sym
        mcus = S_BITS * T_SUBS // per_mcu + 8
        w = (16 if colour else 8) * 16
        h = (16 if colour else 8) * -(-mcus // 16)
    f, ends = C.long_block_file(w, h, colour, seed=chunks)
    starts = np.array([0] + ends[:-1])
    last = np.array(ends) - sym
    assert (np.array(ends) - starts).min() > S_BITS
    owners = np.bincount(last // S_BITS)
    empty = np.flatnonzero(owners == 0)
    three = np.flatnonzero(last // S_BITS - starts // S_BITS >= 2)
    assert empty.size and three.size
    if chunks == 2:
        assert ends[-1] > S_BITS * T_SUBS and empty[-1] >= T_SUBS and starts[three[-1]] > S_BITS * T_SUBS
    else:
        assert ends[-1] < S_BITS * T_SUBS
    check_twin(evam, gpu, pp, [f, f], f"long blocks {w}x{h}")


def test_flat_content(evam, gpu, pp):
    """One colour: the shortest blocks there are, more than a hundred per sub-sequence."""
    f, stats = jpeg_ref.encode(content("const", 640, 368, 0), 75)
    blocks = (640 // 8) * (368 // 8) * 3 // 2
    assert scan_bits(f, stats) // blocks <= 8 and S_BITS // 8 > 100
    check_twin(evam, gpu, pp, [f], "flat")


@pytest.mark.parametrize("h", range(1, 34))
def test_420_residue_grid(evam, gpu, pp, h):
    """W in 1..33 at this height, two files of one size per call."""
    rng = np.random.default_rng(100 + h)
    for w in range(1, 34):
        files = [jpeg_ref.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), q)[0] for q in (50, 95)]
        check_twin(evam, gpu, pp, files, f"{w}x{h}")


def nv12_images(evam, O, gpu, n, w, h, seed):
    rng = np.random.default_rng(seed)
    frames = [O.random_frame(rng, O.NV12, w, h, pitch_align=64, pattern="gradient" if i % 3 == 1 else "uniform")
              for i in range(n)]
    return [evam.Image.from_host(f.fourcc, f.width, f.height, f.planes, device=gpu) for f in frames]


def test_round_trip(evam, O, gpu, pp):
    """encode_jpeg of 3 distinct 320x180 NV12 frames, then decode_jpeg: equal to the host twin on the same files."""
    N = evam.native
    files = pp.encode_jpeg(nv12_images(evam, O, gpu, 3, 320, 180, 7), 90)
    assert len(set(files)) == 3
    imgs = pp.decode_jpeg(files)
    assert pp.stats().kernels & N.KERNEL_JPEG_DEC
    ref, status = host(evam, files)
    assert status.tolist() == [0, 0, 0]
    for i, im in enumerate(imgs):
        assert (im.fourcc, im.width, im.height) == (N.FOURCC_BGRX, 320, 180)
        assert_equal(im.planes[0].cpu().numpy()[:, :320 * 4].reshape(180, 320, 4), ref[i], f"frame {i}")


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)])
def test_large_frames(evam, O, gpu, pp, size):
    """Files of this project's own encoder: several chunks, and offsets that need 32 bits."""
    w, h = size
    files = pp.encode_jpeg(nv12_images(evam, O, gpu, 1, w, h, w), 90)
    assert len(files[0]) * 8 > 4 * S_BITS * T_SUBS
    check_twin(evam, gpu, pp, files, f"{w}x{h}")


def test_mixed_geometries_in_one_call(evam, gpu, pp):
    """decode_jpeg groups by geometry and returns the images in the order given."""
    fx = C.fixtures()
    names = ["w3_420", "noise_64x48_444", "w3_420", "noise_64x48_grey", "rst1_33x17_420", "noise_64x48_444"]
    imgs = pp.decode_jpeg([fx[k][0] for k in names], "BGR")
    for k, im in zip(names, imgs):
        ref = fx[k][1]
        h, w = ref.shape[:2]
        assert_equal(im.planes[0].cpu().numpy()[:, :w * 3].reshape(h, w, 3), ref, k)
    with pytest.raises(evam.PreProcError, match=r"files\[1\]"):
        pp.decode_jpeg([fx["w3_420"][0], C.damaged_scans()[1][1]])


def test_calls_in_flight_on_three_streams(evam, gpu):
    """18 seeded random calls, n in 1..5 files of mixed lengths and one geometry each, on three handles and streams,
    synchronised once at the end."""
    import torch

    N = evam.native
    rng = np.random.default_rng(18)
    fx = C.fixtures()
    pools = [[k for k in fx if k.startswith(p)] for p in ("noise_64x48_420", "rstwrap", "w4_422")]
    pools.append(["big"])
    big = [jpeg_ref.encode(content(kind, 200, 120, 4), q)[0] for kind, q in (("noise", 95), ("grad", 50), ("sat", 100))]
    streams = [torch.cuda.Stream(device=gpu) for _ in range(3)]
    handles = [evam.HipPreProcessor(device=0, stream=s) for s in streams]
    calls = []
    for call in range(18):
        pool = pools[int(rng.integers(len(pools)))]
        n = int(rng.integers(1, 6))
        if pool == ["big"]:
            files = [big[int(rng.integers(3))] for _ in range(n)]
        else:
            files = [fx[pool[int(rng.integers(len(pool)))]][0] for _ in range(n)]
        i = N.jpeg_info_struct(files[0])
        imgs = [evam.Image.alloc("BGRX", i.width, i.height, device=gpu) for _ in range(n)]
        calls.append((files, imgs, torch.full((n,), 77, dtype=torch.int32, device=gpu), i))
    torch.cuda.synchronize()  # the fills above ran on torch's stream
    for call, (files, imgs, status, i) in enumerate(calls):
        handles[call % 3].decode_jpeg_into(files, imgs, status)
    torch.cuda.synchronize()
    for call, (files, imgs, status, i) in enumerate(calls):
        ref, ref_status = host(evam, files)
        assert status.cpu().tolist() == ref_status.tolist() == [0] * len(files), call
        for k, im in enumerate(imgs):
            assert_equal(im.planes[0].cpu().numpy()[:, :i.width * 4].reshape(i.height, i.width, 4), ref[k], (call, k))
    for h in handles:
        h.close()


def test_damaged_scans(evam, gpu, pp):
    """The fixed list of 16 damaged scans (the sanitizer program has passed on the same files): zero / non-zero status
    agrees with the host twin, a guard band of noise around every output image stays intact, and the same handle then
    decodes a good file exactly."""
    N = evam.native
    good, ref = C.fixtures()["noise_64x48_420"]
    for name, f, must_fail in C.damaged_scans():
        _, want = host(evam, [f])
        px, status, intact = device_decode(evam, gpu, pp, [f], N.FOURCC_BGRX, pad=16, guard=4, seed=1)
        assert status[0] in (0, N.ERR_INVALID_ARG), name
        assert (status[0] != 0) == (want[0] != 0), (name, status, want)
        if must_fail:
            assert status[0] != 0, name
        assert intact, name
        px, status, intact = device_decode(evam, gpu, pp, [good], N.FOURCC_BGRX, pad=16, guard=4, seed=2)
        assert status.tolist() == [0] and intact, name
        assert_equal(px[0][..., :3], ref, f"good file after {name}")


# ---- pipeline server ---------------------------------------------------------------------------------------------
@pytest.fixture
def server(evam, tmp_path):
    ps = evam.pipeline_server
    mdir = make_model_tree(str(tmp_path / "models"), {
        "det_alias": {"det_ver": (64, 64, {"json_schema_version": "2.0.0", "input_preproc": [],
                                           "output_postproc": [{"labels": ["bg", "car"]}]})}})
    yield ps, mdir
    ps.PipelineServer.stop()


def run_pipeline(ps, frames, seen):
    import torch

    def detector(t):
        seen.append(t.detach().cpu().numpy().copy())
        out = torch.full((t.shape[0], 1, 7), -1.0)
        out[:, 0] = torch.tensor([0, 1, 0.9, 0.25, 0.25, 0.5, 0.75])
        return out

    ps.PipelineServer.register_model("det_alias/det_ver", ps.InferenceModel(detector, (64, 64), name="det"))
    qout = queue.Queue()
    p = ps.PipelineServer.pipeline("detect", "hip")
    p.start(source={"type": "frames", "frames": frames},
            destination={"metadata": {"type": "application", "output": qout, "mode": "json"}})
    st = p.wait(60)
    lines = []
    while (x := qout.get(timeout=5)) is not None:
        lines.append(x)
    return st, lines


@pytest.mark.parametrize("runner", ["device", "threads"])
def test_pipeline_jpeg_source(evam, gpu, pp, server, runner):
    """A frames source of JPEG bytes (and the {"jpeg": ..} form) through a detect stage gives the tensors and metadata
    of the same frames submitted as decoded BGRX Images; a progressive file ends the pipeline in ERROR with the
    decoder's message."""
    ps, mdir = server
    ps.PipelineServer.start({"pipeline_dir": PIPES, "model_dir": mdir, "runner": runner})
    fx = C.fixtures()
    files = [fx[k][0] for k in ("noise_64x48_420", "grad_64x48_q10_420", "noise_64x48_444", "rstrow_64x48_444")]
    a_seen, b_seen = [], []
    items = [files[0], bytearray(files[1]), {"jpeg": memoryview(files[2]), "timestamp": 2}, files[3]]
    st, a_lines = run_pipeline(ps, items, a_seen)
    assert st["state"] == "COMPLETED", st
    st, b_lines = run_pipeline(ps, pp.decode_jpeg(files), b_seen)
    assert st["state"] == "COMPLETED", st
    assert len(a_lines) == 4 and a_lines == b_lines  # the dict item's timestamp is its frame index
    assert np.array_equal(np.concatenate(a_seen), np.concatenate(b_seen))
    st, lines = run_pipeline(ps, [files[0], C.refused_fixture()], [])
    assert st["state"] == "ERROR" and "progressive" in st["message"], st
