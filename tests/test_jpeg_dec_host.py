"""CPU tests of the JPEG decoder: ``evam_pp_decode_jpeg_host`` (the arithmetic the kernels share, driven sequentially)
against pixels Pillow (libjpeg-turbo) decoded, byte for byte: the stored fixtures always, fresh files where Pillow is
importable. Also the header parse: every refusal with its status, and ``jpeg_info``; and the pipeline server's JPEG
source items with a stand-in decoder."""
import io

import numpy as np
import pytest

import jpeg_content
import jpeg_dec_cases as C
import jpeg_ref


def decode(N, files, fourcc=None, pad=0):
    """[n, H, W, bpp] pixels, the statuses, and the padding bytes of every row."""
    fourcc = N.FOURCC_BGR if fourcc is None else fourcc
    buf, pitch, status = N.decode_jpeg_host(files, fourcc, pad)
    info = N.jpeg_info_struct(files[0])
    bpp = 3 if fourcc == N.FOURCC_BGR else 4
    row = info.width * bpp
    return buf[:, :, :row].reshape(len(files), info.height, info.width, bpp), status, buf[:, :, row:]


def check(N, file, ref, what):
    px, status, _ = decode(N, [file])
    assert status[0] == 0, what
    assert px.shape[1:] == ref.shape, what
    bad = np.argwhere(px[0] != ref)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first {bad[:3].tolist()}"


def test_fixtures_equal_pillow(evam):
    N = evam.native
    fx = C.fixtures()
    assert len(fx) >= 40
    for name, (f, ref) in fx.items():
        check(N, f, ref, name)
    enc = C.encoder_fixtures()
    assert len(enc) == 21
    for name, (f, ref) in enc.items():
        check(N, f, ref, name)


@pytest.mark.parametrize("pad", [0, 16, 48])
def test_fourcc_and_pitch(evam, pad):
    """BGR and BGRX (X = 255) at padded pitches: the bytes behind every row's pixels are never written."""
    N = evam.native
    for name in ("w3_420", "noise_64x48_422", "w5_grey", "rst1_33x17_420", "sat_31x23_q100_422"):
        f, ref = C.fixtures()[name]
        for fourcc in (N.FOURCC_BGR, N.FOURCC_BGRX):
            px, status, padding = decode(N, [f, f], fourcc, pad)
            assert status.tolist() == [0, 0]
            for i in range(2):
                assert np.array_equal(px[i][..., :3], ref), (name, fourcc)
            if fourcc == N.FOURCC_BGRX:
                assert (px[..., 3] == 255).all()
            assert (padding == 0xA5).all(), (name, fourcc, pad)


def test_adobe_ycc_file_decodes(evam):
    f, ref = C.fixtures()["noise_64x48_444"]
    check(evam.native, C.adobe_ycc(f), ref, "Adobe transform 1")


def test_jpeg_info_fields(evam):
    fx = C.fixtures()
    for name, (f, ref) in fx.items():
        i = evam.jpeg_info(f)
        assert (i.height, i.width) == ref.shape[:2], name
        samp = name.rsplit("_", 1)[-1]
        want = {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "grey": (1, 1, 1)}[samp]
        assert (i.components, i.h_samp, i.v_samp) == want, name
        assert f[i.scan_offset - 14 if i.components == 3 else i.scan_offset - 10:][:2] == b"\xFF\xDA", name
        assert (i.restart_interval > 0) == name.startswith("rst"), name
    assert evam.jpeg_info(fx["rst3_40x24_422"][0]).restart_interval == 3
    assert evam.jpeg_info(fx["rstrow_64x48_444"][0]).restart_interval == 8
    assert evam.jpeg_info(bytearray(fx["w1_420"][0])).width == 1
    assert evam.jpeg_info(memoryview(fx["w1_420"][0])).width == 1
    with pytest.raises(evam.PreProcError) as e:
        evam.jpeg_info(C.refused_fixture())
    assert e.value.status == evam.native.ERR_UNSUPPORTED and "progressive" in str(e.value)


def _raw_host(N, files, imgs, n=None, status=None):
    lib = N.load_library()
    keep, ptrs, lens = N.jpeg_file_arrays(files)
    st = np.full(max(len(files), 1), 77, np.int32) if status is None else status
    rc = lib.evam_pp_decode_jpeg_host(ptrs, lens, len(files) if n is None else n, imgs,
                                      None if st is False else st.ctypes.data)
    return rc, st, lib.evam_pp_last_error().decode()


def _out_images(N, n, w, h, fourcc, pitch=None, offset=0):
    bpp = 3 if fourcc == N.FOURCC_BGR else 4
    pitch = (w * bpp + 15) // 16 * 16 if pitch is None else pitch
    raw = np.full(n * h * max(pitch, 16) + 64, 0x5A, np.uint8)
    off = (-raw.ctypes.data) % 16 + offset
    imgs = (N.EvamImage * n)()
    for i in range(n):
        imgs[i].fourcc, imgs[i].width, imgs[i].height = fourcc, w, h
        imgs[i].pitch[0] = pitch
        imgs[i].planes[0] = raw.ctypes.data + off + i * h * pitch
    return imgs, raw


def test_refused_files(evam):
    """Every refusal of the header parse: its status, a message that names the reason, nothing written."""
    N = evam.native
    cases = C.refusals()
    assert len(cases) >= 25
    for name, f, want, word in cases:
        with pytest.raises(evam.PreProcError) as e:
            N.jpeg_info_struct(f)
        assert e.value.status == want and word in str(e.value), (name, str(e.value))
        imgs, raw = _out_images(N, 1, 64, 48, N.FOURCC_BGR)
        rc, st, msg = _raw_host(N, [f], imgs)
        assert rc == want and word in msg and "files[0]" in msg, (name, rc, msg)
        assert (raw == 0x5A).all() and st[0] == 77, name
    f = C.refused_fixture()
    imgs, raw = _out_images(N, 1, 16, 16, N.FOURCC_BGR)
    rc, st, msg = _raw_host(N, [f], imgs)
    assert rc == N.ERR_UNSUPPORTED and "progressive" in msg and (raw == 0x5A).all()


def test_refused_arguments(evam):
    N = evam.native
    fx = C.fixtures()
    f = fx["noise_64x48_420"][0]
    INV = N.ERR_INVALID_ARG

    def refused(files, imgs, raw, word, **kw):
        rc, st, msg = _raw_host(N, files, imgs, **kw)
        assert rc == INV and word in msg, (rc, msg)
        assert (raw == 0x5A).all()

    imgs, raw = _out_images(N, 2, 64, 48, N.FOURCC_BGR)
    for other in ("noise_64x48_422", "noise_64x48_grey", "rstwrap_64x48_420", "w3_420"):
        refused([f, fx[other][0]], imgs, raw, "geometry")
    refused([f], *_out_images(N, 1, 48, 64, N.FOURCC_BGR), "out[0] is 48x64")
    refused([f], *_out_images(N, 1, 64, 48, N.FOURCC_NV12), "fourcc")
    refused([f], *_out_images(N, 1, 64, 48, N.FOURCC_BGRA), "fourcc")
    refused([f], *_out_images(N, 1, 64, 48, N.FOURCC_BGR, pitch=200), "multiples of 16")
    refused([f], *_out_images(N, 1, 64, 48, N.FOURCC_BGR, pitch=176), "at least 192")
    refused([f], *_out_images(N, 1, 64, 48, N.FOURCC_BGR, offset=4), "multiples of 16")
    imgs, raw = _out_images(N, 1, 64, 48, N.FOURCC_BGR)
    refused([f], imgs, raw, "outside 1..65535", n=0)
    refused([f], imgs, raw, "outside 1..65535", n=65536)
    refused([f], imgs, raw, "NULL", status=False)
    lib = N.load_library()
    assert lib.evam_pp_decode_jpeg_host(None, None, 1, imgs, None) == INV
    assert lib.evam_pp_jpeg_info(None, 10, None) == INV
    assert lib.evam_pp_decode_jpeg(None, None, None, 1, None, None) == INV  # no handle: nothing reaches a device
    with pytest.raises(evam.PreProcError):
        N.jpeg_info_struct("a string")


def test_damaged_scans_end_with_a_status(evam):
    N = evam.native
    for name, f, must_fail in C.damaged_scans():
        px, status, padding = decode(N, [f], N.FOURCC_BGRX, 16)
        assert status[0] in (0, N.ERR_INVALID_ARG), name
        if must_fail:
            assert status[0] == N.ERR_INVALID_ARG, name
        assert (padding == 0xA5).all(), name


def test_a_damaged_file_leaves_its_neighbours_alone(evam):
    N = evam.native
    f, ref = C.fixtures()["noise_64x48_420"]
    bad = C.damaged_scans()[1][1]
    px, status, _ = decode(N, [f, bad, f])
    assert status.tolist() == [0, N.ERR_INVALID_ARG, 0]
    assert np.array_equal(px[0], ref) and np.array_equal(px[2], ref)


def test_stuffed_bytes_and_long_codes_are_in_the_fixtures():
    """What the fixtures must contain to reach the decoder's rarer paths, asserted on the files alone."""
    fx = C.fixtures()
    look = C.source_constant("kJdecLook")
    assert C.max_code_length(fx["noise_64x48_420"][0]) == 16 > look  # Annex K AC tables: codes up to 16 bits
    assert any(C.max_code_length(f) > look for k, (f, _) in fx.items() if k.startswith("optimize"))
    s, e = C.scan_bounds(fx["noise_64x48_420"][0])
    assert b"\xFF\x00" in fx["noise_64x48_420"][0][s:e]
    wrap = fx["rstwrap_64x48_420"][0]
    s, e = C.scan_bounds(wrap)
    assert wrap[s:e].count(b"\xFF\xD0") >= 2 and b"\xFF\xD7" in wrap[s:e]  # more than 8 intervals: RST0..7 wraps


# ---- fresh files, decoded by Pillow and by the host twin ----------------------------------------------------------

def pillow_file(bgr, quality, sampling, **extra):
    from PIL import Image, ImageFile

    ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 22)  # optimize=True on noise outgrows the default buffer
    if sampling is None:
        im, args = Image.fromarray(np.ascontiguousarray(bgr[..., 1])), {}
    else:
        im, args = Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])), {"subsampling": sampling}
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **args, **extra)
    return buf.getvalue()


def pillow_pixels(file):
    from PIL import Image

    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(file)).convert("RGB"))[..., ::-1])


def test_420_residue_grid_from_the_reference_encoder(evam):
    """Every size W, H in 1..33 (all residues of the 16x16 MCU, the chroma-width <= 2 rule at W <= 4), files of
    jpeg_ref.encode."""
    pytest.importorskip("PIL")
    N = evam.native
    rng = np.random.default_rng(33)
    for h in range(1, 34):
        for w in range(1, 34):
            f, _ = jpeg_ref.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), int(rng.choice([35, 75, 95])))
            check(N, f, pillow_pixels(f), f"{w}x{h}")


def test_sixty_pillow_files(evam):
    pytest.importorskip("PIL")
    N = evam.native
    kinds = jpeg_content.KINDS
    n = 0
    for si, samp in enumerate((0, 1, 2, None)):
        for qi, q in enumerate((1, 10, 50, 90, 100)):
            for k in range(3):
                kind = kinds[(si * 15 + qi * 3 + k) % len(kinds)]
                w, h = 17 + 13 * k + si, 9 + 7 * qi + k
                f = pillow_file(jpeg_content.content(kind, w, h, seed=n), q, samp)
                check(N, f, pillow_pixels(f), f"{kind} {w}x{h} q{q} sampling {samp}")
                n += 1
    assert n == 60


def test_restart_intervals_fresh(evam):
    pytest.importorskip("PIL")
    N = evam.native
    rng = np.random.default_rng(5)
    for samp in (0, 1, 2, None):
        for extra in ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 5}, {"restart_marker_rows": 1},
                      {"restart_marker_rows": 2}):
            bgr = rng.integers(0, 256, (70, 123, 3), dtype=np.uint8)
            f = pillow_file(bgr, 85, samp, **extra)
            assert evam.jpeg_info(f).restart_interval > 0
            check(N, f, pillow_pixels(f), f"sampling {samp} {extra}")


def test_optimised_tables_reach_the_maxcode_walk(evam):
    """optimize=True on 256x256 saturated noise at quality 100: tables of the file's own, with codes longer than the
    look-ahead table resolves, so the Annex F walk is reached (the width is read from the source)."""
    pytest.importorskip("PIL")
    N = evam.native
    look = C.source_constant("kJdecLook")
    longest = 0
    for samp in (0, 1, 2, None):
        f = pillow_file(jpeg_content.content("sat", 256, 256, seed=9), 100, samp, optimize=True)
        longest = max(longest, C.max_code_length(f))
        check(N, f, pillow_pixels(f), f"optimised, sampling {samp}")
    assert longest > look, (longest, look)


@pytest.mark.parametrize("colour", [False, True])
def test_blocks_longer_than_a_sub_sequence(evam, colour):
    """The hand-written files whose blocks are all longer than S bits (the GPU tests decode larger ones of the same
    builder): libjpeg reads them as the host twin does, and every block's length is asserted."""
    pytest.importorskip("PIL")
    f, ends = C.long_block_file(40, 24, colour, seed=3)
    assert min(np.diff([0] + ends)) > C.source_constant("kJdecSubBits")
    assert C.max_code_length(f) == 16
    check(evam.native, f, pillow_pixels(f), f"long blocks, colour {colour}")
    if colour:
        f, ends = C.long_block_file(40, 24, True, seed=3, sampling="422", restart=1)
        assert evam.jpeg_info(f).restart_interval == 1 and evam.jpeg_info(f).h_samp == 2 and evam.jpeg_info(f).v_samp == 1
        assert len(C.rst_markers(f)) == 3 * 3 - 1 and len(ends) == 9 * 4
        check(evam.native, f, pillow_pixels(f), "long blocks, 4:2:2, restart 1")


# ---- the files of tests/test_gpu_jpeg_dec_sweep.py: the host twin is what the GPU is compared with there ------------

def check_files(N, files, what):
    """Files of one geometry in one call of the twin, each against Pillow's decode of it."""
    px, status, _ = decode(N, files)
    assert status.tolist() == [0] * len(files), what
    for i, f in enumerate(files):
        ref = pillow_pixels(f)
        bad = np.argwhere(px[i] != ref)
        assert bad.size == 0, f"{what} file {i}: {len(bad)} bytes differ, first {bad[:3].tolist()}"


@pytest.mark.parametrize("sampling,restart", [("444", 0), ("444", 1), ("422", 0), ("422", 1), ("grey", 0), ("grey", 1),
                                              ("420", 1)])
def test_sweep_residue_grids_equal_pillow(evam, sampling, restart):
    """The whole residue grids of the GPU sweep (not a sample of them), the same files."""
    pytest.importorskip("PIL")
    widths, heights = C.RESIDUE_GRIDS[sampling]
    n = 0
    for h in heights:
        for w, files in C.residue_files(sampling, restart, h, widths):
            info = evam.jpeg_info(files[0])
            assert (info.width, info.height, info.restart_interval) == (w, h, restart)
            check_files(evam.native, files, f"{sampling} restart {restart} {w}x{h}")
            n += 1
    assert n == len(widths) * len(heights)


@pytest.mark.parametrize("sampling", C.SAMPLINGS)
def test_sweep_long_restart_scans_equal_pillow(evam, sampling):
    """Scans longer than two passes of evam_jdec_unstuff: a marker behind every MCU (the cut-pairs file), and behind
    every MCU row (the wide frame); and the tall frame."""
    pytest.importorskip("PIL")
    f = C.cut_pairs_file(sampling)
    assert C.cut_pairs_properties(f)["len"] > 2 * C.PASS + 1 and evam.jpeg_info(f).restart_interval == 1
    check_files(evam.native, [f], f"cut pairs {sampling}")
    (what, wide), (_, tall) = C.wide_and_tall_files(sampling)
    s, e = C.scan_bounds(wide)
    assert e - s > 2 * C.PASS + 1 and evam.jpeg_info(wide).restart_interval == -(-C.WIDE // C.mcu_size(sampling)[0])
    assert len(C.rst_markers(wide)) == -(-24 // C.mcu_size(sampling)[1]) - 1
    check_files(evam.native, [wide], f"{what} {sampling}")
    check_files(evam.native, [tall], f"24x1100 {sampling}")


def test_sweep_long_and_many_intervals_equal_pillow(evam):
    """The grey file with two intervals longer than S * T bits, and the files with 2,047, 292 and 255 markers."""
    pytest.importorskip("PIL")
    f, restart, mcus = C.long_interval_file("grey")
    table = C.interval_table(f)
    chunk = C.source_constant("kJdecSubBits") * C.source_constant("kJdecChunk") // 8
    assert len(table) == 4 and table[1] > chunk and table[2] - table[1] > chunk and table[3] - table[2] < chunk
    check_files(evam.native, [f], "long intervals")
    for (what, f, restart), markers in zip(C.many_interval_files(), (2047, 292, 255)):
        assert len(C.rst_markers(f)) == markers and evam.jpeg_info(f).restart_interval == restart
        check_files(evam.native, [f], what)
    for sampling in ("422", "444"):
        for restart in (1, 3):
            f, _ = C.long_block_file(40, 24, True, seed=restart, sampling=sampling, restart=restart)
            check_files(evam.native, [f], f"long blocks {sampling} restart {restart}")


def test_damaged_restart_scans_end_with_a_status(evam):
    N = evam.native
    for name, f, must_fail in C.damaged_restart_scans():
        px, status, padding = decode(N, [f], N.FOURCC_BGRX, 16)
        assert status[0] == N.ERR_INVALID_ARG and must_fail, name
        assert (padding == 0xA5).all(), name


# ---- pipeline server: the source item forms, with a stand-in decoder -----------------------------------------------

def test_pipeline_source_item_forms(evam):
    ps = evam.pipeline_server
    f = C.fixtures()["w1_420"][0]
    calls = []

    class Decoder:
        def decode_jpeg(self, files, fourcc):
            calls.append((list(files), fourcc))
            return [evam.Image(evam.native.FOURCC_BGRX, 1, 5, []) for _ in files]

        def close(self):
            calls.append("closed")

    p = ps.Pipeline.__new__(ps.Pipeline)
    p.device, p._decode_pp, p._export_pp, p._export_host = 0, None, None, None
    p._new_decoder = lambda: Decoder()
    img = evam.Image(evam.native.FOURCC_BGRX, 4, 4, [])
    host = {"fourcc": evam.native.FOURCC_BGRX, "width": 4, "height": 4, "planes": []}
    got = [f, img, bytearray(f), {"jpeg": memoryview(f), "timestamp": 41}, host]
    assert [ps.Pipeline._jpeg_of(x) is not None for x in got] == [True, False, True, True, False]
    dec = p._decode_burst(got)
    assert sorted(dec) == [0, 2, 3] and all(isinstance(v, evam.Image) for v in dec.values())
    assert len(calls) == 1 and calls[0][1] == "BGRX" and len(calls[0][0]) == 3  # one decode call per pull
    assert p._decode_burst([img, host]) == {} and len(calls) == 1
    assert p._as_image(img) is img
    assert p._as_image(f).width == 1 and len(calls) == 2
    with pytest.raises(TypeError):
        p._as_image(3.5)
    p._close_export()
    assert calls[-1] == "closed" and p._decode_pp is None

    class Refusing(Decoder):
        def decode_jpeg(self, files, fourcc):
            raise evam.PreProcError(evam.native.ERR_UNSUPPORTED, "decode_jpeg: files[0]: progressive JPEG")

    p._new_decoder = lambda: Refusing()
    with pytest.raises(evam.PreProcError, match="progressive"):
        p._decode_burst([C.refused_fixture()])


def test_decode_jpeg_names_the_refused_file(evam):
    """HipPreProcessor.decode_jpeg without a device: a header the parse refuses is named by its index before anything
    is allocated or launched."""
    fx = C.fixtures()
    P = evam.HipPreProcessor
    pp = P.__new__(P)
    with pytest.raises(evam.PreProcError, match=r"files\[1\].*progressive"):
        P.decode_jpeg(pp, [fx["w1_420"][0], C.refused_fixture()])
    assert P.decode_jpeg(pp, []) == []
