"""CPU tests of the JPEG decoder's raw-plane output: ``evam_pp_decode_jpeg_planes_host`` (the arithmetic and the clipped
stores the kernel shares, driven sequentially) against the planes Pillow (libjpeg-turbo) yields, byte for byte: the
stored fixtures always, fresh files where Pillow is importable. Also every refusal, the write bound for every output
layout and for damaged scans, ``decode_jpeg``'s routing without a device, and the pipeline source's ``jpeg_format``."""
import io
import types

import numpy as np
import pytest

import jpeg_content
import jpeg_dec_cases as C
import jpeg_planes_cases as PC

FORMATS = ("NV12", "I420")


def check(N, files, planes, fmt, kinds, what, seed=0):
    """Decode ``files`` (one geometry) into a surface of ``kinds``; the whole buffer must equal the expected one."""
    h, w = planes[0][0].shape
    s = PC.Surface(fmt, w, h, kinds, seed)
    rc, buf, st, msg = PC.decode_host(N, files, s)
    assert rc == 0, (what, rc, msg)
    assert st.tolist() == [0] * len(files), (what, st)
    diff = PC.first_difference(buf, s.expected([PC.planes_of(p, fmt) for p in planes]))
    assert not diff, f"{what} {fmt} {kinds}: {diff}"


@pytest.mark.parametrize("fmt", FORMATS)
def test_fixtures_equal_pillow(evam, fmt):
    fx = PC.fixtures()
    names = set(fx)
    for w, h in ((2, 2), (16, 16), (18, 2), (2, 18), (10, 10), (24, 8), (6, 14), (30, 46), (34, 18), (64, 48), (48, 64)):
        assert {f"grad_{w}x{h}_q90", f"sat_{w}x{h}_q100"} <= names
    assert sum(k.startswith("dec/") for k in fx) == 6 and sum(k.startswith("enc/") for k in fx) == 13
    assert sum(evam.jpeg_info(f).restart_interval > 0 for k, (f, _) in fx.items() if "/" not in k) == 3
    for k, (name, (f, ycc)) in enumerate(fx.items()):
        check(evam.native, [f], [ycc], fmt, [PC.KINDS[k % len(PC.KINDS)]], name, seed=k)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", PC.KINDS)
def test_every_layout_kind_keeps_the_noise(evam, fmt, kind):
    """Three files per call in one layout kind, at the sizes whose right and bottom edges clip differently: the
    buffer afterwards is the noise with only the pixel bytes replaced."""
    fx = PC.fixtures()
    for size in ("2x2", "10x10", "24x8", "18x2", "2x18", "6x14", "34x18", "64x48"):
        a, b = fx[f"grad_{size}_q90"], fx[f"sat_{size}_q100"]
        check(evam.native, [a[0], b[0], a[0]], [a[1], b[1], a[1]], fmt, [kind] * 3, size, seed=len(size))


def test_mixed_layout_kinds_in_one_call(evam):
    fx = PC.fixtures()
    a, b = fx["grad_30x46_q90"], fx["sat_30x46_q100"]
    for fmt in FORMATS:
        check(evam.native, [a[0], b[0], a[0], b[0], a[0]], [a[1], b[1], a[1], b[1], a[1]], fmt, list(PC.KINDS), "30x46")


def test_native_helper_returns_compact_planes(evam):
    N = evam.native
    f, ycc = PC.fixtures()["sat_10x10_q100"]
    for fmt, fc in (("NV12", N.FOURCC_NV12), ("I420", N.FOURCC_I420)):
        planes, st = N.decode_jpeg_planes_host([f, f], fc)
        assert st.tolist() == [0, 0] and len(planes) == 2
        for got, want in zip(planes[1], PC.planes_of(ycc, fmt)):
            assert np.array_equal(got, want)


# ---- fresh files ---------------------------------------------------------------------------------------------------

def pillow_420(bgr, quality, **extra):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, **extra)
    return buf.getvalue()


def test_three_hundred_fresh_pillow_files(evam):
    """Even sizes 2..130, qualities 1..100, five kinds of content, with and without restart intervals."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(420)
    kinds = ("noise", "sat", "grad", "checker", "halves")
    extras = ({}, {}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1})
    n = with_rst = 0
    for i in range(320):
        w, h = 2 * int(rng.integers(1, 66)), 2 * int(rng.integers(1, 66))
        q = (1, 50, 100, 10, 75, 90, 95)[i % 7]
        extra = extras[(i // 7) % len(extras)]
        f = pillow_420(jpeg_content.content(kinds[i % 5], w, h, seed=i), q, **extra)
        info = evam.jpeg_info(f)
        assert evam.jpeg_planes_ok(info) and (info.restart_interval > 0) == bool(extra)
        with_rst += bool(extra)
        check(evam.native, [f], [PC.pillow_planes(f)], FORMATS[i % 2], [PC.KINDS[i % 5]],
              f"{kinds[i % 5]} {w}x{h} q{q} {extra}", seed=i)
        n += 1
    assert n >= 300 and 100 < with_rst < 250


@pytest.mark.parametrize("fmt", FORMATS)
def test_sweep_restart_files_equal_pillow(evam, fmt):
    """The 4:2:0 files tests/test_gpu_jpeg_dec_sweep.py decodes to planes: a marker behind every MCU (the cut-pairs
    file's even-sized sibling and the 256-MCU gradient), and two intervals longer than one chunk of evam_jdec_sync."""
    pytest.importorskip("PIL")
    f = C.cut_pairs_file("420")
    assert len(C.rst_markers(f)) == C.cut_pairs_width("420") // 16 - 1 and evam.jpeg_planes_ok(evam.jpeg_info(f))
    check(evam.native, [f], [PC.pillow_planes(f)], fmt, ["unequal"], "cut pairs")
    what, f, restart = C.many_interval_files()[2]
    assert evam.jpeg_info(f).restart_interval == 1 and len(C.rst_markers(f)) == 255
    check(evam.native, [f], [PC.pillow_planes(f)], fmt, ["window"], what)
    f, restart, mcus = C.long_interval_file("420")
    table = C.interval_table(f)
    chunk = C.source_constant("kJdecSubBits") * C.source_constant("kJdecChunk") // 8
    assert len(table) == 4 and table[1] > chunk and table[2] - table[1] > chunk > table[3] - table[2]
    for kind in ("unequal", "window"):
        check(evam.native, [f], [PC.pillow_planes(f)], fmt, [kind], "long intervals")


# ---- refusals ------------------------------------------------------------------------------------------------------

def refused(N, files, surface, want, words, **kw):
    rc, buf, st, msg = PC.decode_host(N, files, surface, **kw)
    assert rc == want and all(w in msg for w in words), (rc, msg, words)
    assert np.array_equal(buf, surface.noise), msg
    if st is not False:
        assert (st == 77).all(), msg
    return msg


def test_refused_files(evam):
    """Every refusal of the header parse keeps its status and its word, and the files the plane output does not serve
    are refused with ERR_UNSUPPORTED: nothing is written."""
    N = evam.native
    cases = C.refusals()
    assert len(cases) >= 25
    for fmt in FORMATS:
        s = PC.Surface(fmt, 64, 48, ["unequal"])
        for name, f, want, word in cases:
            refused(N, [f], s, want, [word, "files[0]"])
        refused(N, [C.refused_fixture()], PC.Surface(fmt, 16, 16, ["compact"]), N.ERR_UNSUPPORTED, ["progressive"])
    fx = C.fixtures()
    good = fx["noise_64x48_420"][0]
    for name, word in (("noise_64x48_444", "sampling"), ("noise_64x48_422", "sampling"), ("noise_64x48_grey", "sampling")):
        for fmt in FORMATS:
            refused(N, [fx[name][0]], PC.Surface(fmt, 64, 48, ["compact"]), N.ERR_UNSUPPORTED, [word, "files[0]"])
            refused(N, [good, fx[name][0]], PC.Surface(fmt, 64, 48, ["compact"] * 2), N.ERR_UNSUPPORTED,
                    [word, "files[1]"])
    odd_w, odd_h = fx["rst1_33x17_420"][0], C.patch(good, C.find_segment(good, 0xC0)[1] + 5, [0, 47])
    assert evam.jpeg_info(odd_h).height == 47 and evam.jpeg_info(odd_h).width == 64
    odd_w2 = C.patch(good, C.find_segment(good, 0xC0)[1] + 7, [0, 63])
    assert evam.jpeg_info(odd_w2).width == 63 and evam.jpeg_info(odd_w2).height == 48
    for f, (w, h) in ((odd_w, (34, 18)), (odd_h, (64, 48)), (odd_w2, (64, 48)), (fx["w3_420"][0], (4, 6))):
        for fmt in FORMATS:
            refused(N, [f], PC.Surface(fmt, w, h, ["compact"]), N.ERR_UNSUPPORTED, ["odd", "files[0]"])


def test_refused_arguments(evam):
    N = evam.native
    INV = N.ERR_INVALID_ARG
    fx = C.fixtures()
    f = fx["noise_64x48_420"][0]
    for fmt in FORMATS:
        two = PC.Surface(fmt, 64, 48, ["compact"] * 2)
        for other in ("rstwrap_64x48_420", "exif_com_16x16_420", "optimize_48x32_420"):
            refused(N, [f, fx[other][0]], two, INV, ["geometry"])
        refused(N, [f], PC.Surface(fmt, 48, 64, ["compact"]), INV, ["out[0] is 48x64"])
        s = PC.Surface(fmt, 64, 48, ["compact"])
        refused(N, [f], s, INV, ["outside 1..65535"], n=0)
        refused(N, [f], s, INV, ["outside 1..65535"], n=65536)
        refused(N, [f], s, INV, ["NULL"], status=False)

    def with_images(fmt, edit, words, n=1):
        s = PC.Surface(fmt, 64, 48, ["unequal"] * n)
        orig = s.c_images

        def c_images(N_, base):
            imgs = orig(N_, base)
            edit(imgs)
            return imgs

        s.c_images = c_images
        return refused(N, [f] * n, s, INV, words)

    def setter(i, **kw):
        def edit(imgs):
            for k, v in kw.items():
                if k == "fourcc":
                    imgs[i].fourcc = v
                elif k.startswith("pitch"):
                    imgs[i].pitch[int(k[5])] = v(imgs[i].pitch[int(k[5])]) if callable(v) else v
                else:
                    imgs[i].planes[int(k[5])] = v(imgs[i].planes[int(k[5])]) if callable(v) else v
        return edit

    for fc in (N.FOURCC_BGR, N.FOURCC_BGRX, N.FOURCC_BGRA):
        with_images("NV12", setter(0, fourcc=fc), ["fourcc", "out[0]"])
    with_images("NV12", setter(1, fourcc=N.FOURCC_I420), ["fourcc", "out[1]"], n=2)  # two fourccs in one call
    for fmt, npl in (("NV12", 2), ("I420", 3)):
        for p in range(npl):
            row = 64 if p == 0 or fmt == "NV12" else 32
            with_images(fmt, setter(0, **{f"plane{p}": None}), ["NULL", "out[0]"])
            with_images(fmt, setter(0, **{f"plane{p}": lambda v: v + 4}), ["multiples of 16", f"plane {p}"])
            with_images(fmt, setter(0, **{f"pitch{p}": lambda v: v + 8}), ["multiples of 16", f"plane {p}"])
            with_images(fmt, setter(0, **{f"pitch{p}": row - 16}), [f"at least {row}", f"plane {p}"])
            with_images(fmt, setter(0, **{f"pitch{p}": (1 << 31) // (48 if p == 0 else 24) // 16 * 16 + 16}), ["2 GiB"])
    lib = N.load_library()
    assert lib.evam_pp_decode_jpeg_planes_host(None, None, 1, None, None) == INV
    assert lib.evam_pp_decode_jpeg_planes(None, None, None, 1, None, None) == INV  # no handle: nothing reaches a device
    assert "evam_pp_decode_jpeg_planes" in lib.evam_pp_last_error().decode()


def test_the_pixel_entry_points_still_refuse_planes(evam):
    """evam_pp_decode_jpeg_host keeps refusing NV12 / I420 output, with its message."""
    N = evam.native
    f = C.fixtures()["noise_64x48_420"][0]
    s = PC.Surface("NV12", 64, 48, ["compact"])
    buf, base = s.host_buffer()
    keep, ptrs, lens = N.jpeg_file_arrays([f])
    st = np.full(1, 77, np.int32)
    lib = N.load_library()
    rc = lib.evam_pp_decode_jpeg_host(ptrs, lens, 1, s.c_images(N, base), st.ctypes.data)
    assert rc == N.ERR_INVALID_ARG and "BGR or BGRX is written" in lib.evam_pp_last_error().decode()
    assert np.array_equal(buf, s.noise)


# ---- damaged scans -------------------------------------------------------------------------------------------------

def eligible_damaged(evam):
    out = [(name, f, must) for name, f, must in C.damaged_scans() if evam.jpeg_planes_ok(evam.jpeg_info(f))]
    assert len(out) >= 10
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_damaged_scans_end_with_a_status(evam, fmt):
    N = evam.native
    for k, (name, f, must_fail) in enumerate(eligible_damaged(evam)):
        s = PC.Surface(fmt, 64, 48, [PC.KINDS[k % len(PC.KINDS)]], seed=k)
        rc, buf, st, msg = PC.decode_host(N, [f], s)
        assert rc == 0 and st[0] in (0, N.ERR_INVALID_ARG), (name, rc, st, msg)
        if must_fail:
            assert st[0] == N.ERR_INVALID_ARG, name
        assert s.outside_intact(buf), name


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_damaged_file_leaves_its_neighbours_alone(evam, fmt):
    N = evam.native
    fx = PC.fixtures()
    a, b = fx["dec/noise_64x48_420"], fx["grad_64x48_q90"]
    bad = C.damaged_scans()[1][1]
    s = PC.Surface(fmt, 64, 48, ["window", "reversed", "unequal"], seed=3)
    rc, buf, st, msg = PC.decode_host(N, [a[0], bad, b[0]], s)
    assert rc == 0 and st.tolist() == [0, N.ERR_INVALID_ARG, 0], (rc, st, msg)
    assert s.outside_intact(buf)
    want = s.expected([PC.planes_of(a[1], fmt), s.extract(buf, 1), PC.planes_of(b[1], fmt)])
    assert not PC.first_difference(buf, want)


# ---- Python routing, without a device ------------------------------------------------------------------------------

def test_jpeg_planes_ok(evam):
    for name, (f, _) in PC.fixtures().items():
        assert evam.jpeg_planes_ok(evam.jpeg_info(f)), name
        assert evam.native.jpeg_planes_ok(evam.native.jpeg_info_struct(f)), name
    n_ok = 0
    for name, (f, ref) in C.fixtures().items():
        h, w = ref.shape[:2]
        want = name.endswith("_420") and w % 2 == 0 and h % 2 == 0
        assert evam.jpeg_planes_ok(evam.jpeg_info(f)) == want, name
        n_ok += want
    assert 0 < n_ok < len(C.fixtures())


def test_decode_jpeg_names_the_first_file_without_planes(evam):
    """No device: the files the plane output does not serve are named before anything is allocated or launched."""
    fx = C.fixtures()
    P = evam.HipPreProcessor
    pp = P.__new__(P)
    ok = fx["noise_64x48_420"][0]
    for fmt in FORMATS:
        for bad in ("noise_64x48_444", "noise_64x48_422", "noise_64x48_grey", "rst1_33x17_420", "w3_420"):
            with pytest.raises(evam.PreProcError, match=r"files\[2\].*4:2:0") as e:
                P.decode_jpeg(pp, [ok, ok, fx[bad][0], fx["w1_444"][0]], fmt)
            assert e.value.status == evam.native.ERR_UNSUPPORTED
        with pytest.raises(evam.PreProcError, match=r"files\[1\].*progressive"):
            P.decode_jpeg(pp, [ok, C.refused_fixture()], fmt, fallback="BGRX")
        assert P.decode_jpeg(pp, [], fmt) == []
    for fourcc, fallback in (("BGRX", "BGRX"), ("NV12", "NV12"), ("I420", "RGB"), ("BGR", "BGR")):
        with pytest.raises(evam.PreProcError, match="fallback") as e:
            P.decode_jpeg(pp, [ok], fourcc, fallback=fallback)
        assert e.value.status == evam.native.ERR_INVALID_ARG


def test_fallback_groups_and_order(evam, monkeypatch):
    """decode_jpeg with a stand-in for the decode call: one call per (geometry, target fourcc) group, files without
    planes routed to the fallback format, the result in the order given, the statuses read back once."""
    import torch

    N = evam.native
    P = evam.HipPreProcessor
    fx = C.fixtures()
    names = ["noise_64x48_420", "noise_64x48_444", "grad_64x48_q10_420", "rst1_33x17_420", "noise_64x48_444",
             "exif_com_16x16_420", "rstwrap_64x48_420", "noise_64x48_grey"]
    files = [fx[k][0] + bytes(i) for i, k in enumerate(names)]  # distinct bytes: a tail behind EOI is never parsed
    calls, reads = [], []

    class Status:
        def __init__(self, t):
            self.t = t

        def __getitem__(self, s):
            return Status(self.t[s])

        def cpu(self):
            reads.append(1)
            return self.t

    fake = types.SimpleNamespace(empty=lambda shape, dtype, device: Status(torch.zeros(shape, dtype=dtype)),
                                 int32=torch.int32)
    monkeypatch.setattr(evam.Image, "alloc", classmethod(
        lambda cls, fourcc, w, h, device="cuda", pitch_align=64: cls(fourcc, w, h, [])))
    pp = P.__new__(P)
    pp._torch, pp.device, pp._follow_torch_stream = fake, 0, True
    pp.decode_jpeg_into = lambda fs, imgs, status: calls.append(([files.index(f) for f in fs], imgs[0].fourcc))
    for fmt, fc in (("NV12", N.FOURCC_NV12), ("I420", N.FOURCC_I420)):
        calls.clear()
        reads.clear()
        imgs = P.decode_jpeg(pp, files, fmt, fallback="BGRX")
        want = [fc, N.FOURCC_BGRX, fc, N.FOURCC_BGRX, N.FOURCC_BGRX, fc, fc, N.FOURCC_BGRX]
        assert [im.fourcc for im in imgs] == want
        assert [(im.width, im.height) for im in imgs] == [(64, 48), (64, 48), (64, 48), (33, 17), (64, 48), (16, 16),
                                                          (64, 48), (64, 48)]
        # files 0 and 2 share a group; 1 and 4 (4:4:4, BGRX) share one; the restart-interval file 6 has its own
        assert calls == [([0, 2], fc), ([1, 4], N.FOURCC_BGRX), ([3], N.FOURCC_BGRX), ([5], fc), ([6], fc),
                         ([7], N.FOURCC_BGRX)]
        assert len(reads) == 1
        calls.clear()
        imgs = P.decode_jpeg(pp, files, fmt, fallback="BGR")
        assert [im.fourcc for im in imgs] == [N.FOURCC_BGR if v == N.FOURCC_BGRX else v for v in want]
    calls.clear()
    imgs = P.decode_jpeg(pp, files)  # the default is unchanged: BGRX for every file, grouped by geometry alone
    assert {im.fourcc for im in imgs} == {N.FOURCC_BGRX}
    assert calls == [([0, 2], N.FOURCC_BGRX), ([1, 4], N.FOURCC_BGRX), ([3], N.FOURCC_BGRX), ([5], N.FOURCC_BGRX),
                     ([6], N.FOURCC_BGRX), ([7], N.FOURCC_BGRX)]


def test_decode_jpeg_into_picks_the_entry_point(evam):
    """decode_jpeg_into calls evam_pp_decode_jpeg_planes for NV12 / I420 images and evam_pp_decode_jpeg otherwise."""
    import torch

    N = evam.native
    P = evam.HipPreProcessor
    called = []
    pp = P.__new__(P)
    pp._torch, pp._h = torch, None
    pp._check_device = lambda t: None
    pp._bind_stream = lambda: None
    pp._lib = types.SimpleNamespace(evam_pp_decode_jpeg=lambda *a: called.append("pixels") or 0,
                                    evam_pp_decode_jpeg_planes=lambda *a: called.append("planes") or 0)
    f = C.fixtures()["exif_com_16x16_420"][0]
    status = torch.zeros(1, dtype=torch.int32)
    for fc in (N.FOURCC_BGRX, N.FOURCC_NV12, N.FOURCC_BGR, N.FOURCC_I420):
        P.decode_jpeg_into(pp, [f], [evam.Image(fc, 16, 16, [])], status)
    assert called == ["pixels", "planes", "pixels", "planes"]


# ---- pipeline server: the source's jpeg_format ----------------------------------------------------------------------

def test_pipeline_source_jpeg_format(evam):
    ps = evam.pipeline_server
    N = evam.native
    assert ps.source_jpeg_format(None) == ps.source_jpeg_format({"type": "frames"}) == "BGRX"
    for fmt in ("BGRX", "I420", "NV12"):
        assert ps.source_jpeg_format({"type": "application", "jpeg_format": fmt}) == fmt
    for bad in ("BGR", "nv12", "RGB", "", None, 3, ["I420"]):
        p = ps.Pipeline.__new__(ps.Pipeline)
        with pytest.raises(evam.PreProcError, match="jpeg_format") as e:
            p.start(source={"type": "frames", "frames": [], "jpeg_format": bad})  # refused before anything is built
        assert e.value.status == N.ERR_INVALID_ARG
        assert not hasattr(p, "stages")

    f = C.fixtures()["exif_com_16x16_420"][0]
    calls = []

    class Decoder:
        def decode_jpeg(self, files, fourcc, **kw):
            calls.append((len(files), fourcc, kw))
            return [evam.Image(N.FOURCC_BGRX, 16, 16, []) for _ in files]

    p = ps.Pipeline.__new__(ps.Pipeline)
    p.device, p._decode_pp = 0, None
    p._new_decoder = lambda: Decoder()
    assert p._jpeg_format == "BGRX"
    p._decode_burst([f, f])
    assert calls == [(2, "BGRX", {})]  # the default route calls decode_jpeg exactly as before
    for fmt in ("I420", "NV12"):
        calls.clear()
        p._jpeg_format = fmt
        assert sorted(p._decode_burst([f, None, {"jpeg": f}])) == [0, 2]
        assert calls == [(2, fmt, {"fallback": "BGRX"})]
