"""Source plane layouts on every kernel family, bit-exact against the C oracle.

Every other GPU test reads frames whose planes are separate 256-byte-aligned allocations with one pitch rounding per
frame, and whose items share pitches within a launch. Here the frames come from tests/source_layouts.py: planes as
views into one noisy buffer, with pairwise different pitches, bases at 16 / 48 / 112 mod 256, chroma below luma, or as
windows of a wider surface, and the items of one launch each in another layout. Every case asserts the kernel family
that ran (``stats().kernels``), so a planner fallback cannot turn it into a test of another kernel.
"""
import os
import zlib

import numpy as np
import pytest

import bench
import source_layouts as SL
from test_gpu_half import half_full, narrow_bits, same_bits
from test_gpu_jpeg import check as jpeg_check
from test_gpu_parity import FORMATS, assert_same, fc, random_case, run_oracle
from test_gpu_plans import all_seven, expect_items

pytestmark = pytest.mark.gpu

NORM = {"range": (0.0, 1.0), "mean": (0.406, 0.456, 0.485), "std": (0.225, 0.224, 0.229)}
ITEM_KINDS = ["compact", "unequal+base16", "window+reversed"]  # items 0, 1, 2 of a family launch
OUTPUTS = ["u8", "f32", "nhwc_u8", "f16"]

# variant -> (family bit, environment, geometry). The environments are those of test_gpu_parity's
# test_wave_kernel_variants / test_band_six_column_lanes / FAMILY_ENVS.
VARIANTS = {
    "generic": ("GENERIC", {"EVAM_PP_ROWS": "0", "EVAM_PP_ROI": "0"}, "down"),
    "rows": ("ROWS", {"EVAM_PP_WAVE": "0", "EVAM_PP_STAGED": "0", "EVAM_PP_BAND": "0", "EVAM_PP_STRIP": "0"}, "rows"),
    "staged": ("STAGED", {"EVAM_PP_WAVE": "0", "EVAM_PP_STRIP": "0", "EVAM_PP_BAND": "0"}, "down"),
    "wave": ("WAVE", {"EVAM_PP_WAVE": "2"}, "up"),
    "strip_px1": ("STRIP", {"EVAM_PP_STRIP": "2", "EVAM_PP_STRIP_PX": "1"}, "down"),
    "strip_px1_unpaired": ("STRIP", {"EVAM_PP_STRIP": "2", "EVAM_PP_STRIP_PX": "1", "EVAM_PP_STRIP_PAIR": "0"}, "down"),
    "strip_px2": ("STRIP", {"EVAM_PP_STRIP": "2", "EVAM_PP_STRIP_PX": "2"}, "down2"),
    "strip_px2_unpaired": ("STRIP", {"EVAM_PP_STRIP": "2", "EVAM_PP_STRIP_PX": "2", "EVAM_PP_STRIP_PAIR": "0"}, "down2"),
    "band_dd1": ("BAND", {"EVAM_PP_BAND": "2", "EVAM_PP_STRIP": "0", "EVAM_PP_BAND_DD": "1"}, "band"),
    "band_dd0": ("BAND", {"EVAM_PP_BAND": "2", "EVAM_PP_STRIP": "0", "EVAM_PP_BAND_DD": "0"}, "band"),
}
# Variants that run only the EXTRA cases below: with them every instantiation of the kernel tables that the API and
# the knobs can reach is dispatched by some test of the suite.
_STAGED = VARIANTS["staged"][1]
EXTRA_VARIANTS = {
    "wave_px2": ("WAVE", {"EVAM_PP_WAVE": "2", "EVAM_PP_PX": "2"}, "up"),
    "wave_noreuse": ("WAVE", {"EVAM_PP_WAVE": "2", "EVAM_PP_REUSE": "0"}, "up"),
    "wave_noreuse_px1": ("WAVE", {"EVAM_PP_WAVE": "2", "EVAM_PP_REUSE": "0", "EVAM_PP_PX": "1"}, "up"),
    "wave_noreuse_px2": ("WAVE", {"EVAM_PP_WAVE": "2", "EVAM_PP_REUSE": "0", "EVAM_PP_PX": "2"}, "up"),
    "wave_noreuse_px4": ("WAVE", {"EVAM_PP_WAVE": "2", "EVAM_PP_REUSE": "0", "EVAM_PP_PX": "4"}, "up"),
    "strip_px2_paired": ("STRIP", {"EVAM_PP_STRIP": "2", "EVAM_PP_STRIP_PX": "2"}, "down2_packed"),
    "staged_r1": ("STAGED", dict(_STAGED, EVAM_PP_STAGE_R="1"), "down"),
    "staged_nsegx2": ("STAGED", dict(_STAGED, EVAM_PP_NSEGX="2"), "down"),
}
EXTRA = ([(v, fmt, "f16") for v in ("wave_noreuse_px1", "wave_noreuse_px2", "wave_noreuse_px4") for fmt in FORMATS] +
         [("wave_px2", fmt, "f16") for fmt in ("NV12", "I420", "BGR")] +
         [("wave_noreuse", fmt, "nhwc_f32") for fmt in ("NV12", "I420", "BGRX")] +
         [(v, fmt, "nhwc_f32") for v in ("strip_px1_unpaired", "strip_px2_unpaired") for fmt in ("NV12", "I420")] +
         [("strip_px2_unpaired", "BGRX", "nhwc_f32")] +
         [("strip_px2_paired", "BGRX", out) for out in ("u8", "f32", "f16")] +
         [("staged_r1", "BGRX", "u8"), ("staged_r1", "BGRX", "f32"), ("staged_nsegx2", "I420", "f32")])
VARIANTS_ALL = dict(VARIANTS, **EXTRA_VARIANTS)


def geometry(geo, fmt, out):
    """(source size, output size, resize) of a family case. The sizes are the smallest test_gpu_parity has shown the
    family to accept; packed formats get narrower sources where a 640-pixel row of 3- or 4-byte pixels is past what a
    strip or a staged tile may stage (1 KB per row segment). Planar fp32 cases take an output width that is not a
    multiple of 4 where the family has a variant for it."""
    odd = out == "f32"
    if geo == "rows":  # a > 15x letterboxed downscale
        return (1178, 566), (38 if odd else 40, 40), "aspect-ratio"
    if geo == "up":
        return (120, 64), (198 if odd else 200, 160), "no-aspect-ratio"
    if geo == "band":  # 3:2 across (the six-column lanes), 2.5x up
        return (120, 64), (80, 160), "no-aspect-ratio"
    src = {"NV12": (640, 360), "I420": (640, 360), "BGRX": (160, 90), "BGR": (240, 136)}[fmt]
    if geo == "down2" and fmt in ("NV12", "I420"):
        src = (320, 180)  # a 128-column strip's rows stay under the 512 B a paired tap takes
    if geo == "down2_packed":
        src = (96, 180)  # ... and those of 4-byte pixels: 1:1 across, 96 columns x 4 B
    return src, (94 if odd and geo == "down" else 96, 96), "no-aspect-ratio"


def unsupported(variant, fmt, out):
    """Why the family has no instantiation for the combination (None: it has one)."""
    family = VARIANTS_ALL[variant][0]
    if family == "STRIP" and fmt == "BGR":
        return "the strip kernel is built for NV12, I420 and BGRX"
    if family == "BAND" and fmt in ("BGRX", "BGR"):
        return "the band kernel is built for NV12 and I420"
    if out == "nhwc_u8" and family in ("ROWS", "STAGED", "STRIP"):
        return f"interleaved u8 output is not built for the {family.lower()} kernel"
    if out == "f16" and family in ("ROWS", "STAGED", "BAND"):
        return f"16-bit output is not built for the {family.lower()} kernel"
    return None


def family_cases():
    cases = []
    for variant in VARIANTS:
        for fmt in FORMATS:
            for out in OUTPUTS:
                why = unsupported(variant, fmt, out)
                cases.append(pytest.param(variant, fmt, out, id=f"{variant}-{fmt}-{out}",
                                          marks=[pytest.mark.skip(reason=why)] if why else []))
    for variant, fmt, out in EXTRA:
        assert unsupported(variant, fmt, out) is None
        cases.append(pytest.param(variant, fmt, out, id=f"{variant}-{fmt}-{out}"))
    return cases


def make_out(torch, out, shape, gpu):
    if out == "f16":
        return half_full(torch, shape, "f16", gpu)
    t = torch.empty(shape, dtype=torch.float32 if out in ("f32", "nhwc_f32") else torch.uint8, device=gpu,
                    memory_format=torch.channels_last if out.startswith("nhwc") else torch.contiguous_format)
    t.fill_(7)
    return t


def compare(torch, out, got, ref, what):
    """``got`` (device tensor, logical NCHW) against the oracle's ``ref`` bit for bit; 16-bit output against the fp32
    reference narrowed once (tests/test_gpu_half.py)."""
    if out == "f16":
        same_bits(torch, got, narrow_bits(torch, ref, "f16"), what)
    else:
        assert_same(got.cpu().numpy(), ref, what)


@pytest.mark.parametrize("variant,fmt,out", family_cases())
def test_family_layouts(evam, O, coracle, gpu, variant, fmt, out, monkeypatch):
    """One launch of three items of one size, item 0 compact, item 1 with unequal pitches at 16-byte bases, item 2 a
    window of a wide surface with chroma below luma; then the same launch with the items rotated, so that item 0 is
    no longer the compact one. Every slot equals the oracle, the slot past the last item keeps its value, and the
    launch ran on the family the case names."""
    import torch

    family, env, geo = VARIANTS_ALL[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (W, H), (DW, DH), resize = geometry(geo, fmt, out)
    rng = np.random.default_rng(zlib.crc32(repr((variant, fmt, out)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), W, H, pattern=p) for p in ("uniform", "gradient", "uniform")]
    imgs, hosts = SL.lay_out_all(evam, torch, O, frames, ITEM_KINDS, rng, gpu)
    rgb = (FORMATS.index(fmt) + (OUTPUTS + ["nhwc_f32"]).index(out)) % 2 == 1
    dtype = "u8" if out in ("u8", "nhwc_u8") else "f32"
    info = evam.PreProcInfo(resize=resize, placement="center", fill=(5, 50, 250), color_space="RGB" if rgb else "BGR",
                            precision="FP16" if out == "f16" else None, **(NORM if dtype == "f32" else {}))
    shape = (4, 3, DH, DW)
    ref, _ = run_oracle(O, coracle, hosts, shape, dtype, info)
    pp = evam.HipPreProcessor(device=0)  # the knobs are read when the handle is created
    try:
        for rot in (0, 1):
            order = [(i + rot) % 3 for i in range(3)]
            got = make_out(torch, out, shape, gpu)
            pp.convert([imgs[i] for i in order], got, info)
            torch.cuda.synchronize()
            what = f"{variant} {fmt} {W}x{H}->{DW}x{DH} {out} {'RGB' if rgb else 'BGR'} items {order}"
            k = pp.stats().kernels
            assert k == getattr(evam.native, "KERNEL_" + family), f"{what}: kernel family bits {k:#x}, not {family}"
            want = ref.copy()
            want[:3] = ref[order]
            assert (want[3] == 7).all()
            compare(torch, out, got, want, what)
    finally:
        pp.close()


# ---- per-item geometry ------------------------------------------------------------------------------------------
ROI_ENVS = {
    "rec_device": ("ROI", {"EVAM_PP_REC_DEVICE": "1"}),
    "rec_host": ("ROI", {"EVAM_PP_REC_DEVICE": "0"}),
    "roi_px1": ("ROI", {"EVAM_PP_ROI_PX": "1"}),
    "roi_px2": ("ROI", {"EVAM_PP_ROI_PX": "2"}),
    "roi_px4": ("ROI", {"EVAM_PP_ROI_PX": "4"}),
    "generic": ("GENERIC", {"EVAM_PP_ROI": "0"}),
}
ROI_SIZES = [(320, 240), (200, 120), (130, 74)]
ROI_KINDS = ["reversed", "window", "unequal"]


def layout_rois(rng):
    rois = []
    for k in range(24):
        si = k % 3
        W, H = ROI_SIZES[si]
        w, h = int(rng.integers(2, W)), int(rng.integers(2, H))
        x, y = int(rng.integers(-20, W - 2)), int(rng.integers(-20, H - 2))  # some partly outside the frame
        rois.append((si, x, y, max(w, 2 - x), max(h, 2 - y)))
    for si, (W, H) in enumerate(ROI_SIZES):
        rois += [(si, 0, 0, W, H), (si, int(rng.integers(0, W)), int(rng.integers(0, H)), 1, 1)]
    rois += [(0, 0, 0, 0, 0), (2, ROI_SIZES[2][0] - 3, ROI_SIZES[2][1] - 3, 10, 10)]
    return rois


@pytest.mark.parametrize("dst,dtype", [((72, 72), "f32"), ((64, 36), "u8"), ((72, 72), "f16")])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("variant", sorted(ROI_ENVS))
def test_roi_layouts(evam, O, coracle, gpu, variant, fmt, dst, dtype, monkeypatch):
    """32 ROIs (partly outside, 1 x 1, whole frames) over three sources of different sizes, each in its own layout:
    the ROI kernel with its records built on the device path and the host path and at every pixels-per-lane setting
    (fp16 too: the 2-byte instantiations at 1, 2 and 4 pixels per lane), and the generic kernel, each asserted to
    have run."""
    import torch

    family, env = ROI_ENVS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(zlib.crc32(repr(("roi", fmt, dst)).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), W, H, pattern="gradient" if i == 1 else "uniform")
              for i, (W, H) in enumerate(ROI_SIZES)]
    imgs, hosts = SL.lay_out_all(evam, torch, O, frames, ROI_KINDS, rng, gpu)
    rois = layout_rois(rng)
    info = evam.PreProcInfo(resize="aspect-ratio", placement="center", fill=(3, 60, 200), color_space="RGB",
                            precision="FP16" if dtype == "f16" else None, **(NORM if dtype != "u8" else {}))
    n = len(rois)
    shape = (n + 1, 3, dst[1], dst[0])
    ref, _ = run_oracle(O, coracle, hosts, shape, "u8" if dtype == "u8" else "f32", info, rois=rois)
    got = make_out(torch, dtype, shape, gpu)
    pp = evam.HipPreProcessor(device=0)
    try:
        pp.convert(imgs, got, info, rois=[evam.Roi(*r) for r in rois])
        torch.cuda.synchronize()
        k = pp.stats().kernels
    finally:
        pp.close()
    what = f"roi layouts {variant} {fmt} -> {dst} {dtype}"
    assert k == getattr(evam.native, "KERNEL_" + family), f"{what}: kernel family bits {k:#x}, not {family}"
    assert (ref[n] == 7).all()
    compare(torch, dtype, got, ref, what)


# ---- the default planner ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,n,family", [("c2", 8, "STRIP"), ("c4", 8, "STRIP"), ("c1_i420", 8, "BAND"),
                                             ("c5_bgrx", 8, "STRIP")])
def test_default_planner_layouts(evam, O, coracle, gpu, config, n, family):
    """bench.py's geometries with no knob set, at 8 items: three frames in three layouts repeated over the launch
    (as test_gpu_plans.test_bench_plans repeats its frames), the family the default planner picks for the config, every
    slot against the oracle, and for the clip-ring config the slots the step does not write."""
    import torch

    wl = bench.WORKLOADS[config]
    K = 3
    W, H = wl["src"]
    DW, DH = wl["dst"]
    dtype = wl["dtype"]
    ring = wl.get("ring")
    rng = np.random.default_rng(zlib.crc32(f"planner{config}".encode()))
    fourcc = evam.preproc.FOURCC_BY_NAME[wl["fourcc"]]
    frames = [O.random_frame(rng, fourcc, W, H) for _ in range(K)]
    imgs, hosts = SL.lay_out_all(evam, torch, O, frames, ITEM_KINDS, rng, gpu)
    info = bench.make_info(evam, wl)
    ref, _ = run_oracle(O, coracle, hosts, (K, 3, DH, DW), dtype, info, init=0)
    ref_dev = torch.from_numpy(ref).to(gpu)
    idx = (torch.arange(n, device=gpu) + 1) % K  # item 0 is not the compact frame
    batch = [imgs[int(i)] for i in idx.cpu()]
    out = torch.full((n * (ring or 1), 3, DH, DW), 7, dtype=torch.float32 if dtype == "f32" else torch.uint8,
                     device=gpu)
    t = 3
    pp = evam.HipPreProcessor(device=0)
    try:
        pp.convert(batch, out, info, **({"slot_offset": t % ring, "slot_stride": ring} if ring else {}))
        torch.cuda.synchronize()
        k = pp.stats().kernels
    finally:
        pp.close()
    what = f"{config} x {n}, layouts {ITEM_KINDS}"
    assert k == getattr(evam.native, "KERNEL_" + family), (what, k)
    if ring:
        rv = out.view(n, ring, 3, DH, DW)
        expect_items(torch, rv[:, t % ring], ref_dev, idx, ref, what)
        assert all_seven(torch, rv[:, :t % ring]) and all_seven(torch, rv[:, t % ring + 1:]), what
    else:
        expect_items(torch, out, ref_dev, idx, ref, what)


# ---- random calls -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout_pp(evam, gpu):
    """One handle for every random case (the pattern of test_gpu_parity's fuzz_pp)."""
    pp = evam.HipPreProcessor(device=0)
    yield pp
    pp.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("EVAM_FUZZ_LAYOUT_CASES", "48"))))
def test_random_layout_calls(evam, O, coracle, gpu, layout_pp, seed):
    """test_gpu_parity's random_case, unchanged, with every frame laid out again in a kind drawn from a second
    generator: any format, size, geometry, ROI list and slot pattern the boundary accepts, over mixed layouts."""
    import torch

    fmt, frames, shape, dtype, info, rois, offset, stride = random_case(evam, O, np.random.default_rng(7000 + seed))
    rng2 = np.random.default_rng(17000 + seed)
    kinds = [SL.KINDS[int(rng2.integers(0, len(SL.KINDS)))] for _ in frames]
    pairs = [SL.lay_out(evam, torch, O, f, k, rng2, gpu) for f, k in zip(frames, kinds)]
    imgs, hosts = [a for a, _ in pairs], [b for _, b in pairs]
    what = f"seed {seed}: {fmt} {[(f.width, f.height) for f in frames]} {kinds} -> {shape} {dtype} {info} " \
           f"{'%d rois' % len(rois) if rois else 'frames'} offset {offset} stride {stride}"
    got = torch.full(shape, 7, dtype=torch.float32 if dtype == "f32" else torch.uint8, device=gpu)
    layout_pp.convert(imgs, got, info, rois=[evam.Roi(*r) for r in rois] if rois else None, slot_offset=offset,
                      slot_stride=stride)
    torch.cuda.synchronize()
    ref, _ = run_oracle(O, coracle, hosts, shape, dtype, info, rois=rois, slot_offset=offset, slot_stride=stride)
    assert_same(got.cpu().numpy(), ref, what)


# ---- JPEG -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpeg_pp(evam, gpu):
    pp = evam.HipPreProcessor(device=0)
    yield pp
    pp.close()


@pytest.mark.parametrize("size", [(50, 34), (200, 120)])
@pytest.mark.parametrize("kind", ["unequal+base16", "window"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_jpeg_layouts(evam, O, gpu, jpeg_pp, fmt, kind, size):
    """encode_jpeg of one laid-out frame (noise at 95, a gradient at 75, both unequal sub-variants): whole files
    against tests/jpeg_ref.py."""
    import torch

    w, h = size
    rng = np.random.default_rng(zlib.crc32(repr(("jpeg", fmt, kind, size)).encode()))
    for variant, (pattern, quality) in enumerate((("uniform", 95), ("gradient", 75))):
        frame = O.random_frame(rng, fc(O, fmt), w, h, pattern=pattern)
        img, host = SL.lay_out(evam, torch, O, frame, kind, rng, gpu, variant=variant)
        jpeg_check(evam, O, gpu, jpeg_pp, [host], quality, f"{fmt} {w}x{h} {kind} {pattern}", imgs=[img])
