"""The plans the default planner picks as item counts and crop widths grow, bit-exact vs the C oracle.

The host planner (plan_strip / plan_band / plan_roi in csrc/evam_plan.h) turns a call's item count, output size and
widest crop into a tile height, a wave count, an LDS carve and sometimes another kernel family. That a plan is
well-formed (every bound its kernel relies on) and what the benchmark's plans are is checked on the CPU, on a fake
kernel backend (tests/native/planner_check.cpp: check_plans, check_pinned_plans; tests/test_native_asan.py). What only
the GPU shows is that the kernels compute bit-exact output under each plan, and ``evam_pp_stats.kernels`` reports only
the family: these tests make the planner produce each plan by issuing the call a real batch would issue, with no
EVAM_PP_* knob set, and compare every output element with the oracle.

A plan depends on the format, the geometry, the output dtype, the item count, the CU count, the crop origins and
(I420) the plane distance, not on whether the items are distinct frames. So a launch of n items repeats K = 2 or 3
distinct frames, the oracle runs on those K only, and the comparison happens on the device: the K oracle slots are
uploaded once and indexed with ``arange(n) % K``. Only a mismatch copies anything back, to name the first differing
element.

Tile heights quoted in the docstrings follow plan_strip's arithmetic, TH = ceil(min(n, 64) * tiles_x * DH /
(n_cu * res)) clamped to [2, min(DH, 64)], on 256 CUs with res = min(16 / nw, the workgroups of 4 waves the kernel's
registers and LDS let a CU hold: at most 8) per CU; they describe what the sweep is for, and are not asserted (the ABI
does not export the plan). Outputs stay under 256 MB: a u8 geometry
can reach the 64-row clamp inside that; an fp32 one of four or more strips cannot (it needs at least 384 x 512 x 12 B
x 150 items), so those fp32 sweeps run smaller outputs and stop at the tile height their docstring names, and only the
one-strip geometry of test_sweep_strip_narrow walks every height in fp32.
"""
import zlib

import numpy as np
import pytest

import bench
from test_gpu_fullsize import host_frames, oracle_items
from test_gpu_parity import assert_same, fc, run_oracle, upload

pytestmark = pytest.mark.gpu

NORM = {"range": (0.0, 1.0), "mean": (0.406, 0.456, 0.485), "std": (0.225, 0.224, 0.229)}
COUNTS = list(range(1, 67)) + [70, 127, 128, 129, 150]
MAX_OUT_BYTES = 256_000_000


def tdtype(torch, dtype):
    return torch.float32 if dtype == "f32" else torch.uint8


def make_info(evam, dtype, **kw):
    return evam.PreProcInfo(**kw, **(NORM if dtype == "f32" else {}))


def bits(torch, t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def expect_items(torch, got, ref_dev, idx, ref, what):
    """got[i] == ref_dev[idx[i]] for every item i, compared on the device; ``ref`` is the host copy of ``ref_dev``,
    read only to report the first differing element."""
    want = ref_dev[idx]
    a, b = bits(torch, got), bits(torch, want)
    if torch.equal(a, b):
        return
    i = int((a != b).flatten(1).any(1).nonzero()[0])
    assert_same(got[i].cpu().numpy(), ref[int(idx[i])], f"{what}: item {i}")
    raise AssertionError(f"{what}: item {i} differs on the device but not on the host")


def all_seven(torch, t):
    return bool((t == 7).all().item())


# ------------------------------------------------------------------------------------------------------------------
# 1. The bench's own plans
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,n,family", [
    ("c4", 64, "STRIP"), ("c4", 32, "STRIP"), ("c4", 16, "STRIP"), ("c4", 8, "STRIP"),
    ("c2_i420", 32, "STRIP"), ("c1_i420", 32, "BAND"), ("c5", 32, "STRIP"), ("c5_bgrx", 32, "STRIP")])
def test_bench_plans(evam, O, coracle, gpu, config, n, family):
    """bench.py's reported lines at the item counts bench.py launches them with (C4: one rank's share of 64 streams at
    1, 2, 4 and 8 GPUs; 64 items is 5 unpaired strips at a tile height in the fifties), on bench.device_frames
    frames: the family the default planner picks, every slot against the oracle, and for the clip-ring configs the 15
    slots per stream the step does not write."""
    import torch

    wl = bench.WORKLOADS[config]
    K = 2
    imgs = bench.device_frames(evam, torch, wl, K, gpu, seed=1234)
    frames = host_frames(O, imgs)
    batch = [imgs[i % K] for i in range(n)]
    DW, DH = wl["dst"]
    dtype = wl["dtype"]
    ring = wl.get("ring")
    idx = torch.arange(n, device=gpu) % K
    pp = evam.HipPreProcessor(device=0)
    try:
        for placement in (("top_left", "center") if config == "c4" else ("top_left",)):
            info = bench.make_info(evam, wl)
            info.placement = placement
            ref = oracle_items(O, coracle, frames, [(k, 0, 0, 0, 0) for k in range(K)], (K, 3, DH, DW), dtype, info)
            ref_dev = torch.from_numpy(ref).to(gpu)
            out = torch.full((n * (ring or 1), 3, DH, DW), 7, dtype=tdtype(torch, dtype), device=gpu)
            t = 3
            xf = pp.convert(batch, out, info, want_transform=True, **({"slot_offset": t % ring, "slot_stride": ring}
                                                                      if ring else {}))
            torch.cuda.synchronize()
            assert pp.stats().kernels == getattr(evam.native, "KERNEL_" + family), (config, n, pp.stats().kernels)
            if config == "c4":
                for x in (xf[0], xf[-1]):
                    assert (x.resized_w, x.resized_h, x.pad_y) == (640, 360, 140 if placement == "center" else 0)
            what = f"{config} x {n} {placement}"
            if ring:
                rv = out.view(n, ring, 3, DH, DW)
                expect_items(torch, rv[:, t % ring], ref_dev, idx, ref, what)
                assert all_seven(torch, rv[:, :t % ring]) and all_seven(torch, rv[:, t % ring + 1:]), what
            else:
                expect_items(torch, out, ref_dev, idx, ref, what)
            del out, ref_dev
    finally:
        pp.close()


# ------------------------------------------------------------------------------------------------------------------
# 2. Item-count sweeps on uniform geometry
# ------------------------------------------------------------------------------------------------------------------
def sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, families, rois=None, **info_kw):
    """One handle, one launch per count in COUNTS of ``fmt`` frames ``src`` -> ``dst`` (K = 3 distinct frames
    repeated, or the distinct ``rois`` repeated), each into its own n + 1 slot tensor initialised to 7: slots 0..n-1
    equal the repeated oracle slots, slot n keeps 7. Every launch's family is one of ``families``; returns
    {count: family bit}."""
    import torch

    N = evam.native
    (W, H), (DW, DH) = src, dst
    assert (max(COUNTS) + 1) * 3 * DW * DH * (4 if dtype == "f32" else 1) < MAX_OUT_BYTES
    rng = np.random.default_rng(zlib.crc32(repr((fmt, src, dst, dtype, sorted(info_kw.items()))).encode()))
    frames = [O.random_frame(rng, fc(O, fmt), W, H, pattern=p) for p in ("uniform", "gradient", "uniform")]
    imgs = upload(evam, frames, gpu)
    info = make_info(evam, dtype, **info_kw)
    period = len(rois) if rois else len(frames)
    ref, _ = run_oracle(O, coracle, frames, (period, 3, DH, DW), dtype, info, rois=rois)
    ref_dev = torch.from_numpy(ref).to(gpu)
    allowed = {getattr(N, "KERNEL_" + f) for f in families}
    got_family = {}
    pp = evam.HipPreProcessor(device=0)
    try:
        for n in COUNTS:
            out = torch.full((n + 1, 3, DH, DW), 7, dtype=tdtype(torch, dtype), device=gpu)
            if rois:
                items = np.array([rois[i % period] for i in range(n)], np.int32)
                pp.convert(imgs, out, info, rois=evam.RoiBatch(items))
            else:
                pp.convert([imgs[i % period] for i in range(n)], out, info)
            k = pp.stats().kernels
            what = f"{fmt} {src}->{dst} {dtype} {info_kw} x {n}"
            assert k in allowed, f"{what}: kernel family bits {k:#x}, expected one of {sorted(families)}"
            got_family[n] = k
            expect_items(torch, out[:n], ref_dev, torch.arange(n, device=gpu) % period, ref, what)
            assert all_seven(torch, out[n]), f"{what}: the slot past the last item was written"
            del out
    finally:
        pp.close()
    return got_family


@pytest.mark.parametrize("fmt,src,dst,dtype", [
    ("NV12", (1200, 2400), (512, 1024), "u8"), ("I420", (1200, 2400), (512, 1024), "u8"),
    ("BGRX", (480, 2100), (256, 1024), "u8"),
    ("NV12", (1200, 640), (512, 272), "f32"), ("I420", (1200, 640), (512, 272), "f32"),
    ("BGRX", (480, 1116), (256, 544), "f32")])
def test_sweep_strip_four_strips(evam, O, coracle, gpu, fmt, src, dst, dtype):
    """Strip, 4 strips: one workgroup of 4 waves per tile row (nw = 4, tiles_x = 1), paired taps, a 2.34x downscale
    (BGRx: 1.875x across, so that a 64-column strip of 4-byte pixels stays under 512 B, and 2.05x down: at 1.875x one
    output row in 8 shares a source row with the next, which is where plan_strip hands over to the wave kernel). u8:
    DH = 1024, so TH = min(n, 64): the sweep visits every tile height 2..64 and stays at the 64-row clamp (a full
    lane-held row table) from 64 items on, in three launches at 129 and 150. fp32: TH up to 17 (BGRx: 34)."""
    sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["STRIP"])


@pytest.mark.parametrize("fmt,src,dst,dtype", [
    ("NV12", (3520, 1616), (640, 800), "u8"), ("I420", (3520, 1616), (640, 800), "u8"),
    ("NV12", (3520, 436), (640, 216), "f32"), ("I420", (3520, 436), (640, 216), "f32")])
def test_sweep_strip_unpaired(evam, O, coracle, gpu, fmt, src, dst, dtype):
    """Strip, unpaired: DW = 640 at a 5.5x horizontal downscale, the C4 shape at a fraction of its source size: five
    128-column strips (nw = 5, 3 workgroups per CU) whose ~704-byte footprints are over the 512 B a paired tap takes,
    so one source row per DMA instruction (BGRx footprints at this scale are over the 1 KB a strip may stage: the strip
    kernel does not take them). NV12 u8: TH = ceil(min(n, 64) * 800 / 768), every height 2..64, the clamp from 62
    items on; I420 stages two chroma planes, its 60 KB of LDS leave 2 workgroups per CU: TH = ceil(n * 800 / 512), the
    clamp from 41 items on. fp32: TH up to 18 (I420: 27)."""
    sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["STRIP"])


@pytest.mark.parametrize("placement", ["top_left", "center"])
@pytest.mark.parametrize("fmt,src,dst,dtype", [
    ("NV12", (1200, 1804), (512, 1024), "u8"), ("I420", (1200, 1804), (512, 1024), "u8"),
    ("BGRX", (564, 1695), (256, 1024), "u8"), ("NV12", (1280, 528), (512, 273), "f32")])
def test_sweep_strip_letterbox(evam, O, coracle, gpu, fmt, src, dst, dtype, placement):
    """Strip, letterbox, both placements: padding rows make tile rows straddle the padding / image boundary at
    every tile height. u8: 1200x1804 -> 512x769 (BGRx: 564x1695 -> 256x769) image rows (769 is prime) in 1024: centred,
    the image starts at row 127 (prime, coprime to every TH in 2..64) and ends at 896; top-left, it ends at row 769.
    TH = min(n, 64), 2..64. fp32: 1280x528 -> 512x211 in 273 rows, the image at rows 31..241 (centred) or 0..210; TH up to 18."""
    sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["STRIP"], resize="aspect-ratio", placement=placement,
                 fill=(114, 17, 201))


@pytest.mark.parametrize("fmt,src,dst,dtype", [
    ("NV12", (1600, 2400), (224, 1024), "u8"), ("I420", (1600, 2400), (224, 1024), "u8"),
    ("BGRX", (768, 1976), (224, 1024), "u8"),
    ("NV12", (1600, 1462), (224, 624), "f32"), ("BGRX", (768, 1204), (224, 624), "f32")])
def test_sweep_strip_central_crop(evam, O, coracle, gpu, fmt, src, dst, dtype):
    """Strip, central crop: aspect-ratio(max) + central crop, the C5 shape (four 64-column strips, the resized image
    wider than the output: ox = -229 for the 1600-wide sources, -86 for BGRx), stretched vertically so the count
    sweep walks the tile height. u8: TH = min(n, 64), 2..64 and the clamp. fp32: TH up to 39."""
    sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["STRIP"], resize="aspect-ratio", crop="central")


@pytest.mark.parametrize("fmt,src,dst,dtype", [
    ("NV12", (120, 4100), (50, 2048), "u8"), ("I420", (120, 4100), (50, 2048), "f32"),    # nw = 1
    ("NV12", (240, 4100), (100, 2048), "u8"), ("BGRX", (180, 4100), (100, 2048), "u8"),   # nw = 2
    ("I420", (456, 2562), (190, 1280), "u8"), ("NV12", (456, 1482), (190, 740), "f32")])  # nw = 3
def test_sweep_strip_narrow(evam, O, coracle, gpu, fmt, src, dst, dtype):
    """Strip, narrow: outputs of 1, 2 and 3 strips (nw = 1, 2, 3: 8, 8 and 5 workgroups per CU), tall enough that
    the sweep still walks the tile height: 50 x 2048 (u8 and fp32, the one fp32 geometry small enough to get there),
    100 x 2048 and 190 x 1280 u8 run TH = min(n, 64), every height 2..64 and the clamp; 190 x 740 fp32 up to TH 37."""
    sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["STRIP"])


@pytest.mark.parametrize("fmt,src,dst,dtype", [
    ("NV12", (2660, 900), (1152, 384), "u8"), ("I420", (2660, 282), (1152, 120), "f32"),   # 9 strips
    ("NV12", (5000, 600), (2176, 256), "u8"), ("I420", (5000, 600), (2176, 256), "u8"),    # 17 strips
    ("BGRX", (2200, 600), (1280, 256), "u8")])                                             # 10 strips
def test_sweep_strip_wide(evam, O, coracle, gpu, fmt, src, dst, dtype):
    """Strip, wide: more than 8 strips, so a tile row is several workgroups (tiles_x >= 2). 1152 columns: 9
    128-column strips in 2 workgroups of 5 waves (one idle), TH = ceil(min(n, 64) * 2 * 384 / 768) = min(n, 64) in u8,
    up to 20 in fp32. 2176 columns: 17 strips in 3 workgroups of 6 (one idle wave), TH = ceil(min(n, 64) * 3 * 256 /
    512), the clamp from 43 items on. BGRx 1280 columns at 1.72x: ten 128-column strips of ~880 B, 2 workgroups of 5, TH
    up to 43."""
    sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["STRIP"])


@pytest.mark.parametrize("fmt,dtype", [("NV12", "u8"), ("I420", "u8"), ("BGRX", "u8"), ("NV12", "f32")])
def test_sweep_strip_varied_crop_origins(evam, O, coracle, gpu, fmt, dtype):
    """Strip, varied crop origins: a uniform group of equal-size ROIs (600 x 2400 crops, BGRx 480 x 2400, fp32 600 x
    1280) at 16 crop origins between 0 and 63 covering 16 x0 mod 32 residues (the test_uniform_rois_varied_x0
    construction, as rois=): the strip footprints are bounded over every origin in x0_mask, at every tile height the
    count sweep reaches (u8: 256 x 1024, TH = min(n, 64); fp32: 256 x 544, TH up to 34)."""
    yuv = fmt != "BGRX"
    ch, dh = (2400, 1024) if dtype == "u8" else (1280, 544)
    if fmt == "BGRX":  # 4-byte pixels: a 64-column strip stays under 1 KB up to a 4x downscale
        cw, W = 480, 560
    else:
        cw, W = 600, 672
    xs = [2 * k + (32 if k % 2 else 0) + (0 if yuv else 1) for k in range(16)]  # 4:2:0 origins stay on even x
    rois = [(k % 3, x, (7 * k) % 40 & ~1, cw, ch) for k, x in enumerate(xs)]
    sweep_counts(evam, O, coracle, gpu, fmt, (W, ch + 40), (256, dh), dtype, ["STRIP"], rois=rois)


@pytest.mark.parametrize("fmt", ["NV12", "I420"])
@pytest.mark.parametrize("src,dst,resize,dtype", [
    ((320, 120), (512, 512), "aspect-ratio", "u8"),      # letterbox rows: 512 x 192 image rows at 160..351
    ((480, 270), (320, 320), "no-aspect-ratio", "f32"),  # 3:2 horizontal: six-column lanes
    ((390, 1366), (260, 2048), "no-aspect-ratio", "u8"),  # 2 strips x 2048 rows: the band kernel's 64-row clamp
])
def test_sweep_band_wave_switch(evam, O, coracle, gpu, fmt, src, dst, resize, dtype):
    """Band / wave: vertical upscales, where plan_band sends launches of at most 16 * n_cu band rows (items x strips
    x DH) to the wave kernel and larger ones to the band kernel with th = band rows / (16 * n_cu), lowered until the
    band's source rows fit the LDS. Every launch runs on one of the two, both occur in the sweep, and once a count
    runs on the band kernel every larger one does. Three geometries: a 1.6x letterbox with padding rows above and
    below (2 strips x 512 rows: the switch is expected above 4 items on 256 CUs, th up to 16), a 3:2 horizontal
    downscale whose lanes read six source columns (fp32, 2 strips x 320 rows: above 6 items, th up to 10), and 260 x
    2048 u8, two strips (the second 4 columns wide) of 2048 rows under the 256 MB cap, whose th = n reaches the band
    kernel's 64-row clamp at 64 items."""
    N = evam.native
    fam = sweep_counts(evam, O, coracle, gpu, fmt, src, dst, dtype, ["WAVE", "BAND"], resize=resize,
                       placement="center", fill=(5, 50, 250))
    band = [n for n in COUNTS if fam[n] == N.KERNEL_BAND]
    assert band and len(band) < len(COUNTS), f"both families must occur: band at {band}"
    assert band == [n for n in COUNTS if n >= band[0]], f"band kernel at {band}: not every count from the first on"
    print(f"band/wave switch {fmt} {src}->{dst}: wave up to {band[0] - 1} items, band from {band[0]}")


# ------------------------------------------------------------------------------------------------------------------
# 3. ROI-count and crop-width sweeps
# ------------------------------------------------------------------------------------------------------------------
def n_cu_of(gpu):
    import torch

    return torch.cuda.get_device_properties(gpu).multi_processor_count


def roi_counts(n_cu):
    return [n_cu - 1, n_cu, n_cu + 1, 2 * n_cu + 1, 3 * n_cu - 1, 4 * n_cu + 7, 5 * n_cu + n_cu // 2, 6 * n_cu + 1,
            7 * n_cu, 7 * n_cu + 1, 8 * n_cu + 3, 16 * n_cu + 5]


ROI_W, ROI_H = 320, 240


def seeded_rois(n):
    """The first n of one seeded ROI list over 3 frames of 320x240: any prefix of a longer list is the shorter list.
    Rects reach up to 24 pixels outside the frame; every 41st item is a whole frame."""
    rng = np.random.default_rng(20261)
    rois = []
    for k in range(n):
        si = int(rng.integers(0, 3))
        w, h = int(rng.integers(2, 300)), int(rng.integers(2, 220))
        x, y = int(rng.integers(-24, ROI_W - 2)), int(rng.integers(-24, ROI_H - 2))
        rois.append((si, 0, 0, 0, 0) if k % 41 == 17 else (si, x, y, max(w, 2 - x), max(h, 2 - y)))
    return rois


@pytest.mark.parametrize("dst,dtype", [((48, 40), "f32"), ((48, 40), "u8"), ((72, 72), "f32"), ((72, 72), "u8")])
@pytest.mark.parametrize("fmt", ["NV12", "BGRX", "I420", "BGR"])
def test_roi_count_sweep(evam, O, coracle, gpu, fmt, dst, dtype):
    """ROI counts: plan_roi's carve for per_cu = ceil(n / n_cu) = 1..7 resident workgroups per CU, and counts past the
    resident slots (n > 7 * n_cu: roi_tail_tiles' `fit` goes non-positive and a second round of workgroups starts), at
    n_cu - 1, n_cu, n_cu + 1, 2 n_cu + 1, 3 n_cu - 1, 4 n_cu + 7, 5.5 n_cu, 6 n_cu + 1, 7 n_cu, 7 n_cu + 1, 8 n_cu + 3
    and 16 n_cu + 5 ROIs (72 x 72: up to 7 n_cu). NV12 and BGRx at every count; I420 and BGR at 2 n_cu + 1, 7 n_cu and
    8 n_cu + 3. Every launch runs on the ROI kernel and every item equals the oracle, which runs once over the
    longest list (each count's set is a prefix of it)."""
    import torch

    n_cu = n_cu_of(gpu)
    counts = roi_counts(n_cu) if fmt in ("NV12", "BGRX") else [2 * n_cu + 1, 7 * n_cu, 8 * n_cu + 3]
    if dst == (72, 72):
        counts = [n for n in counts if n <= 7 * n_cu]
    DW, DH = dst
    rng = np.random.default_rng(zlib.crc32(f"roicount{fmt}".encode()))
    frames = [O.random_frame(rng, fc(O, fmt), ROI_W, ROI_H, pattern="gradient" if i == 1 else "uniform")
              for i in range(3)]
    imgs = upload(evam, frames, gpu)
    rois = seeded_rois(max(counts))
    arr = np.array(rois, np.int32)
    info = make_info(evam, dtype, resize="aspect-ratio", placement="center", fill=(3, 60, 200), color_space="RGB")
    ref, _ = run_oracle(O, coracle, frames, (len(rois), 3, DH, DW), dtype, info, rois=rois)
    ref_dev = torch.from_numpy(ref).to(gpu)
    pp = evam.HipPreProcessor(device=0)
    try:
        for n in counts:
            out = torch.full((n + 1, 3, DH, DW), 7, dtype=tdtype(torch, dtype), device=gpu)
            pp.convert(imgs, out, info, rois=evam.RoiBatch(arr[:n]))
            what = f"{n} ROIs ({n / n_cu:.2f} per CU) {fmt} -> {dst} {dtype}"
            assert pp.stats().kernels == evam.native.KERNEL_ROI, (what, pp.stats().kernels)
            expect_items(torch, out[:n], ref_dev, torch.arange(n, device=gpu), ref, what)
            assert all_seven(torch, out[n]), f"{what}: the slot past the last item was written"
            del out
    finally:
        pp.close()


# very wide, 12..16 rows high sources: (frame 0 width, frame 1 width); a crop's two source rows fill the 32 KB the ROI
# kernel stages at most at about 8,160 (NV12 / I420), 5,450 (BGR) and 4,090 (BGRx) pixels
WIDE_SRC = {"NV12": (8400, 8200), "I420": (8400, 8200), "BGR": (5600, 5400), "BGRX": (4300, 4200)}
WIDTH_STEPS = 12


def width_rois(fmt, step):
    """A 20-ROI batch on the two wide frames whose widest crop (item 0) grows with ``step`` from 1,000 pixels to the
    whole width of frame 0; the other 19 do not depend on the step: narrow and medium crops on both frames, one
    reaching outside."""
    W0, W1 = WIDE_SRC[fmt]
    even = fmt in ("NV12", "I420")
    w = 1000 + (W0 - 1000) * step // (WIDTH_STEPS - 1)
    if even:
        w &= ~1
    x = (W0 - w) // 2 & ~1
    rng = np.random.default_rng(zlib.crc32(f"widths{fmt}".encode()))
    rois = [(0, x, 0, w, 16)]
    for k in range(19):
        si = k % 2
        Wk, Hk = (W0, 16) if si == 0 else (W1, 12)
        cw = int(rng.integers(8, 300)) if k % 3 else int(rng.integers(300, 1000))
        chh = int(rng.integers(2, Hk + 1))
        rois.append((si, int(rng.integers(0, Wk - cw)), int(rng.integers(0, Hk - chh + 1)), cw, chh))
    rois[7] = (1, W1 - 100, 6, 400, 20)  # partly outside
    return rois, w


def width_frames(O, fmt):
    rng = np.random.default_rng(zlib.crc32(f"wide{fmt}".encode()))
    W0, W1 = WIDE_SRC[fmt]
    return [O.random_frame(rng, fc(O, fmt), W0, 16, pattern="uniform"),
            O.random_frame(rng, fc(O, fmt), W1, 12, pattern="gradient")]


@pytest.mark.parametrize("dst,dtype", [((72, 72), "f32"), ((300, 24), "u8")])
@pytest.mark.parametrize("fmt", ["NV12", "I420", "BGR", "BGRX"])
def test_roi_width_sweep(evam, O, coracle, gpu, fmt, dst, dtype):
    """Crop widths: plan_roi raises the staging buffer to row_bytes_bound(widest crop), so from about 3,000 (NV12 /
    I420), 2,000 (BGR) and 1,500 (BGRx) pixels one source row pair's segments fill the whole buffer (one output row per
    group), and past 32 KB the group goes to the generic kernel. A 20-ROI batch over two wide frames of different
    sizes, its widest crop swept in 12 steps from 1,000 pixels to the frame width, with narrow crops in the same launch
    (several rows per group for them); 72 x 72 and a DW > 256 target. Every launch runs on the ROI or the generic
    kernel, both occur, and the generic launches are exactly the widest ones."""
    import torch

    N = evam.native
    frames = width_frames(O, fmt)
    imgs = upload(evam, frames, gpu)
    DW, DH = dst
    info = make_info(evam, dtype, color_space="RGB")
    fam, widths = [], []
    pp = evam.HipPreProcessor(device=0)
    try:
        for step in range(WIDTH_STEPS):
            rois, w = width_rois(fmt, step)
            n = len(rois)
            ref, _ = run_oracle(O, coracle, frames, (n, 3, DH, DW), dtype, info, rois=rois)
            out = torch.full((n + 1, 3, DH, DW), 7, dtype=tdtype(torch, dtype), device=gpu)
            pp.convert(imgs, out, info, rois=[evam.Roi(*r) for r in rois])
            k = pp.stats().kernels
            what = f"widest crop {w} {fmt} -> {dst} {dtype}"
            assert k in (N.KERNEL_ROI, N.KERNEL_GENERIC), (what, k)
            fam.append(k)
            widths.append(w)
            expect_items(torch, out[:n], torch.from_numpy(ref).to(gpu), torch.arange(n, device=gpu), ref, what)
            assert all_seven(torch, out[n]), f"{what}: the slot past the last item was written"
    finally:
        pp.close()
    generic = [w for w, k in zip(widths, fam) if k == N.KERNEL_GENERIC]
    assert generic and len(generic) < WIDTH_STEPS, f"both kernels must occur: generic at {generic} of {widths}"
    assert generic == widths[-len(generic):], f"generic at {generic}: not exactly the widest of {widths}"
    print(f"ROI/generic switch {fmt} -> {dst}: ROI kernel up to {widths[-len(generic) - 1]} pixels, generic from "
          f"{generic[0]}")


@pytest.mark.parametrize("fmt", ["NV12", "I420", "BGR", "BGRX"])
def test_roi_width_steps_many_rois(evam, O, coracle, gpu, fmt):
    """Three of the width steps (4, 9 and 10 of 0..11: the two widest still on the ROI kernel, and one in the middle)
    at 2 n_cu + 1 ROIs, the batch filled up with copies of its narrow crops: plan_roi wants 3 workgroups per CU, the
    wide crop's buffer allows fewer, so the launch runs past its resident slots with a staging buffer a single source
    row pair fills. The copies' oracle slots are those of the 20 distinct ROIs."""
    import torch

    N = evam.native
    n = 2 * n_cu_of(gpu) + 1
    frames = width_frames(O, fmt)
    imgs = upload(evam, frames, gpu)
    DW, DH = 72, 72
    info = make_info(evam, "f32", color_space="RGB")
    pp = evam.HipPreProcessor(device=0)
    try:
        for step in (4, 9, 10):
            base, w = width_rois(fmt, step)
            src_of = list(range(20)) + [1 + k % 19 for k in range(n - 20)]
            ref, _ = run_oracle(O, coracle, frames, (20, 3, DH, DW), "f32", info, rois=base)
            out = torch.full((n + 1, 3, DH, DW), 7, dtype=torch.float32, device=gpu)
            pp.convert(imgs, out, info, rois=evam.RoiBatch(np.array([base[j] for j in src_of], np.int32)))
            what = f"widest crop {w} of {n} ROIs {fmt}"
            assert pp.stats().kernels == N.KERNEL_ROI, (what, pp.stats().kernels)
            expect_items(torch, out[:n], torch.from_numpy(ref).to(gpu), torch.tensor(src_of, device=gpu), ref, what)
            assert all_seven(torch, out[n]), f"{what}: the slot past the last item was written"
    finally:
        pp.close()
