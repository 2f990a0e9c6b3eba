"""The layout builder of tests/source_layouts.py on the CPU: every kind and format gives an Image that evam_pp_run's
source validation accepts, has the property its kind declares, holds the frame's bytes behind (pointer, pitch), keeps
the oracle's output, and ends with the guard tail the GPU tests rely on to stay in bounds."""
import ctypes
import zlib

import numpy as np
import pytest

import source_layouts as SL

FORMATS = ["NV12", "I420", "BGRX", "BGR"]
SIZES = [(2, 2), (50, 34), (130, 74)]


def fc(O, name):
    return {"NV12": O.NV12, "I420": O.I420, "BGRX": O.BGRX, "BGR": O.BGR}[name]


def read_plane(ptr, pitch, rows, row_bytes):
    """rows x row_bytes bytes read from memory at ptr with ``pitch`` bytes between rows (not through the view)."""
    raw = np.ctypeslib.as_array((ctypes.c_uint8 * (pitch * (rows - 1) + row_bytes)).from_address(ptr))
    return np.stack([raw[r * pitch:r * pitch + row_bytes] for r in range(rows)])


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", SL.KINDS)
def test_layout_kinds(evam, O, coracle, kind, fmt, size, variant):
    import torch

    W, H = size
    rng = np.random.default_rng(zlib.crc32(repr((kind, fmt, size, variant)).encode()))
    frame = O.random_frame(rng, fc(O, fmt), W, H, pitch_align=64)
    img, host = SL.lay_out(evam, torch, O, frame, kind, rng, "cpu", variant=variant)
    dims = SL.plane_dims(O, frame.fourcc, W, H)
    ptrs = [int(p.data_ptr()) for p in img.planes]
    pitches = img.pitches
    flags = set(kind.split("+"))
    assert len(img.planes) == len(dims) and (img.fourcc, img.width, img.height) == (frame.fourcc, W, H)

    # the ABI's rules (include/evam_pp.h, evam_pp_run's source validation)
    spans = []
    for (rows, rb), ptr, pitch in zip(dims, ptrs, pitches):
        assert ptr % 16 == 0 and pitch % 16 == 0 and pitch >= rb, (ptr % 16, pitch, rb)
        spans.append((ptr, ptr + pitch * (rows - 1) + rb))
    spans.sort()
    for (_, end), (begin, _) in zip(spans, spans[1:]):
        assert end <= begin, "planes overlap"
    c = img.to_c()
    assert [c.pitch[i] for i in range(len(dims))] == pitches and [c.planes[i] for i in range(len(dims))] == ptrs

    # all of it inside the one buffer, the guard tail behind every plane
    b0, b1 = int(img.buffer.data_ptr()), int(img.buffer.data_ptr()) + img.buffer.numel()
    g_off, g_size = img.guard
    assert max(pitches) <= SL.widest_pitch(O, frame.fourcc, W)
    most = SL.widest_pitch(O, frame.fourcc, W) * max(r for r, _ in dims)  # any kind's pitch, any plane's row count
    assert g_size >= most and b0 + g_off + g_size <= b1
    assert b0 <= spans[0][0] and spans[-1][1] <= b0 + g_off
    for ptr in ptrs:  # any plane read with any plane's pitch and row count stays inside
        assert ptr + most <= b1

    # the property of the kind
    if kind == "compact":
        assert pitches == [pt for _, pt in evam.plane_layout(frame.fourcc, W, H)]
        assert ptrs[0] % 256 == 0
        for p in range(1, len(dims)):
            assert ptrs[p] == ptrs[p - 1] + pitches[p - 1] * dims[p - 1][0]
    if flags & {"unequal", "reversed"} and "window" not in flags:
        assert len(set(pitches)) == len(pitches)
        if fmt == "NV12":
            assert pitches[1] > pitches[0] if variant == 0 else pitches[1] < pitches[0]
        elif fmt == "I420":
            assert pitches[2] < pitches[1] if variant == 0 else pitches[2] > pitches[1]
            assert 2 * pitches[1] != pitches[0]
        else:
            assert pitches[0] - SL.al16(dims[0][1]) in SL.PACKED_EXTRA
    if flags & {"base16", "reversed"} and "window" not in flags:
        res = [p % 256 for p in ptrs]
        assert set(res) <= set(SL.RESIDUES) and len(set(res)) == len(res), res
    if "reversed" in flags:
        assert ptrs == sorted(ptrs, reverse=True), "chroma below luma, V below U"
    elif kind != "compact":
        assert ptrs == sorted(ptrs)
    if "window" in flags:
        assert len(set(pitches)) == len(pitches)
        for p, ((rows, rb), view) in enumerate(zip(dims, img.planes)):
            assert pitches[p] >= 4 * rb and view.stride(0) == pitches[p] and view.shape[0] == rows
        step = SL.x_step(O, frame.fourcc)
        n = O.bpp(frame.fourcc) if len(dims) == 1 else 1
        # the window origin, from the view's geometry: shape[1] = surface pitch - x offset in bytes
        xbytes = [pitches[p] - img.planes[p].shape[1] for p in range(len(dims))]
        assert xbytes[0] > 0 and xbytes[0] % (step * n) == 0, (xbytes, step)
        if fmt == "NV12":
            assert xbytes[1] == xbytes[0]
        if fmt == "I420":
            assert xbytes[1] == xbytes[2] == xbytes[0] // 2

    # the frame's bytes behind (pointer, pitch), and in the host frame
    for p, ((rows, rb), ptr, pitch) in enumerate(zip(dims, ptrs, pitches)):
        want = frame.planes[p][:rows, :rb]
        assert np.array_equal(read_plane(ptr, pitch, rows, rb), want), f"plane {p}"
        assert np.array_equal(host.planes[p][:rows, :rb], want)

    # the oracle reads pixels only: the laid-out host frame gives what the compact one gives
    lut = O.np_norm_lut(3, (0.0, 1.0), (0.1, 0.2, 0.3), (0.3, 0.2, 0.1))
    a = np.zeros((1, 3, 9, 11), np.float32)
    b = np.ones((1, 3, 9, 11), np.float32)
    coracle.preprocess_item(frame, None, a, 0, mode=1, placement=1, lut=lut, fill=(1, 2, 3))
    coracle.preprocess_item(host, None, b, 0, mode=1, placement=1, lut=lut, fill=(1, 2, 3))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_padding_is_noise(evam, O):
    """Padding, gaps and the guard tail are random bytes, not zeros: a kernel that reads them cannot pass by luck."""
    import torch

    rng = np.random.default_rng(3)
    frame = O.random_frame(rng, O.I420, 50, 34)
    for kind in SL.KINDS:
        img, _ = SL.lay_out(evam, torch, O, frame, kind, rng, "cpu")
        g_off, g_size = img.guard
        tail = img.buffer[g_off:g_off + g_size].numpy()
        assert len(np.unique(tail)) > 200, kind
        pad = img.planes[1][:, 25:].numpy()
        assert pad.size and len(np.unique(pad)) > 8, kind


def test_items_of_a_launch_differ(evam, O):
    """The three layouts the GPU matrix puts into one launch differ in every pitch, so a kernel or packer that used
    item 0's pitches for every item reads wrong pixels."""
    import torch

    rng = np.random.default_rng(4)
    for fmt in FORMATS:
        frames = [O.random_frame(rng, fc(O, fmt), 120, 64) for _ in range(3)]
        imgs, _ = SL.lay_out_all(evam, torch, O, frames, ["compact", "unequal+base16", "window+reversed"], rng, "cpu")
        for p in range(len(imgs[0].planes)):
            assert len({im.pitches[p] for im in imgs}) == 3, (fmt, p)
