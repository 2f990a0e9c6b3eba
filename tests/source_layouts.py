"""Source plane layouts for the parity tests: one frame's planes as views into one noisy buffer.

``Image.from_host`` uploads every plane as its own allocation, so every plane base is 256-byte aligned, and
``oracle.random_frame`` rounds every plane of a frame with one ``pitch_align``, so NV12's two pitches and I420's two
chroma pitches are always equal. :func:`lay_out` places the same pixel bytes the way a decoder or a frame pool may
hand them over, within what ``evam_pp_run`` accepts (plane pointers and pitches multiples of 16 bytes, pitch at least
the row bytes):

``compact``   planes back to back at ``plane_layout`` pitches, the first at a 256-byte boundary (the control).
``unequal``   pairwise different pitches. NV12: UV pitch > Y pitch (variant 0) or < Y pitch (variant 1). I420: V pitch
              < U pitch (variant 0) or > U pitch (variant 1), the U pitch never half the Y pitch. BGRX / BGR: the row
              bytes rounded up to 16, plus 16, 48 or 80.
``base16``    plane bases congruent to 16, 48 and 112 mod 256, a different residue for each plane.
``reversed``  chroma below luma in memory, for I420 also V below U; implies ``unequal`` and ``base16``.
``window``    every plane is a window at (xo, yo) of a surface whose pitch is at least four times the window's row
              bytes: ``surface[yo:yo + rows, xb:]``, so the pitch is the surface's. xo is a multiple of 32 pixels
              (I420), 16 (NV12, BGR) or 4 (BGRX), which keeps every plane pointer a multiple of 16; yo is even.

Kinds combine with ``+`` (``"unequal+base16"``, ``"window+reversed"``). The whole buffer is random bytes before the
planes are written, so padding, gaps and the surrounding surface are noise: a read of them that reaches an output shows
as a mismatch. The buffer ends with a guard tail of noise of at least (largest pitch) x (most rows) bytes, the largest
pitch taken over every kind a frame of this size can be laid out in (:func:`widest_pitch`), so reading any plane with
any other plane's pitch, or with the pitch of another frame of the same size in the same launch, stays inside the
allocation: a pitch mix-up gives wrong pixels, never an access out of bounds.
"""
import numpy as np

KINDS = ("compact", "unequal", "base16", "unequal+base16", "reversed", "window", "window+reversed")
RESIDUES = (16, 48, 112)
PACKED_EXTRA = (16, 48, 80)


def al16(n):
    return (n + 15) // 16 * 16


def plane_dims(O, fourcc, width, height):
    """[(rows, row_bytes)] of every plane."""
    if fourcc == O.NV12:
        return [(height, width), (height // 2, width)]
    if fourcc == O.I420:
        return [(height, width), (height // 2, width // 2), (height // 2, width // 2)]
    return [(height, width * O.bpp(fourcc))]


def x_step(O, fourcc):
    """Window origins are multiples of this many pixels: every plane pointer then stays a multiple of 16 bytes."""
    return {O.I420: 32, O.NV12: 16, O.BGR: 16}.get(fourcc, 4)


def widest_pitch(O, fourcc, width):
    """No pitch of any kind, for any plane of a frame of this format and width, is larger than this."""
    n = O.bpp(fourcc)
    return al16(4 * width * n + 3 * x_step(O, fourcc) * n) + 128


def unequal_pitches(O, fourcc, dims, rng, variant):
    """Pairwise different pitches for the planes of ``dims``, see the module docstring."""
    base = [al16(rb) for _, rb in dims]
    if len(dims) == 1:
        return [base[0] + PACKED_EXTRA[int(rng.integers(0, 3))]]
    if fourcc == O.NV12:
        lo, hi = base[0] + 16 * int(rng.integers(0, 2)), base[0] + 16 * int(rng.integers(2, 5))
        return [lo, hi] if variant == 0 else [hi, lo]
    while True:
        y = base[0] + 16 * int(rng.integers(0, 6))
        lo, hi = base[1] + 16 * int(rng.integers(0, 3)), base[1] + 16 * int(rng.integers(3, 7))
        u, v = (hi, lo) if variant == 0 else (lo, hi)
        if 2 * u != y and len({y, u, v}) == 3:
            return [y, u, v]


def lay_out(evam, torch, O, frame, kind, rng, device, variant=None):
    """``(Image, HostFrame)`` of ``frame`` (an ``oracle.HostFrame``) laid out as ``kind``.

    The Image's planes are views into one uint8 buffer on ``device`` (kept as ``image.buffer``; ``image.kind`` and
    ``image.variant`` record what was built); the HostFrame holds the same pixel bytes in compact planes, for the
    oracle. ``variant`` (0 / 1) picks the ``unequal`` sub-variant; None draws it from ``rng``."""
    flags = set(kind.split("+"))
    assert flags and flags <= {"compact", "unequal", "base16", "reversed", "window"}, kind
    assert "compact" not in flags or len(flags) == 1, kind
    if "reversed" in flags:
        flags |= {"unequal", "base16"}
    fc, W, H = frame.fourcc, frame.width, frame.height
    dims = plane_dims(O, fc, W, H)
    npl = len(dims)
    if variant is None:
        variant = int(rng.integers(0, 2))
    order = list(range(npl))[::-1] if "reversed" in flags else list(range(npl))  # memory order, lowest first
    residues = [RESIDUES[i] for i in rng.permutation(3)[:npl]] if "base16" in flags else None

    # per plane: pitch, bytes the plane's region takes, offset of the plane pointer inside its region
    if "window" in flags:
        step = x_step(O, fc)
        xo = step * int(rng.integers(1, 4))
        yo = 2 * int(rng.integers(1, 4))
        xbs = [xo * (O.bpp(fc) if npl == 1 else 1) // (2 if fc == O.I420 and p else 1) for p in range(npl)]
        while True:  # surface pitches: pairwise different
            pitch = [al16(4 * rb + xbs[p]) + 16 * int(rng.integers(0, 8)) for p, (_, rb) in enumerate(dims)]
            if len(set(pitch)) == npl:
                break
        region, inner = [], []
        for p, (rows, rb) in enumerate(dims):
            y = yo // (2 if p else 1)
            region.append(pitch[p] * (y + rows + 1 + int(rng.integers(0, 2))))
            inner.append(y * pitch[p] + xbs[p])
    else:
        if "unequal" in flags:
            pitch = unequal_pitches(O, fc, dims, rng, variant)
        else:
            pitch = [pt for _, pt in evam.plane_layout(fc, W, H)]
        region = [pitch[p] * dims[p][0] for p in range(npl)]
        inner = [0] * npl

    # offsets of the regions from a 256-byte boundary
    start, o = [0] * npl, 0
    for k, p in enumerate(order):
        if residues is not None:
            o += (residues[k] - o) % 256
        start[p] = o
        o += region[p]
        if residues is None and "window" in flags:
            o = al16(o)
    # the guard tail: the largest extent any layout of a frame of this size can have, so that this frame's planes read
    # with the pitches of another item of the same launch (frames of one size) stay inside as well
    guard = max(max(pitch), widest_pitch(O, fc, W)) * max(r for r, _ in dims)
    total = o + guard + 256
    gen = torch.Generator(device=device)
    gen.manual_seed(int(rng.integers(0, 2**31)))
    buf = torch.randint(0, 256, (total + 256,), dtype=torch.uint8, device=device, generator=gen)
    origin = (-buf.data_ptr()) % 256

    planes, host = [], []
    for p, (rows, rb) in enumerate(dims):
        px = np.ascontiguousarray(frame.planes[p][:rows, :rb])
        off = origin + start[p]
        if "window" in flags:
            y, xb = divmod(inner[p], pitch[p])
            surface = buf[off:off + region[p]].view(region[p] // pitch[p], pitch[p])
            view = surface[y:y + rows, xb:]
        else:
            view = buf[off:off + region[p]].view(rows, pitch[p])
        view[:, :rb].copy_(torch.from_numpy(px))
        planes.append(view)
        host.append(px)
    img = evam.Image(fc, W, H, planes)
    img.buffer, img.kind, img.variant = buf, kind, variant
    img.guard = (origin + o, guard)  # offset of the guard tail in the buffer, and its least size
    return img, O.HostFrame(fc, W, H, host)


def lay_out_all(evam, torch, O, frames, kinds, rng, device):
    """:func:`lay_out` of ``frames[i]`` as ``kinds[i]``: ``(images, host frames)``. Frames of one size get pitches
    that differ from frame to frame in every plane (a layout is drawn again until they do), so the items of a
    uniform-geometry launch never share a pitch."""
    imgs, hosts = [], []
    for f, k in zip(frames, kinds):
        for _ in range(64):
            img, host = lay_out(evam, torch, O, f, k, rng, device)
            same_size = [o for o in imgs if (o.fourcc, o.width, o.height) == (img.fourcc, img.width, img.height)]
            if not any(a == b for o in same_size for a, b in zip(o.pitches, img.pitches)):
                break
        else:
            raise AssertionError(f"no distinct pitches for {k} next to {[o.kind for o in imgs]}")
        imgs.append(img)
        hosts.append(host)
    return imgs, hosts
