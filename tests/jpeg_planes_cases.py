"""Shared inputs of the tests of the JPEG decoder's raw-plane output (evam_pp_decode_jpeg_planes): the fixtures under
tests/golden/jpeg_planes/ with Pillow's raw planes of each, Pillow's planes of a fresh file, and output images laid
out as views into one noisy buffer, with the buffer a correct decode leaves behind.

Nothing here needs a GPU; only :func:`pillow_planes` needs Pillow."""
import io
import os

import numpy as np

import jpeg_dec_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
PLANES_DIR = os.path.join(HERE, "golden", "jpeg_planes")
DEC_DIR, ENC_DIR = C.DEC_DIR, C.ENC_DIR

_planes = None


def header_420_even(f):
    """True for a baseline file of three components, luma sampling (2,2), chroma (1,1) and even width and height:
    read from the SOF0 segment alone."""
    try:
        segs = C.segments(f)
    except (AssertionError, IndexError):
        return False
    sof = [s for s in segs if s[0] == 0xC0]
    if not sof:
        return False
    d = f[sof[0][1] + 4:sof[0][2]]
    h, w, nc = d[1] << 8 | d[2], d[3] << 8 | d[4], d[5]
    return nc == 3 and d[7] == 0x22 and d[10] == 0x11 and d[13] == 0x11 and w % 2 == 0 and h % 2 == 0


def fixtures():
    """{name: (file bytes, (Y [H, W], Cb [H/2, W/2], Cr [H/2, W/2]))}: Pillow's raw planes of every fixture. Names
    that start with "dec/" and "enc/" are files of tests/golden/jpeg_dec/ and tests/golden/jpeg/."""
    global _planes
    if _planes is None:
        with np.load(os.path.join(PLANES_DIR, "planes.npz")) as z:
            _planes = {k: z[k] for k in z.files}
    out = {}
    for name in sorted(k[:-2] for k in _planes if k.endswith(".y")):
        d = {"dec/": DEC_DIR, "enc/": ENC_DIR}.get(name[:4], PLANES_DIR)
        fn = name[4:] if name[:4] in ("dec/", "enc/") else name
        out[name] = (open(os.path.join(d, fn + ".jpg"), "rb").read(),
                     (_planes[name + ".y"], _planes[name + ".cb"], _planes[name + ".cr"]))
    return out


def pillow_planes(file):
    """(Y, Cb, Cr) of an even-sized 4:2:0 file as libjpeg's jpeg_read_raw_data returns them, through Pillow's draft
    mode: Y is channel 0 of the full-scale YCbCr decode (luma is never re-sampled), Cb / Cr are channels 1, 2 of the
    half-scale decode, where libjpeg gives 4:2:0 chroma the full 8x8 islow IDCT and no up-sampling."""
    from PIL import Image

    im = Image.open(io.BytesIO(file))
    w, h = im.size
    assert w % 2 == 0 and h % 2 == 0 and im.mode == "RGB", (w, h, im.mode)
    got = im.draft("YCbCr", (w, h))
    assert got is not None and got[0] == "YCbCr" and im.size == (w, h) and im.decoderconfig[0] == 1, (got, im.size)
    y = np.ascontiguousarray(np.asarray(im)[..., 0])
    im = Image.open(io.BytesIO(file))
    got = im.draft("YCbCr", (w // 2, h // 2))
    assert got is not None and got[0] == "YCbCr" and im.size == (w // 2, h // 2) and im.decoderconfig[0] == 2, \
        (got, im.size, im.decoderconfig)
    c = np.asarray(im)
    assert y.shape == (h, w) and c.shape == (h // 2, w // 2, 3)
    return y, np.ascontiguousarray(c[..., 1]), np.ascontiguousarray(c[..., 2])


def planes_of(ycc, fmt):
    """The compact output planes of (Y, Cb, Cr): NV12 [Y, UV interleaved], I420 [Y, U, V]."""
    y, cb, cr = ycc
    if fmt == "NV12":
        return [y, np.ascontiguousarray(np.stack([cb, cr], axis=-1).reshape(cb.shape[0], cb.shape[1] * 2))]
    return [y, cb, cr]


# ---- output layouts (the kinds of tests/source_layouts.py, for planes that are written, not read) ------------------

KINDS = ("compact", "unequal", "base16", "reversed", "window")
RESIDUES = (16, 48, 112)


def al16(n):
    return (n + 15) // 16 * 16


def plane_dims(fmt, w, h):
    """[(rows, row bytes)] of every plane."""
    return [(h, w), (h // 2, w)] if fmt == "NV12" else [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def plan(fmt, w, h, kind, rng):
    """One image's planes inside a region that starts at a 256-byte boundary: ([(offset, pitch)] per plane, bytes).

    compact   planes back to back at their row bytes rounded up to 16
    unequal   pairwise different pitches, none of them another's half or double by construction of the row bytes
    base16    plane bases congruent to 16, 48 and 112 mod 256, and unequal pitches
    reversed  chroma below luma in memory, V below U; implies base16
    window    every plane is a window, below and to the right of the origin of a surface at least four times as wide
    Pointers and pitches stay multiples of 16."""
    assert kind in KINDS, kind
    dims = plane_dims(fmt, w, h)
    npl = len(dims)
    if kind == "compact":
        pitch = [al16(rb) for _, rb in dims]
    elif kind == "window":
        pitch = [al16(4 * rb) + 16 * int(e) for (_, rb), e in zip(dims, rng.permutation(8)[:npl] + 2)]
    else:
        while True:
            pitch = [al16(rb) + 16 * int(e) for (_, rb), e in zip(dims, rng.permutation(7)[:npl] + 1)]
            if len(set(pitch)) == npl:
                break
    order = list(range(npl))[::-1] if kind == "reversed" else list(range(npl))
    residues = [RESIDUES[i] for i in rng.permutation(3)[:npl]] if kind in ("base16", "reversed") else None
    offs, at = [0] * npl, 0
    for k, p in enumerate(order):
        rows = dims[p][0]
        if residues is not None:
            at += (residues[k] - at) % 256
        if kind == "window":
            above, left = int(rng.integers(1, 4)), 16 * int(rng.integers(1, 4))
            offs[p] = at + above * pitch[p] + left
            at += (above + rows + 1) * pitch[p]
        else:
            offs[p] = at
            at += rows * pitch[p]
    return list(zip(offs, pitch)), at


class Surface:
    """Output images of one size and fourcc, image i laid out as kinds[i], all inside one buffer of seeded noise."""

    def __init__(self, fmt, w, h, kinds, seed=0):
        rng = np.random.default_rng(seed)
        self.fmt, self.w, self.h = fmt, w, h
        self.dims = plane_dims(fmt, w, h)
        self.images, at = [], 0
        for kind in kinds:
            pl, size = plan(fmt, w, h, kind, rng)
            self.images.append([(at + o, pitch) for o, pitch in pl])
            at = (at + size + 255) // 256 * 256
        self.total = at + 256
        self.noise = rng.integers(0, 256, self.total, dtype=np.uint8)

    def fourcc(self, N):
        return N.FOURCC_NV12 if self.fmt == "NV12" else N.FOURCC_I420

    def c_images(self, N, base):
        """``evam_image[n]`` whose planes lie in a copy of the buffer at address ``base`` (a multiple of 256)."""
        assert base % 256 == 0
        imgs = (N.EvamImage * len(self.images))()
        for im, pl in zip(imgs, self.images):
            im.fourcc, im.width, im.height = self.fourcc(N), self.w, self.h
            for p, (off, pitch) in enumerate(pl):
                im.pitch[p] = pitch
                im.planes[p] = base + off
        return imgs

    def host_buffer(self):
        """(a writable copy of the noise at a 256-byte boundary, its address)."""
        raw = np.empty(self.total + 256, np.uint8)
        o = (-raw.ctypes.data) % 256
        buf = raw[o:o + self.total]
        buf[:] = self.noise
        return buf, buf.ctypes.data

    def device_images(self, evam, torch, device):
        """(the buffer on the device, [evam.Image] whose planes are views into it)."""
        raw = torch.empty(self.total + 256, dtype=torch.uint8, device=device)
        o = (-raw.data_ptr()) % 256
        buf = raw[o:o + self.total]
        buf.copy_(torch.from_numpy(self.noise))
        imgs = []
        N = evam.native
        for pl in self.images:
            views = [torch.as_strided(buf, (rows, rb), (pitch, 1), buf.storage_offset() + off)
                     for (off, pitch), (rows, rb) in zip(pl, self.dims)]
            imgs.append(evam.Image(self.fourcc(N), self.w, self.h, views))
        return buf, imgs

    def _view(self, buf, i, p):
        (off, pitch), (rows, rb) = self.images[i][p], self.dims[p]
        return np.lib.stride_tricks.as_strided(buf[off:], (rows, rb), (pitch, 1))

    def expected(self, planes):
        """The buffer after a correct decode: the noise with only the pixel bytes of ``planes[i]`` (compact planes of
        image i, or None for an image that must stay untouched) pasted in."""
        buf = self.noise.copy()
        for i, pls in enumerate(planes):
            for p, px in enumerate(pls or []):
                self._view(buf, i, p)[...] = px
        return buf

    def extract(self, buf, i):
        return [self._view(buf, i, p).copy() for p in range(len(self.dims))]

    def outside_intact(self, buf):
        """True when every byte outside all images' pixel bytes kept its noise."""
        mask = np.ones(self.total, bool)
        for i in range(len(self.images)):
            for p in range(len(self.dims)):
                self._view(mask, i, p)[...] = False
        return bool((buf[mask] == self.noise[mask]).all())


def decode_host(N, files, surface, n=None, status=None):
    """``evam_pp_decode_jpeg_planes_host`` of ``files`` into ``surface``: (rc, the buffer afterwards, status, the
    library's message)."""
    lib = N.load_library()
    keep, ptrs, lens = N.jpeg_file_arrays(files)
    buf, base = surface.host_buffer()
    imgs = surface.c_images(N, base)
    st = np.full(max(len(files), 1), 77, np.int32) if status is None else status
    rc = lib.evam_pp_decode_jpeg_planes_host(ptrs, lens, len(files) if n is None else n, imgs,
                                             None if st is False else st.ctypes.data)
    return rc, buf, st, lib.evam_pp_last_error().decode()


def first_difference(a, b):
    bad = np.flatnonzero(a != b)
    return f"{len(bad)} bytes differ, first at {bad[:3].tolist()}" if bad.size else ""
