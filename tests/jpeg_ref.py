"""numpy restatement of libjpeg's baseline encoder as cv2.imencode('.jpg') and Pillow (subsampling=2) drive it:
baseline, 4:2:0, JDCT_ISLOW, Annex K tables, no restart interval. ``encode`` returns the whole JFIF file and a few
counts of what the entropy coder met, so a test can assert that its input really exercised the hard parts. Its
``sampling`` and ``restart`` arguments write the other files the decoder accepts, as Pillow's ``subsampling=0 / 1``,
mode ``L`` and ``restart_marker_blocks`` make libjpeg write them: 4:2:2 (h2v1 down-sampling, 16x8 MCUs), 4:4:4, one
grey component, and restart intervals (a DRI segment, RST0..7 in turn behind bits padded with ones).

The colour conversion, down-sampling, DCT and quantisation are vectorised over blocks; only the entropy loop runs per
block. ``tests/test_jpeg_host.py`` pins this file byte for byte to files libjpeg-turbo (through Pillow) wrote."""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63])

Q_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
    51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
    101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
    99, 99, 99, 99] + [99] * 32)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
    0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]

HEADER_LEN = 623


def _huff(bits, vals):
    """symbol -> (code, length) of a JPEG Huffman table given as its 16 counts and its symbols."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


HUFF = {"dc0": _huff(DC_LUMA_BITS, DC_VALS), "ac0": _huff(AC_LUMA_BITS, AC_LUMA_VALS),
        "dc1": _huff(DC_CHROMA_BITS, DC_VALS), "ac1": _huff(AC_CHROMA_BITS, AC_CHROMA_VALS)}


def quant_tables(quality: int):
    """The two 8-bit tables of jpeg_set_quality(quality, TRUE), in natural order."""
    q = max(1, min(100, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64) for base in (Q_LUMA, Q_CHROMA))


SAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "grey": (1, 1)}


def header(width: int, height: int, quality: int, sampling: str = "420", restart: int = 0) -> bytes:
    """Everything up to the scan, as libjpeg writes it: grey files carry the luma tables alone, and a DRI segment
    stands between the last DHT and the SOS."""
    ql, qc = quant_tables(quality)
    hs, vs = SAMPLINGS[sampling]
    ncomp = 1 if sampling == "grey" else 3
    b = bytearray(b"\xFF\xD8")
    b += b"\xFF\xE0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for i, t in enumerate((ql, qc)[:2 if ncomp == 3 else 1]):
        b += b"\xFF\xDB\x00\x43" + bytes([i]) + bytes(int(v) for v in t[ZIGZAG])
    b += bytes([0xFF, 0xC0, 0x00, 8 + 3 * ncomp, 0x08, height >> 8, height & 255, width >> 8, width & 255, ncomp])
    b += bytes([0x01, hs << 4 | vs, 0x00]) + (b"\x02\x11\x01\x03\x11\x01" if ncomp == 3 else b"")
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS))[:4 if ncomp == 3 else 2]:
        n = 2 + 1 + 16 + len(vals)
        b += b"\xFF\xC4" + bytes([n >> 8, n & 255, tc_th]) + bytes(bits) + bytes(vals)
    if restart:
        b += bytes([0xFF, 0xDD, 0x00, 0x04, restart >> 8, restart & 255])
    b += bytes([0xFF, 0xDA, 0x00, 6 + 2 * ncomp, ncomp, 0x01, 0x00]) + (b"\x02\x11\x03\x11" if ncomp == 3 else b"")
    b += b"\x00\x3F\x00"
    assert sampling != "420" or restart or len(b) == HEADER_LEN
    return bytes(b)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(bgr: np.ndarray):
    """libjpeg's rgb_ycc_convert on u8 values: three int64 [H, W] planes."""
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def _downsample(c, h16):
    """h2v2_downsample on a plane already padded to a multiple of 16 columns; rows are padded as libjpeg does."""
    h, w = c.shape
    c = _pad(c, h + (h & 1), w)
    bias = np.tile(np.array([1, 2]), w // 4 + 1)[:w // 2]
    d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    return _pad(d, h16 // 2, w // 2)


def _downsample_h2v1(c, h8):
    """h2v1_downsample (bias 0, 1, 0, 1) on a plane already padded to a multiple of 16 columns."""
    h, w = c.shape
    bias = np.tile(np.array([0, 1]), w // 4 + 1)[:w // 2]
    return _pad((c[:, 0::2] + c[:, 1::2] + bias) >> 1, h8, w // 2)


_C = {k: int(v * 8192 + 0.5) for k, v in dict(
    c0_298=0.298631336, c0_390=0.390180644, c0_541=0.541196100, c0_765=0.765366865, c0_899=0.899976223,
    c1_175=1.175875602, c1_501=1.501321110, c1_847=1.847759065, c1_961=1.961570560, c2_053=2.053119869,
    c2_562=2.562915447, c3_072=3.072711026).items()}


def _dct_pass(d, first):
    """One pass of jfdctint.c along the last axis of d [..., 8]."""
    def desc(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0] = (t10 + t11) << 2
        out[..., 4] = (t10 - t11) << 2
    else:
        out[..., 0] = desc(t10 + t11, 2)
        out[..., 4] = desc(t10 - t11, 2)
    z1 = (t12 + t13) * _C["c0_541"]
    out[..., 2] = desc(z1 + t13 * _C["c0_765"], n)
    out[..., 6] = desc(z1 - t12 * _C["c1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _C["c1_175"]
    t4, t5, t6, t7 = t4 * _C["c0_298"], t5 * _C["c2_053"], t6 * _C["c3_072"], t7 * _C["c1_501"]
    z1, z2 = -z1 * _C["c0_899"], -z2 * _C["c2_562"]
    z3, z4 = -z3 * _C["c1_961"] + z5, -z4 * _C["c0_390"] + z5
    out[..., 7] = desc(t4 + z1 + z3, n)
    out[..., 5] = desc(t5 + z2 + z4, n)
    out[..., 3] = desc(t6 + z2 + z3, n)
    out[..., 1] = desc(t7 + z1 + z4, n)
    return out


def blocks_quantised(plane: np.ndarray, qtab: np.ndarray) -> np.ndarray:
    """[H8, W8] samples -> [H8/8, W8/8, 64] quantised coefficients in zig-zag order."""
    h, w = plane.shape
    b = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [by, bx, row, col]
    b = _dct_pass(b, True)
    b = _dct_pass(b.swapaxes(-1, -2), False).swapaxes(-1, -2)
    c = b.reshape(h // 8, w // 8, 64)
    qv = 8 * qtab
    q = np.sign(c) * ((np.abs(c) + (qv >> 1)) // qv)
    return q[..., ZIGZAG]


def mcu_grid(w: int, h: int, sampling: str = "420"):
    """(MCU rows, MCUs per row, blocks per MCU). A grey scan is not interleaved: its MCU is one block."""
    hs, vs = SAMPLINGS[sampling]
    return -(-h // (8 * vs)), -(-w // (8 * hs)), hs * vs + (0 if sampling == "grey" else 2)


def coefficients(bgr: np.ndarray, quality: int, sampling: str = "420"):
    """The MCU-ordered blocks of the scan: ([n_mcu, blocks per MCU, 64] int64, number of dummy Y blocks)."""
    h, w = bgr.shape[:2]
    ql, qc = quant_tables(quality)
    hs, vs = SAMPLINGS[sampling]
    mr, mc, bpm = mcu_grid(w, h, sampling)
    h8, w8, hm, wm = -(-h // 8) * 8, -(-w // 8) * 8, mr * 8 * vs, mc * 8 * hs
    if sampling == "grey":
        return blocks_quantised(_pad(bgr[..., 1].astype(np.int64), h8, w8), ql).reshape(mr * mc, 1, 64), 0
    y, cb, cr = ycc(bgr)
    yq = blocks_quantised(_pad(y, h8, w8), ql)
    yb = np.zeros((mr * vs, mc * hs, 64), np.int64)
    yb[:h8 // 8, :w8 // 8] = yq
    out = np.zeros((mr, mc, bpm, 64), np.int64)
    dummies = 0
    for k, (dy, dx) in enumerate((dy, dx) for dy in range(vs) for dx in range(hs)):
        out[:, :, k] = yb[dy::vs, dx::hs]
        rows = (np.arange(mr) * vs + dy) >= h8 // 8
        cols = (np.arange(mc) * hs + dx) >= w8 // 8
        dummy = rows[:, None] | cols[None, :]
        if k:
            out[:, :, k, 0] = np.where(dummy, out[:, :, k - 1, 0], out[:, :, k, 0])
        dummies += int(dummy.sum())
    for k, c in ((hs * vs, cb), (hs * vs + 1, cr)):
        if sampling == "420":
            c = _downsample(_pad(c, h, wm), hm)
        elif sampling == "422":
            c = _downsample_h2v1(_pad(c, h, wm), hm)
        else:
            c = _pad(c, hm, wm)
        out[:, :, k] = blocks_quantised(c, qc)
    return out.reshape(mr * mc, bpm, 64), dummies


def _pack(codes, lens):
    """(code, length) pairs -> (bytes padded with ones and stuffed, number of stuffed zeros)."""
    codes = np.asarray(codes, np.int64)
    lens = np.asarray(lens, np.int64)
    total = int(lens.sum())
    idx = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    bits = ((codes[idx] >> (lens[idx] - 1 - pos)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    raw = np.packbits(bits)
    ff = raw == 0xFF
    out = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    out[np.arange(len(raw)) + np.cumsum(ff) - ff] = raw
    return out.tobytes(), int(ff.sum())


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def encode(bgr_u8: np.ndarray, quality: int, *, sampling: str = "420", restart: int = 0):
    """(JFIF bytes, stats) of an [H, W, 3] uint8 BGR image. sampling: "420", "422", "444", or "grey" (one component,
    the G channel). restart: MCUs per restart interval, 0 for none; the bits before each RSTn are padded with ones and
    the DC predictions start again behind it. stats: zrl, stuffed, max_category, dummy_blocks,
    min_block_bits, max_dc_category (the largest DC-difference category), max_zrl_run (the most ZRL codes in front of
    one AC coefficient), no_eob_blocks (blocks whose coefficient 63 is non-zero: they end without an EOB)."""
    bgr = np.ascontiguousarray(bgr_u8)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    assert 0 <= restart <= 65535
    h, w = bgr.shape[:2]
    coef, dummies = coefficients(bgr, quality, sampling)
    bpm = coef.shape[1]
    nluma = bpm if sampling == "grey" else bpm - 2
    codes, lens, scan = [], [], bytearray()
    stats = {"zrl": 0, "stuffed": 0, "max_category": 0, "dummy_blocks": dummies, "min_block_bits": 1 << 30,
             "max_dc_category": 0, "max_zrl_run": 0, "no_eob_blocks": 0}
    pred = [0, 0, 0]
    flat = coef.reshape(-1, 64).tolist()
    for bi, blk in enumerate(flat):
        kb = bi % bpm
        if restart and kb == 0 and bi and (bi // bpm) % restart == 0:
            data, stuffed = _pack(codes, lens)
            scan += data + bytes([0xFF, 0xD0 + (bi // bpm // restart - 1) % 8])
            stats["stuffed"] += stuffed
            codes, lens, pred = [], [], [0, 0, 0]
        comp = 0 if kb < nluma else kb - nluma + 1
        dc, ac = (HUFF["dc0"], HUFF["ac0"]) if comp == 0 else (HUFF["dc1"], HUFF["ac1"])
        n0 = len(lens)
        v = blk[0] - pred[comp]
        pred[comp] = blk[0]
        s = _category(v)
        stats["max_category"] = max(stats["max_category"], s)
        stats["max_dc_category"] = max(stats["max_dc_category"], s)
        c, ln = dc[s]
        codes.append(c)
        lens.append(ln)
        if s:
            codes.append((v if v >= 0 else v - 1) & ((1 << s) - 1))
            lens.append(s)
        run = 0
        for k in range(1, 64):
            v = blk[k]
            if v == 0:
                run += 1
                continue
            stats["max_zrl_run"] = max(stats["max_zrl_run"], run >> 4)
            while run > 15:
                c, ln = ac[0xF0]
                codes.append(c)
                lens.append(ln)
                stats["zrl"] += 1
                run -= 16
            s = _category(v)
            stats["max_category"] = max(stats["max_category"], s)
            c, ln = ac[(run << 4) | s]
            codes.append(c)
            lens.append(ln)
            codes.append((v if v >= 0 else v - 1) & ((1 << s) - 1))
            lens.append(s)
            run = 0
        if run:
            c, ln = ac[0x00]
            codes.append(c)
            lens.append(ln)
        else:
            stats["no_eob_blocks"] += 1
        stats["min_block_bits"] = min(stats["min_block_bits"], sum(lens[n0:]))
    data, stuffed = _pack(codes, lens)
    stats["stuffed"] += stuffed
    return header(w, h, quality, sampling, restart) + bytes(scan) + data + b"\xFF\xD9", stats
