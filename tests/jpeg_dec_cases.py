"""Shared inputs of the JPEG decoder tests: the fixtures under tests/golden/jpeg_dec/ (files written by Pillow and
Pillow's own decode of each), the fixed list of 16 damaged scans derived from three of them, and the byte patches that
turn a valid file into each file the header parse refuses. Nothing here needs Pillow or a GPU."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEC_DIR = os.path.join(HERE, "golden", "jpeg_dec")
ENC_DIR = os.path.join(HERE, "golden", "jpeg")
DEC_SRC = os.path.join(os.path.dirname(HERE), "edge-video-analytics-microservice_amd", "csrc", "evam_jpeg_dec.h")

_pixels = None


def fixtures():
    """{name: (file bytes, Pillow's [H, W, 3] BGR pixels)} of every decodable fixture."""
    global _pixels
    if _pixels is None:
        with np.load(os.path.join(DEC_DIR, "pixels.npz")) as z:
            _pixels = {k: z[k] for k in z.files}
    return {k: (open(os.path.join(DEC_DIR, k + ".jpg"), "rb").read(), v) for k, v in sorted(_pixels.items())}


def refused_fixture():
    return open(os.path.join(DEC_DIR, "progressive_16x16.jpg"), "rb").read()


def encoder_fixtures():
    """{name: (file bytes, Pillow's BGR pixels)} of the 21 files of tests/golden/jpeg/ (the encoder's goldens)."""
    with np.load(os.path.join(DEC_DIR, "encoder_pixels.npz")) as z:
        return {k: (open(os.path.join(ENC_DIR, k + ".jpg"), "rb").read(), z[k]) for k in sorted(z.files)}


def source_constant(name):
    """An integer ``constexpr int <name> = <value>;`` of csrc/evam_jpeg_dec.h."""
    m = re.search(r"constexpr int %s = (\d+);" % name, open(DEC_SRC).read())
    assert m, name
    return int(m.group(1))


def segments(f):
    """[(marker, offset of the FF, offset behind the segment)] up to and including SOS."""
    out, pos = [], 2
    while True:
        assert f[pos] == 0xFF, pos
        m = f[pos + 1]
        ln = f[pos + 2] << 8 | f[pos + 3]
        out.append((m, pos, pos + 2 + ln))
        pos += 2 + ln
        if m == 0xDA:
            return out


def scan_bounds(f):
    """(first byte of the entropy-coded data, the EOI's offset) of a complete file."""
    assert f[-2:] == b"\xFF\xD9"
    return segments(f)[-1][2], len(f) - 2


def find_segment(f, marker):
    return next(s for s in segments(f) if s[0] == marker)


def max_code_length(f):
    """The longest Huffman code any DHT segment of the file defines."""
    best = 0
    for m, a, b in segments(f):
        if m != 0xC4:
            continue
        o = a + 4
        while o < b:
            counts = f[o + 1:o + 17]
            best = max([best] + [ln + 1 for ln in range(16) if counts[ln]])
            o += 17 + sum(counts)
    return best


DAMAGED_SOURCES = ("noise_64x48_420", "rstwrap_64x48_420", "optimize_48x32_444")


def damaged_scans():
    """The fixed list: [(name, file bytes, status must be non-zero)]. Bit flips and the all-zero scan may leave a
    decodable scan, so only agreement with the host twin is asked of them."""
    fx = fixtures()
    a, b, c = (fx[k][0] for k in DAMAGED_SOURCES)
    out = []
    s0, e0 = scan_bounds(a)
    n = e0 - s0
    for label, keep in (("1", 1), ("half", n // 2), ("all_but_one", n - 1)):
        out.append((f"truncated_{label}", a[:s0 + keep], True))
    k = a.index(b"\xFF\x00", s0)
    assert k < e0
    out.append(("ff_without_00", a[:k + 1] + a[k + 2:], True))
    sb, eb = scan_bounds(b)
    k = b.index(b"\xFF\xD0", sb)
    out.append(("rst_out_of_sequence", b[:k + 1] + b"\xD1" + b[k + 2:], True))
    k = b.index(b"\xFF\xD3", sb)
    out.append(("rst_missing", b[:k] + b[k + 2:], True))
    rng = np.random.default_rng(2026)
    for i in range(8):
        src = (a, b, c)[i % 3]
        s, e = scan_bounds(src)
        at, bit = int(rng.integers(s, e)), int(rng.integers(0, 8))
        out.append((f"bit_flip_{i}", src[:at] + bytes([src[at] ^ (1 << bit)]) + src[at + 1:], False))
    out.append(("all_ff", a[:s0] + b"\xFF" * n + a[e0:], True))
    # zeros are codes of the Annex K tables (DC category 0, AC 0/1): a long enough run of them is a valid scan
    out.append(("all_zero", a[:s0] + b"\x00" * n + a[e0:], False))
    assert len(out) == 16
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out, self.pos = 0, 0, bytearray(), 0

    def put(self, value, length):
        self.acc = self.acc << length | value
        self.n += length
        self.pos += length
        while self.n >= 8:
            self.n -= 8
            byte = self.acc >> self.n & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            pad = 8 - self.n
            self.put((1 << pad) - 1, pad)
        return bytes(self.out)


def _one_code_per_length(symbols):
    """A DHT body's (counts, symbols) and {symbol: (code, length)}: symbol k gets the code of k ones and a zero,
    k + 1 bits long, so the last of 16 symbols has a 16-bit code and the all-ones code stays unused."""
    assert len(symbols) <= 16
    return ([1] * len(symbols) + [0] * (16 - len(symbols)), list(symbols),
            {s: ((1 << (k + 1)) - 2, k + 1) for k, s in enumerate(symbols)})


def long_block_file(w, h, colour, seed):
    """A baseline file written from coefficients, not pixels, whose every block is longer than any pixel content gives:
    63 AC coefficients of size 3, each a 16-bit Huffman code and 3 value bits, 1,197 bits and a DC symbol per block and
    no EOB. All quantisers are 1, so the values stay small. Grey, or 4:2:0 with a second pair of tables for chroma.
    Returns (file bytes, [bit position in the un-stuffed scan at which each block ends])."""
    rng = np.random.default_rng(seed)
    dc_counts, dc_syms, dc_code = _one_code_per_length(range(12))
    # run 0 / size 3 last: the 16-bit code. The others are legal filler that the scan never uses.
    ac_syms = [0x00, 0xF0, 0x01, 0x02, 0x11, 0x04, 0x12, 0x21, 0x05, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x03]
    ac_counts, ac_syms, ac_code = _one_code_per_length(ac_syms)
    ncomp = 3 if colour else 1
    seg = lambda m, body: bytes([0xFF, m, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)
    f = b"\xFF\xD8" + seg(0xDB, [0] + [1] * 64)
    sof = [8, h >> 8, h & 255, w >> 8, w & 255, ncomp]
    for c in range(ncomp):
        sof += [c + 1, 0x22 if colour and c == 0 else 0x11, 0]
    f += seg(0xC0, sof)
    for t in range(2 if colour else 1):
        f += seg(0xC4, [t] + dc_counts + dc_syms) + seg(0xC4, [0x10 | t] + ac_counts + ac_syms)
    sos = [ncomp]
    for c in range(ncomp):
        sos += [c + 1, 0x11 if c else 0x00]
    f += seg(0xDA, sos + [0, 63, 0])
    mcu = 16 if colour else 8
    n_blocks = -(-w // mcu) * -(-h // mcu) * (6 if colour else 1)
    bits, ends = _Bits(), []
    for _ in range(n_blocks):
        cat = int(rng.integers(0, 3))  # DC differences of -3..3: the sums stay near 0
        bits.put(*dc_code[cat])
        if cat:
            bits.put(int(rng.integers(0, 1 << cat)), cat)
        for v in rng.integers(0, 8, 63):  # 3 value bits: -7..-4 and 4..7
            bits.put(*ac_code[0x03])
            bits.put(int(v), 3)
        ends.append(bits.pos)
    return f + bits.finish() + b"\xFF\xD9", ends


def patch(f, at, new):
    return f[:at] + bytes(new) + f[at + len(new):]


UNSUPPORTED, INVALID = -2, -1


def refusals():
    """[(name, file bytes, expected status, a word of the message)]: each built by patching a valid fixture."""
    fx = fixtures()
    f = fx["noise_64x48_420"][0]
    g = fx["noise_64x48_grey"][0]
    sof = find_segment(f, 0xC0)[1]
    sos = find_segment(f, 0xDA)[1]
    dqt = find_segment(f, 0xDB)[1]
    app0 = find_segment(f, 0xE0)
    out = []
    for m, word in ((0xC1, "extended"), (0xC2, "progressive"), (0xC3, "lossless"), (0xC5, "differential"),
                    (0xC9, "arithmetic"), (0xCA, "arithmetic")):
        out.append((f"sof{m & 15}", patch(f, sof + 1, [m]), UNSUPPORTED, word))
    out.append(("12_bit", patch(f, sof + 4, [12]), UNSUPPORTED, "12-bit"))
    out.append(("2_components", patch(f, sof + 9, [2]), UNSUPPORTED, "2 components"))
    out.append(("4_components", patch(f, sof + 9, [4]), UNSUPPORTED, "4 components"))
    out.append(("sampling_4x1", patch(f, sof + 11, [0x41]), UNSUPPORTED, "sampling"))
    out.append(("sampling_1x2", patch(f, sof + 11, [0x12]), UNSUPPORTED, "sampling"))
    out.append(("chroma_2x1", patch(f, sof + 14, [0x21]), UNSUPPORTED, "sampling"))
    out.append(("dqt_16_bit", patch(f, dqt + 4, [0x10]), UNSUPPORTED, "16-bit"))
    # a scan of one of the three components: what a multi-scan (non-interleaved) file starts with
    one = f[:sos] + b"\xFF\xDA\x00\x08\x01\x01\x00\x00\x3F\x00" + f[sos + 14:]
    out.append(("more_than_one_scan", one, UNSUPPORTED, "scan"))
    out.append(("spectral_selection", patch(f, sos + 11, [1]), UNSUPPORTED, "spectral"))
    out.append(("spectral_end", patch(f, sos + 12, [5]), UNSUPPORTED, "spectral"))
    out.append(("successive_approximation", patch(f, sos + 13, [0x10]), UNSUPPORTED, "approximation"))
    adobe = b"\xFF\xEE\x00\x0EAdobe\x00\x64\x00\x00\x00\x00"
    out.append(("adobe_transform_0", f[:app0[2]] + adobe + b"\x00" + f[app0[2]:], UNSUPPORTED, "Adobe"))
    out.append(("adobe_transform_2", f[:app0[2]] + adobe + b"\x02" + f[app0[2]:], UNSUPPORTED, "Adobe"))
    out.append(("no_soi", patch(f, 0, [0xFF, 0xD9]), INVALID, "SOI"))
    out.append(("no_soi_text", b"not a jpeg file at all", INVALID, "SOI"))
    out.append(("segment_past_len", patch(f, dqt + 2, [0xFF, 0xFF]), INVALID, "past"))
    out.append(("cut_in_header", f[:sof + 6], INVALID, "past"))
    out.append(("undefined_dc_table", patch(g, find_segment(g, 0xDA)[1] + 6, [0x10]), INVALID, "never"))
    out.append(("undefined_ac_table", patch(g, find_segment(g, 0xDA)[1] + 6, [0x01]), INVALID, "never"))
    out.append(("zero_width", patch(f, sof + 7, [0, 0]), INVALID, "zero"))
    out.append(("zero_height", patch(f, sof + 5, [0, 0]), INVALID, "zero"))
    return out


def adobe_ycc(f):
    """The file with an Adobe APP14 segment of transform 1 (YCbCr) behind its APP0: decoded as before."""
    app0 = find_segment(f, 0xE0)
    return f[:app0[2]] + b"\xFF\xEE\x00\x0EAdobe\x00\x64\x00\x00\x00\x00\x01" + f[app0[2]:]
