"""Shared inputs of the JPEG decoder tests: the fixtures under tests/golden/jpeg_dec/ (files written by Pillow and
Pillow's own decode of each), the fixed list of 16 damaged scans derived from three of them, and the byte patches that
turn a valid file into each file the header parse refuses; and the files of the GPU sweep, which tests/jpeg_ref.py
writes from seeds, with their preconditions as functions of the file bytes. Nothing here needs Pillow or a GPU."""
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


def source_constant(name, path=None):
    """An integer ``constexpr int <name> = <value>;`` of csrc/evam_jpeg_dec.h, or of the csrc/ file named."""
    src = DEC_SRC if path is None else os.path.join(os.path.dirname(DEC_SRC), path)
    m = re.search(r"constexpr int %s = (\d+);" % name, open(src).read())
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

    def pad(self):
        if self.n:
            pad = 8 - self.n
            self.put((1 << pad) - 1, pad)

    def finish(self):
        self.pad()
        return bytes(self.out)


def _one_code_per_length(symbols):
    """A DHT body's (counts, symbols) and {symbol: (code, length)}: symbol k gets the code of k ones and a zero,
    k + 1 bits long, so the last of 16 symbols has a 16-bit code and the all-ones code stays unused."""
    assert len(symbols) <= 16
    return ([1] * len(symbols) + [0] * (16 - len(symbols)), list(symbols),
            {s: ((1 << (k + 1)) - 2, k + 1) for k, s in enumerate(symbols)})


def long_block_file(w, h, colour, seed, sampling=None, restart=0):
    """A baseline file written from coefficients, not pixels, whose every block is longer than any pixel content gives:
    63 AC coefficients of size 3, each a 16-bit Huffman code and 3 value bits, 1,197 bits and a DC symbol per block and
    no EOB. All quantisers are 1, so the values stay small. Grey, or 4:2:0 with a second pair of tables for chroma;
    ``sampling`` ("420", "422", "444", "grey") overrides ``colour``. ``restart`` is the number of MCUs per restart
    interval: a DRI segment, ones up to the byte border, RSTn cycling 0..7. The DC differences are drawn all the same,
    so each interval's sums stay near 0.
    Returns (file bytes, [bit position in the compacted scan (no stuffing, no markers, each interval's padding counted)
    at which each block ends])."""
    if sampling is None:
        sampling = "420" if colour else "grey"
    colour = sampling != "grey"
    hs, vs = {"420": (2, 2), "422": (2, 1), "444": (1, 1), "grey": (1, 1)}[sampling]
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
        sof += [c + 1, hs << 4 | vs if c == 0 else 0x11, 0]
    f += seg(0xC0, sof)
    for t in range(2 if colour else 1):
        f += seg(0xC4, [t] + dc_counts + dc_syms) + seg(0xC4, [0x10 | t] + ac_counts + ac_syms)
    sos = [ncomp]
    for c in range(ncomp):
        sos += [c + 1, 0x11 if c else 0x00]
    if restart:
        f += seg(0xDD, [restart >> 8, restart & 255])
    f += seg(0xDA, sos + [0, 63, 0])
    bpm = hs * vs + 2 if colour else 1
    n_blocks = -(-w // (8 * hs)) * -(-h // (8 * vs)) * bpm
    bits, ends = _Bits(), []
    for b in range(n_blocks):
        if restart and b and b % (restart * bpm) == 0:
            bits.pad()
            bits.out += bytes([0xFF, 0xD0 + (b // (restart * bpm) - 1) % 8])
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


# ---- the files of tests/test_gpu_jpeg_dec_sweep.py ----------------------------------------------------------------
# Built here so that the CPU tests pin the host twin to Pillow on the very files the GPU tests compare with the twin,
# and so that the sanitizer program runs on them first. Every precondition is a function of the file's bytes alone.

SAMPLINGS = ("420", "422", "444", "grey")
UNSTUFF_BYTES = source_constant("kJdecUnstuffBytes", "evam_jpeg_dec_kernels.h")
PASS = 256 * UNSTUFF_BYTES  # raw scan bytes one pass of evam_jdec_unstuff takes


def _scan_array(f):
    s, e = scan_bounds(f)
    return np.frombuffer(f, np.uint8, e - s, s)


def rst_markers(f):
    """[(offset of the FF in the raw scan, n)] of every RSTn of a complete file."""
    a = _scan_array(f)
    at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7))
    return [(int(k), int(a[k + 1]) & 7) for k in at]


def stuffed_pairs(f):
    """Offsets in the raw scan of the FF of every FF 00 pair."""
    a = _scan_array(f)
    return np.flatnonzero((a[:-1] == 0xFF) & (a[1:] == 0)).tolist()


def interval_table(f):
    """The interval table evam_jdec_unstuff must write: the byte of the compacted scan (stuffed zeros and markers
    dropped) at which each restart interval starts, and behind the last one the compacted length."""
    a = _scan_array(f)
    ff = a == 0xFF
    after_ff = np.concatenate([[False], ff[:-1]])
    marker = ff & np.concatenate([(a[1:] >= 0xD0) & (a[1:] <= 0xD7), [False]])
    keep = ~((after_ff & (a == 0)) | marker | np.concatenate([[False], marker[:-1]]))
    kept = np.cumsum(keep)
    return [0] + kept[marker].tolist() + [int(kept[-1])]


def sampled(kind, w, h, seed, quality, sampling, restart):
    from jpeg_content import content
    import jpeg_ref

    return jpeg_ref.encode(content(kind, w, h, seed), quality, sampling=sampling, restart=restart)[0]


def mcu_size(sampling):
    return {"420": (16, 16), "422": (16, 8), "444": (8, 8), "grey": (8, 8)}[sampling]


_cut_widths = {}


def cut_pairs_width(sampling):
    """One MCU more than the smallest width, one MCU row high, at which saturated noise (seed 0) at quality 100 with
    a marker behind every MCU has more than 2 * PASS + 1 bytes of raw scan; the smallest is found as
    test_chunk_borders finds its widths. At the smallest width itself the last marker, which stands in front of the
    last MCU, cannot lie in the third pass."""
    if sampling not in _cut_widths:
        mw, mh = mcu_size(sampling)
        per_mcu = len(_scan_array(sampled("sat", 4 * mw, mh, 0, 100, sampling, 1))) // 4
        k = max((2 * PASS + 1) // per_mcu - 3, 1)
        while len(_scan_array(sampled("sat", k * mw, mh, 0, 100, sampling, 1))) <= 2 * PASS + 1:
            k += 1
            assert k * mw <= 32768
        _cut_widths[sampling] = (k + 1) * mw
    return _cut_widths[sampling]


def cut_pairs_properties(f):
    """What the cut-pairs tests assert of a file, from its raw scan: its length, the number of residues mod
    UNSTUFF_BYTES at which markers start, the markers and the FF 00 pairs whose FF is the last byte of a pass,
    whether a marker lies wholly in the third pass, how often the markers run past RST7, and that they cycle 0..7."""
    m = rst_markers(f)
    return {"len": len(_scan_array(f)),
            "residues": len({k % UNSTUFF_BYTES for k, _ in m}),
            "marker_cut": [k for k, _ in m if k % PASS == PASS - 1],
            "pair_cut": [k for k in stuffed_pairs(f) if k % PASS == PASS - 1],
            "third_pass": any(2 * PASS <= k and k + 2 <= 3 * PASS for k, _ in m),
            "wraps": (len(m) - 1) // 8 if m else 0,
            "in_sequence": [n for _, n in m] == [i % 8 for i in range(len(m))]}


# sampling -> (seed, residues, marker_cut, pair_cut, wraps) of its cut-pairs file. search_cut_seeds (seeds 0..199) found
# no seed with both a marker and an FF 00 pair on a pass border for any sampling, and none with a marker there for
# 4:2:2 and 4:4:4 (their markers stand about 400 and 300 bytes apart with little spread, and the two borders fall
# between them); 13 and 21 markers cannot start at 16 residues or pass RST7 twice. Each file has what is listed here,
# and the four together have every property.
CUT_SEEDS = {"420": (112, 12, [PASS - 1], [], 1), "422": (67, 14, [], [PASS - 1], 2),
             "444": (0, 13, [], [2 * PASS - 1], 3), "grey": (1, 16, [PASS - 1], [], 8)}


def cut_pairs_file(sampling, seed=None):
    """The cut-pairs file of the sampling: saturated noise at quality 100, one MCU row, a marker behind every MCU."""
    seed = CUT_SEEDS[sampling][0] if seed is None else seed
    return sampled("sat", cut_pairs_width(sampling), mcu_size(sampling)[1], seed, 100, sampling, 1)


def search_cut_seeds(sampling, limit=200):
    """How CUT_SEEDS was chosen: [(seed, properties)] of the seeds whose file is long enough, has a marker in the third
    pass and a marker or an FF 00 pair on a pass border."""
    out = []
    for seed in range(limit):
        p = cut_pairs_properties(cut_pairs_file(sampling, seed))
        if p["len"] > 2 * PASS + 1 and p["third_pass"] and (p["marker_cut"] or p["pair_cut"]):
            out.append((seed, p))
    return out


def grad_noise(w, h, seed):
    """A gradient with +-8 of noise on it."""
    from jpeg_content import content

    n = np.random.default_rng(seed).integers(-8, 9, (h, w, 3))
    return np.clip(content("grad", w, h).astype(np.int64) + n, 0, 255).astype(np.uint8)


_long = {}


def long_interval_file(sampling):
    """(file, restart, MCUs) of saturated noise at quality 100 whose intervals 0 and 1 are each longer than one chunk
    of evam_jdec_sync (S * T bits) and whose third and last interval is shorter: the interval length comes from the
    measured bytes per MCU with a twentieth to spare, is more than kJdecDcThreads and no multiple of it, the frame is 32 MCUs wide."""
    if sampling not in _long:
        import jpeg_ref
        from jpeg_content import content

        mw, mh = mcu_size(sampling)
        chunk = source_constant("kJdecSubBits") * source_constant("kJdecChunk") // 8
        per_mcu = len(_scan_array(sampled("sat", 8 * mw, mh, 0, 100, sampling, 0))) // 8
        dc_threads = source_constant("kJdecDcThreads", "evam_jpeg_dec_kernels.h")
        restart = max(chunk * 21 // 20 // per_mcu, dc_threads) + 1
        restart += restart % dc_threads == 0
        rows = -(-(2 * restart + restart // 3) // 32)
        f = jpeg_ref.encode(content("sat", 32 * mw, rows * mh, 5), 100, sampling=sampling, restart=restart)[0]
        _long[sampling] = (f, restart, 32 * rows)
    return _long[sampling]


def damaged_restart_scans():
    """[(name, file bytes, status must be non-zero)] built from the 4:2:2 cut-pairs file, whose second pass holds
    markers and whose FF 00 pair is cut by the first pass border; the two damages of a marker that is cut by a pass
    border are built from the 4:2:0 file, since no 4:2:2 seed has such a marker (CUT_SEEDS)."""
    f, g = cut_pairs_file("422"), cut_pairs_file("420")
    s, _ = scan_bounds(f)
    second = [(k, n) for k, n in rst_markers(f) if PASS <= k < 2 * PASS - 2]
    assert len(second) >= 4
    k, n = second[1]
    out = [("rst_truncated_in_pass_2", f[:s + PASS + PASS // 2], True),
           ("rst_out_of_sequence_in_pass_2", patch(f, s + k + 1, [0xD0 + (n + 1) % 8]), True)]
    sg, _ = scan_bounds(g)
    (cut,) = CUT_SEEDS["420"][2]
    assert g[sg + cut] == 0xFF and 0xD0 <= g[sg + cut + 1] <= 0xD7
    out.append(("rst_on_the_border_removed", g[:sg + cut] + g[sg + cut + 2:], True))
    k, n = second[2]
    out.append(("rst_one_too_many", f[:s + k] + bytes([0xFF, 0xD0 + n]) + f[s + k:], True))
    # the marker's bits become data: an all-ones byte in front of the next interval's first code
    out.append(("rst_on_the_border_stuffed", patch(g, sg + cut + 1, [0]), True))
    return out


def residue_files(sampling, restart, h, widths):
    """[(w, [file at quality 50, file at quality 95])] of random pixels at this height: one row of a residue grid."""
    import jpeg_ref

    rng = np.random.default_rng([SAMPLINGS.index(sampling), restart, h])
    return [(w, [jpeg_ref.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), q, sampling=sampling,
                                 restart=restart)[0] for q in (50, 95)]) for w in widths]


# sampling -> (widths, heights) of its residue grid: every residue of the MCU and of the up-sampling's edge rules
RESIDUE_GRIDS = {"444": (range(1, 18), range(1, 18)), "grey": (range(1, 18), range(1, 18)),
                 "422": (range(1, 34), range(1, 18)), "420": (range(1, 34), range(1, 34))}

WIDE = 2 * 256 * source_constant("kVec", "evam_jpeg_dec_api.h") + 5  # two workgroups of evam_jdec_colour and a tail


def wide_and_tall_files(sampling):
    """[(what, file)]: WIDE x 24 with a marker behind every MCU row, and 24 x 1,100."""
    import jpeg_ref

    per_row = -(-WIDE // mcu_size(sampling)[0])
    return [(f"{WIDE}x24", jpeg_ref.encode(grad_noise(WIDE, 24, 1), 85, sampling=sampling, restart=per_row)[0]),
            ("24x1100", jpeg_ref.encode(grad_noise(24, 1100, 2), 85, sampling=sampling)[0])]


def many_interval_files():
    """[(what, file, restart)]: grey gradients of 2,048 MCUs with a marker behind every MCU and behind every 7th (the
    row holds 64), and a 4:2:0 one of 256 MCUs with a marker behind every MCU."""
    return [("grey 512x256 restart 1", sampled("grad", 512, 256, 0, 50, "grey", 1), 1),
            ("grey 512x256 restart 7", sampled("grad", 512, 256, 0, 50, "grey", 7), 7),
            ("420 256x256 restart 1", sampled("grad", 256, 256, 0, 50, "420", 1), 1)]
