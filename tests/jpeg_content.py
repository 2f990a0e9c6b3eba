"""Frame contents of the JPEG tests: [H, W, 3] uint8 BGR images chosen for what they make the entropy coder do.
tests/test_jpeg_host.py asserts on the reference alone (``jpeg_ref.encode``'s stats) what each kind is used for, so the
GPU tests' preconditions are known to hold without a device."""
import numpy as np

KINDS = ("noise", "sat", "grad", "const", "checker", "lowchecker", "blocks", "halves")

# (kind, width, height, seed, quality) of the frames test_arbitrary_cut truncates at dst_stride in
# {625, L-3, L-2, L-1, L, L+1} (L: the file's length). The seeds were searched on the reference so that a cut falls
# between a stuffed 0xFF and its 0x00: the noise file's last scan byte is a stuffed 0xFF (stride L-3 keeps the 0xFF and
# drops the 0x00), the saturated file's second scan byte is one (stride 625 = header + 2). Stride L-1 cuts every file
# between the 0xFF and the 0xD9 of EOI.
CUT_FRAMES = (("noise", 200, 120, 1, 95), ("sat", 50, 34, 8, 100), ("const", 48, 32, 0, 95))


def cut_strides(length):
    return (625, length - 3, length - 2, length - 1, length, length + 1)


def content(kind, w, h, seed=0):
    """noise: uniform bytes. sat: every channel 0 or 255. checker: per-pixel 0 / 255. lowchecker: per-pixel 88 / 168
    (128 +- 40: at low quality only coefficient 63 survives). blocks: 8x8 blocks alternately all 0 and all 255 (DC
    differences of category 11 at quality 100). const: one colour. halves: the left and right halves differ in kind.
    Anything else: a gradient."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]

    def grey(a):
        return np.repeat(a.astype(np.uint8)[..., None], 3, -1)

    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "sat":
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "checker":
        return grey(((x + y) & 1) * 255)
    if kind == "lowchecker":
        return grey(88 + ((x + y) & 1) * 80)
    if kind == "blocks":
        return grey((((x >> 3) + (y >> 3)) & 1) * 255)
    if kind == "const":
        return np.broadcast_to(np.array([37, 150, 201], np.uint8), (h, w, 3)).copy()
    if kind == "halves":
        a, b = (KINDS[int(k)] for k in rng.choice(len(KINDS) - 1, 2, replace=False))
        out = content(a, w, h, seed + 1)
        out[:, w // 2:] = content(b, w, h, seed + 2)[:, w // 2:]
        return out
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 3) % 256], -1).astype(np.uint8)
