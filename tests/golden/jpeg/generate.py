"""Writes the JPEG golden fixtures: inputs.npz (BGR u8 images keyed by case name) and one <case>.jpg per image, as
Pillow (bundling libjpeg-turbo) encodes it with quality=q, subsampling=2 — the baseline 4:2:0 defaults cv2.imencode
uses. Run once where Pillow is installed:  python tests/golden/jpeg/generate.py
A case name ends in _q<quality>; the tests read the quality from it."""
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def image(kind: str, w: int, h: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "sat":  # every channel 0 or 255
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "grad":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 3) % 256], -1).astype(np.uint8)
    if kind == "checker":  # per-pixel checkerboard
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    if kind == "const":
        return np.broadcast_to(np.array([37, 150, 201], np.uint8), (h, w, 3)).copy()
    raise ValueError(kind)


# (kind, width, height, quality): W and H cover the residues 0, 1, 2, 8, 9, 10 modulo 16 (and a few others)
CASES = [
    ("noise", 1, 1, 75), ("const", 1, 1, 1), ("noise", 8, 8, 50), ("grad", 16, 16, 95), ("noise", 16, 16, 100),
    ("noise", 18, 18, 10), ("grad", 24, 40, 75), ("noise", 26, 10, 95), ("sat", 17, 9, 100), ("noise", 23, 25, 1),
    ("noise", 33, 47, 50), ("grad", 33, 47, 10), ("noise", 41, 16, 75), ("sat", 50, 34, 100), ("noise", 50, 34, 95),
    ("checker", 48, 32, 10), ("const", 48, 32, 95), ("checker", 17, 9, 100), ("noise", 200, 120, 95),
    ("grad", 200, 120, 75), ("sat", 26, 10, 1),
]


def case_name(kind, w, h, q):
    return f"{kind}_{w}x{h}_q{q}"


def main():
    from PIL import Image

    inputs = {}
    for i, (kind, w, h, q) in enumerate(CASES):
        bgr = image(kind, w, h, 1000 + i)
        name = case_name(kind, w, h, q)
        inputs[name] = bgr
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=q, subsampling=2)
        with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
            f.write(buf.getvalue())
    np.savez_compressed(os.path.join(HERE, "inputs.npz"), **inputs)


if __name__ == "__main__":
    main()
