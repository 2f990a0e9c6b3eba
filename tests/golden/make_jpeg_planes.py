"""Writes the fixtures of the JPEG decoder's raw-plane output under tests/golden/jpeg_planes/: small 4:2:0 files
written by Pillow (bundling libjpeg-turbo), and planes.npz with Pillow's raw planes of each of them and of the
even-sized 4:2:0 files that tests/golden/jpeg_dec/ and tests/golden/jpeg/ already hold.

planes.npz keys: "<name>.y" [H, W], "<name>.cb" and "<name>.cr" [H/2, W/2]; <name> is the file's name without ".jpg",
prefixed "dec/" or "enc/" for the files of the two older directories. The planes are jpeg_planes_cases.pillow_planes:
Y from draft("YCbCr", (W, H)), Cb / Cr from draft("YCbCr", (W/2, H/2)), where libjpeg gives 4:2:0 chroma the full 8x8
islow IDCT and no up-sampling.
Run once where Pillow is installed:  python tests/golden/make_jpeg_planes.py
The tests read these files and never need Pillow."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_planes_cases as PC  # noqa: E402
from jpeg_content import content  # noqa: E402

SIZES = ((2, 2), (16, 16), (18, 2), (2, 18), (10, 10), (24, 8), (6, 14), (30, 46), (34, 18), (64, 48), (48, 64))

# name -> (kind, width, height, quality, extra save() arguments)
CASES = {}
for _w, _h in SIZES:
    CASES[f"grad_{_w}x{_h}_q90"] = ("grad", _w, _h, 90, {})
    CASES[f"sat_{_w}x{_h}_q100"] = ("sat", _w, _h, 100, {})
CASES.update({
    "rst1_34x18_q75": ("noise", 34, 18, 75, {"restart_marker_blocks": 1}),
    "rstrow_64x48_q90": ("noise", 64, 48, 90, {"restart_marker_rows": 1}),
    "rstrow_320x180_q75": ("grad", 320, 180, 75, {"restart_marker_rows": 1}),  # the GPU tests' larger restart file
})


def write(name, spec):
    from PIL import Image

    kind, w, h, q, extra = spec
    bgr = content(kind, w, h, seed=sum(name.encode()))
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=q, subsampling=2, **extra)
    data = buf.getvalue()
    assert len(data) <= 64 * 1024, name
    with open(os.path.join(PC.PLANES_DIR, name + ".jpg"), "wb") as f:
        f.write(data)
    return data


def main():
    os.makedirs(PC.PLANES_DIR, exist_ok=True)
    out = {}
    for name, spec in CASES.items():
        out[name] = PC.pillow_planes(write(name, spec))
    for prefix, d in (("dec/", PC.DEC_DIR), ("enc/", PC.ENC_DIR)):
        for fn in sorted(os.listdir(d)):
            if not fn.endswith(".jpg"):
                continue
            data = open(os.path.join(d, fn), "rb").read()
            if PC.header_420_even(data):
                out[prefix + fn[:-4]] = PC.pillow_planes(data)
    flat = {}
    for name, (y, cb, cr) in out.items():
        flat[name + ".y"], flat[name + ".cb"], flat[name + ".cr"] = y, cb, cr
    path = os.path.join(PC.PLANES_DIR, "planes.npz")
    np.savez_compressed(path, **flat)
    print(f"{len(out)} files, planes.npz {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
