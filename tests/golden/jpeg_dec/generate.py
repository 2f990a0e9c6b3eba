"""Writes the JPEG decoder's golden fixtures: one <case>.jpg per case, written by Pillow (bundling libjpeg-turbo), and
pixels.npz with Pillow's own decode of each file as an [H, W, 3] uint8 BGR image keyed by case name (a grey file's
three channels are equal). progressive_16x16.jpg is a file the decoder refuses: it has no pixels entry.
encoder_pixels.npz holds Pillow's decode of the 21 files of tests/golden/jpeg/ (the encoder's fixtures) likewise.
Run once where Pillow is installed:  python tests/golden/jpeg_dec/generate.py
The tests read these files and never import Pillow."""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from jpeg_content import content  # noqa: E402

SAMPLING = {"444": 0, "422": 1, "420": 2, "grey": None}

# name -> (kind, width, height, quality, sampling, extra save() arguments)
CASES = {}
for _s in SAMPLING:
    for _w in range(1, 7):  # the chroma-width <= 2 rule: replication instead of the fancy filter
        CASES[f"w{_w}_{_s}"] = ("noise", _w, 5, 90, _s, {})
    CASES[f"noise_64x48_{_s}"] = ("noise", 64, 48, 90, _s, {})
CASES.update({
    "optimize_48x32_420": ("noise", 48, 32, 100, "420", {"optimize": True}),
    "optimize_48x32_444": ("sat", 48, 32, 100, "444", {"optimize": True}),
    "rst1_33x17_420": ("noise", 33, 17, 75, "420", {"restart_marker_blocks": 1}),
    "rst3_40x24_422": ("noise", 40, 24, 75, "422", {"restart_marker_blocks": 3}),
    "rstrow_64x48_444": ("halves", 64, 48, 50, "444", {"restart_marker_rows": 1}),
    "rstwrap_64x48_420": ("noise", 64, 48, 90, "420", {"restart_marker_blocks": 1}),  # 12 intervals: RST0..7 wraps
    "rst1_24x16_grey": ("noise", 24, 16, 90, "grey", {"restart_marker_blocks": 1}),
    "exif_com_16x16_420": ("grad", 16, 16, 75, "420",
                           {"exif": b"Exif\x00\x00MM\x00\x2a\x00\x00\x00\x08\x00\x00\x00\x00\x00\x00",
                            "comment": b"a comment segment"}),
    "grad_64x48_q10_420": ("grad", 64, 48, 10, "420", {}),
    "const_17x9_422": ("const", 17, 9, 95, "422", {}),
    "sat_31x23_q100_422": ("sat", 31, 23, 100, "422", {}),
    "blocks_48x32_q100_420": ("blocks", 48, 32, 100, "420", {}),
    "checker_33x33_q1_444": ("checker", 33, 33, 1, "444", {}),
})
REFUSED = {"progressive_16x16": ("grad", 16, 16, 75, "420", {"progressive": True})}


def write(name, spec):
    from PIL import Image

    kind, w, h, q, samp, extra = spec
    bgr = content(kind, w, h, seed=sum(name.encode()))
    if samp == "grey":
        im, args = Image.fromarray(np.ascontiguousarray(bgr[..., 1])), {}
    else:
        im, args = Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])), {"subsampling": SAMPLING[samp]}
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=q, **args, **extra)
    data = buf.getvalue()
    assert len(data) <= 64 * 1024, name
    with open(os.path.join(HERE, name + ".jpg"), "wb") as f:
        f.write(data)
    return data


def main():
    from PIL import Image

    pixels = {}
    for name, spec in CASES.items():
        data = write(name, spec)
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        pixels[name] = np.ascontiguousarray(rgb[..., ::-1])
    for name, spec in REFUSED.items():
        write(name, spec)
    np.savez_compressed(os.path.join(HERE, "pixels.npz"), **pixels)
    enc_dir = os.path.join(os.path.dirname(HERE), "jpeg")
    enc = {}
    for fn in sorted(os.listdir(enc_dir)):
        if fn.endswith(".jpg"):
            rgb = np.asarray(Image.open(os.path.join(enc_dir, fn)).convert("RGB"))
            enc[fn[:-4]] = np.ascontiguousarray(rgb[..., ::-1])
    np.savez_compressed(os.path.join(HERE, "encoder_pixels.npz"), **enc)


if __name__ == "__main__":
    main()
