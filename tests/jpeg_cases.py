"""The JPEG files of the jpeg tests, written by Pillow at test time (nothing is committed).  Not a test module.

Content: a gradient plus seeded noise plus hard black / white bars (the bars overshoot the inverse DCT at low quality, so the clamp works).
Matrix: mode L and RGB with subsampling 0 / 1 / 2 (4:4:4, 4:2:2, 4:2:0), quality 10 / 75 / 100, plain / optimize=True (custom Huffman
tables) / restart_marker_rows=1 / restart_marker_blocks=3, at the sizes that pad to whole MCUs differently and reach the first and last
row and column of every upsampler."""
import os

import numpy as np
from PIL import Image

SIZES = ((1, 1), (7, 5), (8, 8), (9, 9), (16, 16), (17, 33), (31, 15), (100, 37))     # (width, height)
MODES = (("L", None), ("RGB", 0), ("RGB", 1), ("RGB", 2))                                # (Pillow mode, subsampling)
MODE_IDS = ("L", "444", "422", "420")
QUALITIES = (10, 75, 100)
VARIANTS = (("plain", {}), ("optimize", {"optimize": True}), ("rst_rows", {"restart_marker_rows": 1}),
            ("rst_blocks", {"restart_marker_blocks": 3}))


def content(w, h, rgb, seed=0):
    rng = np.random.default_rng(seed * 1000003 + w * 1009 + h)
    y, x = np.mgrid[0:h, 0:w]
    a = (x * 255 // max(w - 1, 1) + 3 * y) % 256 + rng.integers(-24, 25, (h, w))
    a[:, w // 3:w // 3 + 2] = 0                                      # hard bars
    a[h // 2:h // 2 + 1, :] = 255
    a = np.clip(a, 0, 255).astype(np.uint8)
    if not rgb:
        return a
    return np.stack([a, np.roll(a, 3, axis=1), 255 - np.roll(a, 2, axis=0)], axis=-1)


def save(path, w, h, mode, subsampling, quality, **kw):
    if subsampling is not None:
        kw["subsampling"] = subsampling
    Image.fromarray(content(w, h, mode == "RGB")).save(path, format="JPEG", quality=quality, **kw)
    return str(path)


def restart_variants(tmp_dir):
    """the restart variants whose keyword this Pillow honours (a DRI segment appears in a 100 x 37 file); a dropped one is printed"""
    kept = []
    for name, kw in VARIANTS:
        if not name.startswith("rst"):
            continue
        try:
            p = save(os.path.join(str(tmp_dir), f"probe_{name}.jpg"), 100, 37, "L", None, 75, **kw)
            ok = b"\xff\xdd\x00\x04" in open(p, "rb").read()
            reason = "the file has no DRI segment"
        except Exception as e:                                       # noqa: BLE001 -- any rejection of the keyword drops the case
            ok, reason = False, repr(e)
        if ok:
            kept.append(name)
        else:
            print(f"jpeg cases: variant {name} dropped: Pillow does not honour {kw}: {reason}")
    assert kept, "no restart marker case is left"
    return kept


def matrix(tmp_dir, mode_index, sizes=SIZES):
    """[(label, path)] of one mode's files"""
    mode, ss = MODES[mode_index]
    rst = restart_variants(tmp_dir)
    out = []
    for (w, h) in sizes:
        for q in QUALITIES:
            for name, kw in VARIANTS:
                if name.startswith("rst") and name not in rst:
                    continue
                label = f"{MODE_IDS[mode_index]}_{w}x{h}_q{q}_{name}"
                out.append((label, save(os.path.join(str(tmp_dir), label + ".jpg"), w, h, mode, ss, q, **kw)))
    return out


def _insert_after_soi(raw, segment):
    assert raw[:2] == b"\xff\xd8"
    return raw[:2] + segment + raw[2:]


def refused_files(tmp_dir):
    """{name: path} of files the device path must leave to Pillow"""
    d = str(tmp_dir)
    out = {}
    rgb = Image.fromarray(content(40, 24, True))
    out["progressive"] = os.path.join(d, "progressive.jpg")
    rgb.save(out["progressive"], quality=75, progressive=True)
    out["cmyk"] = os.path.join(d, "cmyk.jpg")
    rgb.convert("CMYK").save(out["cmyk"], quality=75)
    out["exif_orientation_6"] = os.path.join(d, "orient6.jpg")
    exif = Image.Exif()
    exif[0x0112] = 6
    rgb.save(out["exif_orientation_6"], quality=75, exif=exif)
    plain = os.path.join(d, "plain_for_patching.jpg")
    rgb.save(plain, quality=75, subsampling=0)
    raw = open(plain, "rb").read()
    out["adobe_transform_0"] = os.path.join(d, "adobe0.jpg")
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"      # version 100, flags 0, 0, transform 0
    open(out["adobe_transform_0"], "wb").write(_insert_after_soi(raw, adobe))
    # a 16 x 16 4:2:0 file has one MCU of 4 Y + Cb + Cr blocks: so has a 32 x 8 file with luma sampling 4 x 1 (4:1:1) -- the same scan,
    # a valid stream under the patched frame header
    src = os.path.join(d, "420_16x16.jpg")
    Image.fromarray(content(16, 16, True)).save(src, quality=75, subsampling=2)
    raw = bytearray(open(src, "rb").read())
    sof = raw.index(b"\xff\xc0")
    assert raw[sof + 9] == 3 and raw[sof + 11] == 0x22
    raw[sof + 5:sof + 9] = bytes([0, 8, 0, 32])                      # height 8, width 32
    raw[sof + 11] = 0x41
    out["sampling_411"] = os.path.join(d, "411.jpg")
    open(out["sampling_411"], "wb").write(bytes(raw))
    raw = open(plain, "rb").read()
    sos = raw.index(b"\xff\xda")
    out["truncated"] = os.path.join(d, "truncated.jpg")
    open(out["truncated"], "wb").write(raw[:sos + (len(raw) - sos) // 2])
    return out
