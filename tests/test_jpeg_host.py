"""csrc/host_jpeg.c (libasep_host.so) and tests/jpeg_ref.py, on the CPU: the Huffman decode of every file of the matrix (jpeg_cases.py),
pushed through the numpy restatement of libjpeg-turbo's inverse DCT, fancy upsampling and colour conversion, equals what Pillow
decodes bit for bit -- so the restatement the device kernels are written against is the judge's arithmetic -- and every flavour the
path does not take gives None and is decoded by load_image_bgr as before."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases  # noqa: E402
import jpeg_ref  # noqa: E402

from citlab_article_separation_new_amd import image_io  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not image_io._host_jpeg_lib():
        import __graft_entry__ as g
        g.build()
        image_io._host = image_io._host_jpeg = None
    assert image_io._host_jpeg_lib(), "libasep_host.so with the JPEG entry points"


def test_host_jpeg_header_symbols_are_exported(repo_root):
    src = open(os.path.join(repo_root, "include", "asep_host_jpeg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(asep_[a-z0-9_]+)\s*\(", src))
    assert names == {"asep_jpeg_probe", "asep_jpeg_entropy_decode"}
    assert '#include "asep_host_jpeg.h"' in open(os.path.join(repo_root, "include", "asep_host.h")).read()
    lib = image_io._host_jpeg_lib()
    for n in names:
        assert hasattr(lib, n)
    # the ctypes mirror of asep_jpeg_info: 18 int32 and one int64, no padding
    assert C.sizeof(image_io.JpegInfo) == 80 and image_io.JpegInfo.coef_bytes.offset == 72


@pytest.mark.parametrize("mode_index", range(4), ids=jpeg_cases.MODE_IDS)
def test_restatement_of_the_coefficients_equals_pillow(tmp_path, mode_index):
    cases = jpeg_cases.matrix(tmp_path, mode_index)
    assert len(cases) >= 8 * 3 * 3
    restarts = 0
    for label, path in cases:
        page = image_io.load_jpeg_coefficients(path)
        assert page is not None, label
        ref = np.asarray(Image.open(path))
        assert (page.width, page.height) == (ref.shape[1], ref.shape[0]), label
        assert page.ncomp == (1 if mode_index == 0 else 3) and (page.hs, page.vs) == ((1, 1), (1, 1), (2, 1), (2, 2))[mode_index], label
        restarts += page.info.restart_interval > 0
        got = jpeg_ref.pixels(page, "rgb")
        assert got.shape == ref.shape and np.array_equal(got, ref), f"{label}: max |diff| {np.abs(got.astype(int) - ref).max()}"
        bgr = image_io.load_image_bgr(path)
        assert np.array_equal(jpeg_ref.pixels(page, "bgr"), bgr), label
        assert np.array_equal(jpeg_ref.pixels(page, "gray"), image_io.load_image_gray(path)), label
    assert restarts >= 8 * 3, "the restart marker cases carry a restart interval"


def test_coefficient_layout(tmp_path):
    """natural order, DC prediction undone, blocks padded to whole MCUs: a flat gray page has one DC value in every block and nothing else"""
    p = str(tmp_path / "flat.jpg")
    Image.fromarray(np.full((20, 33), 200, np.uint8)).save(p, quality=100)
    page = image_io.load_jpeg_coefficients(p)
    (y,) = page.components()
    assert y.shape == (3, 5, 64) and page.coef.size * 2 == page.info.coef_bytes
    assert np.all(y[:, :, 0] == (200 - 128) * 8) and not y[:, :, 1:].any()
    assert page.qt.shape == (4, 64) and np.all(page.qt[page.qt_index[0]] == 1)
    p2 = str(tmp_path / "ramp.jpg")
    Image.fromarray(np.tile(np.arange(0, 256, 8, dtype=np.uint8), (8, 1))).save(p2, quality=100)       # varies along x only
    (y,) = image_io.load_jpeg_coefficients(p2).components()
    blk = y[0, 0].reshape(8, 8)
    assert blk[0, 1:].any() and not blk[1:, :].any(), "horizontal frequencies sit in the first ROW of a natural-order block"


def test_orientation_1_and_plain_app_segments_are_accepted(tmp_path):
    exif = Image.Exif()
    exif[0x0112] = 1
    p = str(tmp_path / "orient1.jpg")
    Image.fromarray(jpeg_cases.content(40, 24, True)).save(p, quality=75, exif=exif, comment=b"scanned")
    page = image_io.load_jpeg_coefficients(p)
    assert page is not None
    assert np.array_equal(jpeg_ref.pixels(page, "bgr"), image_io.load_image_bgr(p))


def test_refused_files_go_to_pillow_as_before(tmp_path):
    files = jpeg_cases.refused_files(tmp_path)
    assert set(files) == {"progressive", "cmyk", "exif_orientation_6", "adobe_transform_0", "sampling_411", "truncated"}
    lib = image_io._host_jpeg_lib()
    for name, path in files.items():
        assert image_io.load_jpeg_coefficients(path) is None, name
        raw = open(path, "rb").read()
        info = image_io.JpegInfo()
        rc = lib.asep_jpeg_probe(raw, len(raw), C.byref(info))
        if name == "truncated":                                      # the header is fine: the scan runs out
            assert rc == 0
            coef = np.full(info.coef_bytes // 2, 7, np.int16)
            qt = np.full((4, 64), 7, np.uint16)
            assert lib.asep_jpeg_entropy_decode(raw, len(raw), C.byref(info), coef.ctypes.data, qt.ctypes.data) == -2
            assert not coef.any() and not qt.any(), "no partial output"
            with pytest.raises(OSError):
                image_io.load_image_bgr(path)
            with pytest.raises(OSError):
                image_io.load_image_bgr_or_jpeg(path)
            continue
        assert rc == -1 and info.width == 0 and info.coef_bytes == 0, name
        today = image_io.load_image_bgr(path)
        assert np.array_equal(image_io.load_image_bgr_or_jpeg(path), today), name
    # what "today" means for the rotated file: the orientation is applied
    assert image_io.load_image_bgr(files["exif_orientation_6"]).shape == (40, 24, 3)
    assert image_io.load_image_bgr(files["sampling_411"]).shape == (8, 32, 3)
    for other in (tmp_path / "page.png", tmp_path / "missing.jpg"):
        if other.name == "page.png":
            Image.fromarray(jpeg_cases.content(9, 9, False)).save(other)
        assert image_io.load_jpeg_coefficients(str(other)) is None


def test_a_header_cannot_size_anything_alone(tmp_path):
    """a frame header that announces 65535 x 65535 over a few hundred bytes of scan is refused by the probe, before any buffer exists"""
    p = str(tmp_path / "small.jpg")
    Image.fromarray(jpeg_cases.content(16, 16, False)).save(p, quality=75)
    raw = bytearray(open(p, "rb").read())
    sof = raw.index(b"\xff\xc0")
    raw[sof + 5:sof + 9] = b"\xff\xff\xff\xff"
    info = image_io.JpegInfo()
    assert image_io._host_jpeg_lib().asep_jpeg_probe(bytes(raw), len(raw), C.byref(info)) == -2
    open(p, "wb").write(bytes(raw))
    assert image_io.load_jpeg_coefficients(p) is None


def _differences_from_pillow(path, n_flips, seed):
    """single-bit flips in the scan of ``path``: (accepted, [those whose restated pixels differ from what Pillow decodes])"""
    raw = open(path, "rb").read()
    first = raw.index(b"\xff\xda") + 2 + int.from_bytes(raw[raw.index(b"\xff\xda") + 2:raw.index(b"\xff\xda") + 4], "big")
    rng = np.random.default_rng(seed)
    mutated = path + ".mutated.jpg"
    accepted, differing = 0, []
    for _ in range(n_flips):
        at, bit = int(rng.integers(first, len(raw) - 2)), int(rng.integers(0, 8))
        data = bytearray(raw)
        data[at] ^= 1 << bit
        open(mutated, "wb").write(bytes(data))
        page = image_io.load_jpeg_coefficients(mutated)
        if page is None:
            continue
        accepted += 1
        try:
            ref = np.asarray(Image.open(mutated))
        except OSError:
            differing.append((at, bit, "Pillow refuses the file"))
            continue
        got = jpeg_ref.pixels(page, "rgb")
        if got.shape != ref.shape or not np.array_equal(got, ref):
            differing.append((at, bit, int(np.abs(got.astype(int) - ref).max())))
    return accepted, differing


@pytest.mark.parametrize("mode_index", (0, 3), ids=("L", "420"))
def test_every_accepted_mutation_decodes_like_pillow(tmp_path, mode_index):
    """3000 seeded single-bit flips in the scan of a 100 x 37 file of quality 10 (large table entries, so a flipped bit makes large
    dequantised coefficients): a flipped file is refused or gives Pillow's bytes.  Coefficients beyond what 8-bit samples give leave
    the 16-bit lanes of libjpeg-turbo's SIMD inverse DCT, where it and wide integers part: host_jpeg.c refuses such blocks."""
    mode, ss = jpeg_cases.MODES[mode_index]
    path = jpeg_cases.save(tmp_path / "q10.jpg", 100, 37, mode, ss, 10)
    accepted, differing = _differences_from_pillow(path, 3000, 7 + mode_index)
    print(f"{accepted} of 3000 flips accepted, {len(differing)} differ from Pillow")
    assert accepted >= 500, "the bound still accepts the harmless mutations"
    assert not differing, differing[:10]


def test_short_jfif_app0_does_not_count(tmp_path):
    """libjpeg takes an APP0 of fewer than 14 data bytes for no JFIF marker: with component ids R G B such a file is RGB, not YCbCr"""
    p = str(tmp_path / "rgb_ids.jpg")
    Image.fromarray(jpeg_cases.content(16, 16, True)).save(p, quality=75, subsampling=0)
    raw = bytearray(open(p, "rb").read())
    app0 = raw.index(b"\xff\xe0")
    assert raw[app0 + 4:app0 + 9] == b"JFIF\0" and raw[app0 + 2:app0 + 4] == b"\x00\x10"
    raw[app0:app0 + 18] = b"\xff\xe0\x00\x0fJFIF\0\x01\x01\x00\x00\x01\x00\x01\x00"          # 13 data bytes: one short of a JFIF marker
    sof = raw.index(b"\xff\xc0")
    sos = raw.index(b"\xff\xda")
    for k, ident in enumerate(b"RGB"):
        raw[sof + 10 + 3 * k] = ident
        raw[sos + 5 + 2 * k] = ident
    open(p, "wb").write(bytes(raw))
    assert image_io.load_jpeg_coefficients(p) is None
    assert np.array_equal(image_io.load_image_bgr_or_jpeg(p), image_io.load_image_bgr(p))


def test_a_library_without_the_jpeg_symbols_keeps_the_png_path(tmp_path, monkeypatch):
    class Old:
        def __init__(self, lib):
            self.asep_png_unfilter, self.asep_rgb_to_bgr = lib.asep_png_unfilter, lib.asep_rgb_to_bgr
    monkeypatch.setattr(image_io, "_host", Old(image_io._host_lib()))
    monkeypatch.setattr(image_io, "_host_jpeg", None)
    p = jpeg_cases.save(tmp_path / "a.jpg", 16, 16, "L", None, 75)
    assert image_io.load_jpeg_coefficients(p) is None
    png = str(tmp_path / "a.png")
    Image.fromarray(jpeg_cases.content(16, 16, True)).save(png)
    assert image_io._load_png_plain(png) is not None


def test_flag_is_off_by_default():
    from citlab_article_separation_new_amd.run_net_post_processing import build_parser
    base = ["--path_to_image_list", "l", "--path_to_pb", "p", "--mode", "separator"]
    assert build_parser().parse_args(base).device_jpeg is False
    assert build_parser().parse_args(base + ["--device_jpeg", "True"]).device_jpeg is True
