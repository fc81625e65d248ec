"""The device's entropy decode of JPEG scans (csrc/jpeg_huffman_kernels.h) and --device_huffman of run_net_post_processing: the coefficients
computed on the GPU from the unstuffed scan equal the host decoder's bit for bit with status 0, on the matrix of jpeg_cases.py at three
subsequence lengths and on noise pages of many workgroups; damaged scans give a non-zero status or the host's coefficients; a cap of one
round reports "not converged" and the page falls back; the PAGE-XML of the command line does not change with the flags."""
import os
import re
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases  # noqa: E402
import jpeg_huff_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SYNC, SCAN = "jpeg_huff_sync_kernel", "jpeg_huff_scan_kernel"


def _device_coefficients(scan, subseq_bits=0):
    from citlab_article_separation_new_amd import image_io
    d_coef, d_status = image_io.jpeg_scan_entropy_to_device(scan, 0, subseq_bits=subseq_bits)
    return d_coef.cpu().numpy(), int(d_status.cpu()[0])


@pytest.fixture(scope="module")
def matrix_files(tmp_path_factory):
    """{mode index: [(label, prepared scan, the host decoder's coefficients)]}: written and decoded on the host once for the three lengths"""
    from citlab_article_separation_new_amd import image_io
    out = {}
    for m in range(4):
        out[m] = []
        for label, path in jpeg_cases.matrix(tmp_path_factory.mktemp(f"matrix{m}"), m):
            page, scan = image_io.load_jpeg_coefficients(path), image_io.load_jpeg_scan(path)
            assert page is not None and scan is not None, label
            out[m].append((label, scan, page.coef.copy()))
    return out


@pytest.mark.parametrize("subseq_bits", (64, 128, 0))
@pytest.mark.parametrize("mode_index", range(4), ids=jpeg_cases.MODE_IDS)
def test_device_coefficients_equal_the_host_decoders_on_the_matrix(matrix_files, mode_index, subseq_bits):
    """64 bits: even the 17 x 33 file has several subsequences per segment, the gray 1 x 1 file one; the rst_rows variants have segments shorter
    than a subsequence; the 100 x 37 file of quality 100 has symbols across subsequence ends in every component"""
    from citlab_article_separation_new_amd import image_io
    most = (0, 0, "")
    for label, scan, want in matrix_files[mode_index]:
        got, status = _device_coefficients(scan, subseq_bits)
        rounds, subs = image_io.jpeg_entropy_rounds()
        assert status == 0 and got.shape == want.shape and np.array_equal(got, want), \
            f"{label} at {subseq_bits} bits: status {status}, {np.count_nonzero(got != want)} coefficients differ ({subs} subsequences, {rounds} rounds)"
        bits = subseq_bits or 128
        assert subs == sum(-(-int(s["byte_length"]) * 8 // bits) for s in scan.segments), label
        if label.startswith("L_1x1_"):                               # one subsequence: nothing is guessed (a 1 x 1 colour file of quality 100 has two)
            assert subs == scan.n_segments == 1 and rounds == 0, label
        if "17x33" in label and "rst" not in label and subseq_bits == 64:
            assert subs > 2, label
        most = max(most, (rounds, subs, label))
    print(f"{jpeg_cases.MODE_IDS[mode_index]} at {subseq_bits} bits: most rounds {most[0]} over {most[1]} subsequences ({most[2]})")


@pytest.mark.parametrize("mode_index", (0, 3), ids=("L", "420"))
def test_noise_page_of_many_workgroups(tmp_path, mode_index):
    """512 x 384 of uniform noise at quality 100, the default 128 bits: about 200 KB of scan, so more than 10 000 subsequences in about 50
    workgroups of 256 (asserted: more than two), and one segment -- the fixed point has to cross every workgroup boundary"""
    from citlab_article_separation_new_amd import image_io
    rng = np.random.default_rng(5 + mode_index)
    mode, ss = jpeg_cases.MODES[mode_index]
    noise = rng.integers(0, 256, (384, 512) if mode == "L" else (384, 512, 3), dtype=np.uint8)
    path = str(tmp_path / "noise.jpg")
    Image.fromarray(noise).save(path, quality=100, **({} if ss is None else {"subsampling": ss}))
    page, scan = image_io.load_jpeg_coefficients(path), image_io.load_jpeg_scan(path)
    assert page is not None and scan is not None and scan.n_segments == 1
    got, status = _device_coefficients(scan)
    rounds, subs = image_io.jpeg_entropy_rounds()
    groups = -(-subs // 256)
    print(f"{scan.scan_bytes} scan bytes, {subs} subsequences in {groups} workgroups, {rounds} rounds")
    assert groups > 2
    assert status == 0 and np.array_equal(got, page.coef), f"status {status}, {np.count_nonzero(got != page.coef)} coefficients differ"
    d_page, d_status = image_io.jpeg_scan_to_device(scan, 0, "bgr")
    assert int(d_status.cpu()[0]) == 0
    assert np.array_equal(d_page.cpu().numpy(), image_io.load_image_bgr(path))
    names = image_io.jpeg_scan_launches()
    assert names[0] == SYNC + "<speculate>" and SYNC in names and names.count(SCAN + "<place>") == 2 and names.count(SCAN + "<dc>") == 2
    assert names.count("jpeg_huff_carry_kernel") == 2 and "jpeg_huff_write_kernel" in names and "jpeg_huff_energy_kernel" in names
    assert names[-1] == ("jpeg_idct_kernel" if mode_index == 0 else "jpeg_colour_kernel")


@pytest.mark.parametrize("mode_index", (0, 3), ids=("L", "420"))
def test_flipped_scans_are_refused_or_decode_like_the_host(tmp_path, mode_index):
    """300 seeded single-bit flips in the scan of a 100 x 37 file of quality 10 (jpeg_huff_ref.flipped_files; the seed is checked on the CPU, tests/test_jpeg_scan_host.py)"""
    from citlab_article_separation_new_amd import image_io
    mode, ss = jpeg_cases.MODES[mode_index]
    path = jpeg_cases.save(tmp_path / "q10.jpg", 100, 37, mode, ss, 10)
    mutated = str(tmp_path / "m.jpg")
    accepted = refused = 0
    for k, data in enumerate(jpeg_huff_ref.flipped_files(path, mode_index)):
        open(mutated, "wb").write(data)
        page = image_io.load_jpeg_coefficients(mutated)
        scan, _ = image_io.prepare_jpeg_scan(data)
        if scan is None:
            assert page is None, k
            refused += 1
            continue
        got, status = _device_coefficients(scan)
        if page is None:
            assert status != 0, f"flip {k}: the host decoder refuses the file, the device reports status 0"
            refused += 1
        else:
            assert status == 0 and np.array_equal(got, page.coef), f"flip {k}: status {status}"
            accepted += 1
    print(f"{accepted} flips accepted, {refused} refused")
    assert accepted > 0 and refused > 0


def test_a_cap_of_one_round_reports_not_converged_and_the_page_falls_back(tmp_path):
    from citlab_article_separation_new_amd import image_io
    path = jpeg_cases.save(tmp_path / "a.jpg", 100, 37, "RGB", 2, 100)
    scan = image_io.load_jpeg_scan(path)
    assert _device_coefficients(scan, 64)[1] == 0
    image_io.jpeg_entropy_set_max_rounds(1)
    try:
        _one_round_falls_back(path, scan)
    finally:
        image_io.jpeg_entropy_set_max_rounds(0)


def _one_round_falls_back(path, scan):
    from citlab_article_separation_new_amd import image_io
    _, status = _device_coefficients(scan, 64)
    assert status == image_io.JPEG_STATUS_NOT_CONVERGED and image_io.jpeg_entropy_rounds()[0] == 1
    before = image_io.jpeg_huffman_fallbacks
    # 128 bits, the pipeline's length: one round is not enough there either
    (_, image), = image_io.resolve_jpeg_scans([(path, scan.packed)], 0)
    assert image_io.jpeg_huffman_fallbacks == before + 1
    page = image_io.as_jpeg_page(image)                              # what --device_jpeg alone hands out for the file
    assert page is not None
    assert np.array_equal(image_io.jpeg_page_to_device(page, 0, "bgr").cpu().numpy(), image_io.load_image_bgr(path))
    image_io.jpeg_entropy_set_max_rounds(0)
    (_, image), = image_io.resolve_jpeg_scans([(path, scan.packed)], 0)
    assert isinstance(image, image_io.DevicePage) and image_io.jpeg_huffman_fallbacks == before + 1
    assert np.array_equal(image.d_img.cpu().numpy(), image_io.load_image_bgr(path))


def test_host_pointer_form_and_refused_arguments(tmp_path):
    import ctypes as C
    from citlab_article_separation_new_amd import _lib, image_io, image_ops
    path = jpeg_cases.save(tmp_path / "p.jpg", 100, 37, "RGB", 2, 75, restart_marker_blocks=3)
    page, scan = image_io.load_jpeg_coefficients(path), image_io.load_jpeg_scan(path)
    lib, ws = image_ops._workspace(0)
    coef = np.full(page.coef.size, 7, np.int16)
    status = C.c_int32(-1)

    def call(info=scan.info, scan_bytes=scan.scan_bytes, segments=scan.segments, n_segments=scan.n_segments, bits=0):
        return lib.asep_jpeg_entropy(ws, C.byref(info), scan.scan.ctypes.data, scan_bytes, C.byref(scan.tables), segments.ctypes.data,
                                     n_segments, bits, coef.ctypes.data, C.byref(status))
    _lib.check(call(), "asep_jpeg_entropy")
    assert status.value == 0 and np.array_equal(coef, page.coef)
    assert image_io.jpeg_device_launches()[0] == SYNC + "<speculate>"
    for bits in (32, 96 + 8, -64):
        assert call(bits=bits) == -1 and "subseq_bits" in _lib.last_error()
    bad = image_io.JpegInfo.from_buffer_copy(scan.info)
    bad.blocks_w[1] += 1
    assert call(info=bad) == -1 and "contradicts itself" in _lib.last_error()
    assert call(n_segments=scan.n_segments - 1) == -1 and "segments" in _lib.last_error()
    assert call(scan_bytes=scan.scan_bytes - 1) == -1
    moved = scan.segments.copy()
    moved[1]["byte_offset"] += 1
    assert call(segments=moved) == -1 and "does not continue" in _lib.last_error()
    longer = scan.segments.copy()
    longer[-1]["n_mcus"] += 1
    assert call(segments=longer) == -1


def _write_page_xml(path, name, W, H):
    open(path, "w").write(
        '<?xml version="1.0" encoding="UTF-8"?><PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2013-07-15">'
        '<Metadata><Creator>t</Creator><Created>2020-01-01T00:00:00</Created><LastChange>2020-01-01T00:00:00</LastChange></Metadata>'
        f'<Page imageFilename="{name}" imageWidth="{W}" imageHeight="{H}"><TextRegion id="r0"><Coords points="20,20 {W - 20},20 '
        f'{W - 20},{H - 20} 20,{H - 20}"/><TextLine id="l0"><Coords points="30,40 {W - 30},40 {W - 30},80 30,80"/>'
        f'<Baseline points="30,75 {W - 30},75"/></TextLine></TextRegion></Page></PcGts>')


def test_separator_command_line_writes_the_same_page_xml_with_the_flags(tmp_path, capsys):
    """three plain JPEG pages (gray, 4:2:0, one with restart markers), one PNG and one progressive JPEG in one list, inline and with decode
    workers: the flags change no byte of the PAGE-XML, the device decoded exactly the three plain JPEGs and none fell back"""
    from citlab_article_separation_new_amd import image_io, run_net_post_processing, synth
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    import tf_aru_graph
    acfg = AruConfig()
    pb = tmp_path / "net.pb"
    pb.write_bytes(tf_aru_graph.build_aru_pb(init_aru_weights(acfg, 21, bias_jitter=0.05, logit_scale=0.05), acfg))
    W, H = 300, 420
    pages = (("a.jpg", False, {"quality": 90}), ("b.jpg", True, {"quality": 75, "subsampling": 2}),
             ("c.jpg", True, {"quality": 90, "subsampling": 1, "restart_marker_rows": 2}), ("d.png", False, {}),
             ("e.jpg", True, {"quality": 75, "progressive": True}))
    results = {}
    for run, (flags, procs) in {"off": ([], "1"), "inline": (["--device_jpeg", "True", "--device_huffman", "True"], "1"),
                                "workers": (["--device_jpeg", "True", "--device_huffman", "True"], "4")}.items():
        data = tmp_path / run
        (data / "page").mkdir(parents=True)
        names = []
        for i, (name, rgb, kw) in enumerate(pages):
            gray = synth.synth_page(30 + i, W=W + 7 * i, H=H + 5 * i)
            img = np.stack([gray, np.roll(gray, 1, axis=1), gray], axis=-1) if rgb else gray
            Image.fromarray(img).save(data / name, **kw)
            _write_page_xml(data / "page" / (os.path.splitext(name)[0] + ".xml"), name, W + 7 * i, H + 5 * i)
            names.append(str(data / name))
        lst = tmp_path / f"{run}.lst"
        lst.write_text("\n".join(names) + "\n")
        before = image_io.jpeg_huffman_pages, image_io.jpeg_huffman_fallbacks, image_io.jpeg_device_pages
        assert run_net_post_processing.main(["--path_to_image_list", str(lst), "--path_to_pb", str(pb), "--mode", "separator",
                                             "--fixed_height", "200", "--threshold", "0.5", "--num_processes", procs, *flags]) == 0
        assert image_io.jpeg_huffman_pages - before[0] == (3 if flags else 0)
        assert image_io.jpeg_huffman_fallbacks == before[1] and image_io.jpeg_device_pages == before[2]
        if flags:
            assert "device_huffman: 3 pages entropy-decoded on the device, 0 of them fell back" in capsys.readouterr().out
        written = sorted(f for f in os.listdir(data / "page") if f.endswith(".xml.xml"))
        assert len(written) == len(pages), written
        results[run] = [(f, re.sub(rb"<((?:\w+:)?LastChange)>[^<]*</", rb"<\1></", open(data / "page" / f, "rb").read().replace(str(data).encode(), b"")))
                        for f in written]
        assert all(b"Coords" in x for _, x in results[run])
    assert results["inline"] == results["off"]
    assert results["workers"] == results["off"]
