"""asep_jpeg_scan_prepare (csrc/host_jpeg.c) and the five steps of the device's entropy decode restated in Python (tests/jpeg_huff_ref.py),
on the CPU: re-stuffing the prepared bytes and putting the restart markers back gives the file's scan; the fixed point of the
self-synchronising subsequences is the sequential decode, bit for bit, on the whole matrix of jpeg_cases.py at 64 and 128 bits; every
refused file, every prefix and the host-side sanitizer program (tests/host_jpeg_scan_check.c) return success or a refusal."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases  # noqa: E402
import jpeg_huff_ref  # noqa: E402

from citlab_article_separation_new_amd import image_io  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not image_io._host_scan_lib():
        import __graft_entry__ as g
        g.build()
        image_io._host = image_io._host_jpeg = None
    assert image_io._host_scan_lib(), "libasep_host.so with asep_jpeg_scan_prepare"


def _scan_of_file(raw):
    """the entropy-coded bytes of the file's one scan, markers and stuffing included, up to EOI"""
    sos = raw.index(b"\xff\xda")
    first = sos + 2 + int.from_bytes(raw[sos + 2:sos + 4], "big")
    assert raw[-2:] == b"\xff\xd9"
    return raw[first:-2]


def _restuffed(scan):
    out = b""
    for i, seg in enumerate(scan.segments):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        b = bytes(scan.scan[int(seg["byte_offset"]):int(seg["byte_offset"]) + int(seg["byte_length"])])
        out += b.replace(b"\xff", b"\xff\x00")
    return out


@pytest.mark.parametrize("mode_index", range(4), ids=jpeg_cases.MODE_IDS)
def test_prepared_scan_is_the_files_scan(tmp_path, mode_index):
    lib = image_io._host_scan_lib()
    restarts = 0
    for label, path in jpeg_cases.matrix(tmp_path, mode_index):
        raw = open(path, "rb").read()
        scan, rc = image_io.prepare_jpeg_scan(raw)
        assert rc == 0 and scan is not None, label
        info = scan.info
        cap, nseg = C.c_size_t(), C.c_size_t()
        assert lib.asep_jpeg_scan_sizes(C.byref(info), len(raw), C.byref(cap), C.byref(nseg)) == 0
        assert scan.n_segments == nseg.value and scan.scan_bytes <= cap.value and cap.value % 4 == 0, label
        assert _restuffed(scan) == _scan_of_file(raw), label
        assert not scan.scan[scan.scan_bytes:].any() and scan.scan.size % 4 == 0, label
        mcus, ri = info.mcus_w * info.mcus_h, info.restart_interval
        want = [(k * ri, min(ri, mcus - k * ri)) for k in range(-(-mcus // ri))] if ri else [(0, mcus)]
        assert [(int(s["first_mcu"]), int(s["n_mcus"])) for s in scan.segments] == want, label
        restarts += ri > 0
        page = image_io.load_jpeg_coefficients(path)
        assert np.array_equal(scan.qt, page.qt) and bytes(scan.info) == bytes(page.info), label
        assert image_io.as_jpeg_scan(scan.packed) is not None and image_io.as_jpeg_page(scan.packed) is None
        assert image_io.as_jpeg_scan(page.packed) is None
        assert image_io.load_jpeg_scan(path).packed.tobytes() == scan.packed.tobytes()
    assert restarts >= 8 * 3


def test_sizes_and_arguments_are_checked(tmp_path):
    lib = image_io._host_scan_lib()
    path = jpeg_cases.save(tmp_path / "a.jpg", 100, 37, "RGB", 2, 75, restart_marker_blocks=3)
    raw = open(path, "rb").read()
    scan, _ = image_io.prepare_jpeg_scan(raw)
    tables = image_io.JpegScanTables()
    segs = np.zeros(scan.n_segments, image_io.JPEG_SEGMENT)
    buf = np.zeros(len(raw) + 4, np.uint8)
    used, got = C.c_size_t(7), C.c_size_t(7)

    def prepare(cap, max_segments, info=scan.info):
        return lib.asep_jpeg_scan_prepare(raw, len(raw), C.byref(info), buf.ctypes.data, cap, C.byref(used), segs.ctypes.data, max_segments,
                                          C.byref(got), C.byref(tables))
    assert prepare(buf.size, scan.n_segments) == 0 and used.value == scan.scan_bytes and got.value == scan.n_segments
    assert prepare(scan.scan_bytes - 1, scan.n_segments) == -3 and used.value == 0 and got.value == 0      # too small a buffer: ASEP_JPEG_ARG
    assert prepare(buf.size, scan.n_segments - 1) == -3
    other = image_io.JpegInfo.from_buffer_copy(scan.info)
    other.width += 1
    assert prepare(buf.size, scan.n_segments, other) == -3                                                   # not the probe of these bytes


def test_refused_files_are_refused_with_the_host_decoders_code(tmp_path):
    lib = image_io._host_jpeg_lib()
    for name, path in jpeg_cases.refused_files(tmp_path).items():
        raw = open(path, "rb").read()
        info = image_io.JpegInfo()
        rc = lib.asep_jpeg_probe(raw, len(raw), C.byref(info))
        if rc == 0:
            coef = np.zeros(info.coef_bytes // 2, np.int16)
            qt = np.zeros((4, 64), np.uint16)
            rc = lib.asep_jpeg_entropy_decode(raw, len(raw), C.byref(info), coef.ctypes.data, qt.ctypes.data)
        assert rc < 0, name
        scan, got = image_io.prepare_jpeg_scan(raw)
        assert scan is None and got == rc, (name, got, rc)
        assert image_io.load_jpeg_scan(path) is None, name


def test_every_prefix_is_an_error(tmp_path):
    files = (jpeg_cases.save(tmp_path / "g.jpg", 17, 33, "L", None, 75), jpeg_cases.save(tmp_path / "c.jpg", 31, 15, "RGB", 2, 75),
             jpeg_cases.save(tmp_path / "r.jpg", 31, 15, "RGB", 1, 75, restart_marker_blocks=1))
    for path in files:
        raw = open(path, "rb").read()
        assert image_io.prepare_jpeg_scan(raw)[1] == 0
        for k in range(len(raw)):
            scan, rc = image_io.prepare_jpeg_scan(raw[:k])
            assert scan is None and rc in (-1, -2), (path, k, rc)


@pytest.fixture(scope="module")
def round_log():
    return []


@pytest.mark.parametrize("subseq_bits", (64, 128))
@pytest.mark.parametrize("mode_index", range(4), ids=jpeg_cases.MODE_IDS)
def test_fixed_point_is_the_sequential_decode(tmp_path, mode_index, subseq_bits, round_log):
    for label, path in jpeg_cases.matrix(tmp_path, mode_index):
        page = image_io.load_jpeg_coefficients(path)
        scan = image_io.load_jpeg_scan(path)
        coef, status, rounds, longest = jpeg_huff_ref.entropy_decode(scan, subseq_bits)
        assert status == 0 and np.array_equal(coef, page.coef), (label, status, rounds, longest)
        round_log.append((rounds, longest, label, subseq_bits))
        # the cap is longest + 1 rounds: correctness moves one subsequence forward per round, so `longest` rounds are the most a file can
        # take, the confirming round included, and the cap leaves one more
        assert rounds <= longest < jpeg_huff_ref.round_cap(longest), (label, rounds, longest)
    worst = max(r for r in round_log if r[3] == subseq_bits)
    print(f"subseq_bits {subseq_bits}, {jpeg_cases.MODE_IDS[mode_index]}: most rounds so far {worst[0]} at {worst[1]} subsequences ({worst[2]})")


def test_a_cap_of_one_round_does_not_converge(tmp_path):
    path = jpeg_cases.save(tmp_path / "a.jpg", 100, 37, "RGB", 2, 100)
    scan = image_io.load_jpeg_scan(path)
    _, status, rounds, longest = jpeg_huff_ref.entropy_decode(scan, 64, max_rounds=1)
    assert status == jpeg_huff_ref.NOT_CONVERGED and rounds == 1 and longest > 8


@pytest.mark.parametrize("mode_index", (0, 3), ids=("L", "420"))
def test_flip_seed_keeps_both_outcomes(tmp_path, mode_index):
    """the seeded single-bit flips of the GPU test (tests/test_jpeg_huffman_gpu.py), judged by the host decoder alone: between a quarter and
    three quarters stay accepted, and the reference decode of every flipped file agrees with the host decoder's verdict"""
    mode, ss = jpeg_cases.MODES[mode_index]
    path = jpeg_cases.save(tmp_path / "q10.jpg", 100, 37, mode, ss, 10)
    accepted = 0
    for data in jpeg_huff_ref.flipped_files(path, mode_index):
        mutated = str(tmp_path / "m.jpg")
        open(mutated, "wb").write(data)
        page = image_io.load_jpeg_coefficients(mutated)
        accepted += page is not None
        scan, rc = image_io.prepare_jpeg_scan(data)
        if scan is None:
            assert page is None
            continue
        coef, status, _, _ = jpeg_huff_ref.entropy_decode(scan, 128)
        assert (status == 0) == (page is not None), (status, rc)
        if page is not None:
            assert np.array_equal(coef, page.coef)
    print(f"{accepted} of {jpeg_huff_ref.FLIPS} flips accepted")
    assert jpeg_huff_ref.FLIPS // 4 <= accepted <= 3 * jpeg_huff_ref.FLIPS // 4


def _host_compiler():
    for name in (os.environ.get("CC"), "gcc", "cc", "clang"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_scan_prepare_under_the_sanitizers(tmp_path):
    """tests/host_jpeg_scan_check.c + host_jpeg.c as a stand-alone program with the address and undefined-behaviour sanitizers linked in:
    the matrix files, every prefix of them and 2000 single-byte mutations; nothing is loaded into Python"""
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C compiler (gcc, cc or clang) on PATH")
    exe = str(tmp_path / "host_jpeg_scan_check")
    is_clang = "clang" in subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
    cmd = [cc, "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), os.path.join(ROOT, "tests", "host_jpeg_scan_check.c"),
           os.path.join(CSRC, "host_jpeg.c"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    files = [p for m in range(4) for _, p in jpeg_cases.matrix(tmp_path, m)]
    ran = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    words = ran.stdout.replace(",", "").split()
    assert ran.stdout.startswith("host jpeg scan ok:") and "Sanitizer" not in ran.stderr, ran.stdout + ran.stderr
    n_files, n_prefixes, n_mutations = (int(words[words.index(k) - 1]) for k in ("files", "prefixes", "mutations"))
    assert n_files == len(files) and n_prefixes == sum(os.path.getsize(p) for p in files) and n_mutations == 2000


def test_device_huffman_is_off_by_default_and_refused_without_device_jpeg(tmp_path, capsys):
    from citlab_article_separation_new_amd import run_net_post_processing
    base = ["--path_to_image_list", str(tmp_path / "l"), "--path_to_pb", "p", "--mode", "separator"]
    args = run_net_post_processing.build_parser().parse_args(base)
    assert args.device_huffman is False and args.device_jpeg is False
    with pytest.raises(SystemExit) as e:
        run_net_post_processing.main(base + ["--device_huffman", "True"])
    assert e.value.code == 2
    assert "--device_huffman True needs --device_jpeg True" in capsys.readouterr().err
