"""csrc/host_jpeg.c under the address and undefined-behaviour sanitizers: tests/host_jpeg_check.c and host_jpeg.c are compiled with the host C
compiler into a stand-alone program that runs as a child process (no GPU, nothing loaded into Python) over the files of the matrix, over
every prefix of one small colour file and over 2000 seeded single-byte mutations of it.  It must exit 0 without a sanitizer report, and
every call must return success or a refusal."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")


def _host_compiler():
    for name in (os.environ.get("CC"), "gcc", "cc", "clang"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C compiler (gcc, cc or clang) on PATH")
    exe = str(tmp_path_factory.mktemp("host_jpeg") / "host_jpeg_check")
    # the sanitizers' runtimes are linked into the program (clang's default), so that it does not depend on what else the environment loads first
    is_clang = "clang" in subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
    cmd = [cc, "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), os.path.join(ROOT, "tests", "host_jpeg_check.c"),
           os.path.join(CSRC, "host_jpeg.c"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def test_matrix_files_decode_clean(checker, tmp_path):
    files = [p for m in range(4) for _, p in jpeg_cases.matrix(tmp_path, m)]
    ran = subprocess.run([checker] + files, capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith(f"host jpeg ok: files, {len(files)} accepted, 0 refused"), ran.stdout
    refused = list(jpeg_cases.refused_files(tmp_path).values())
    for path in refused:                                             # refused, not faulted
        ran = subprocess.run([checker, path], capture_output=True, text=True, timeout=60)
        assert ran.returncode == 1 and "is not accepted" in ran.stderr and "Sanitizer" not in ran.stderr, ran.stdout + ran.stderr


def test_prefixes_and_mutations_return_success_or_refusal(checker, tmp_path):
    small = jpeg_cases.save(tmp_path / "small.jpg", 31, 15, "RGB", 2, 75, restart_marker_blocks=1)
    ran = subprocess.run([checker, "--fuzz", small], capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("host jpeg ok: fuzz,"), ran.stdout
    accepted, refused = (int(w) for w in ran.stdout.replace(",", "").split() if w.isdigit())
    assert accepted + refused == 1 + os.path.getsize(small) + 2000
    assert accepted >= 100 and refused >= os.path.getsize(small), ran.stdout     # mutations of coefficient bits still decode; prefixes never do
