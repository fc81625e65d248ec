"""csrc/aru_pack.h, the fragment orders in which the ARU-Net kernels read their filters, checked on the host: tests/aru_pack_check.cpp is compiled
with the host C++ compiler under the address and undefined-behaviour sanitizers and run as a child process (no GPU, nothing loaded into Python).
It packs generated filters of every shape that takes another branch of a packer into heap vectors of their exact length, asserts that the
three-part buffers sum back to the fp32 coefficients bit for bit and that every coefficient of the fp32 orders lands as often as its layout says,
and prints a digest of every packed vector.  The digests and the shape-derived integers must equal tests/golden/aru_pack_digests.json, which was
recorded from the packing code before it moved into the header: a digest that differs means the header is wrong, the file is never re-recorded."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_aru_pack_orders_match_recorded_digests(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path / "aru_pack_check")
    # the sanitizers' runtimes are linked into the program (clang's default), so that it does not depend on what else the environment loads first
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), "-I", CSRC, os.path.join(ROOT, "tests", "aru_pack_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-4000:]
    lines = ran.stdout.splitlines()
    assert lines[-1].startswith("aru pack ok:"), ran.stdout[-4000:]
    vectors, ints = {}, {}
    for line in lines[:-1]:
        t = line.split()
        if t[0] == "D":
            assert t[1] not in vectors, line
            vectors[t[1]] = {"count": int(t[2]), "fnv1a64": t[3]}
        else:
            assert t[0] == "I" and t[1] not in ints, line
            ints[t[1]] = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in t[2:]}
    with open(os.path.join(ROOT, "tests", "golden", "aru_pack_digests.json")) as f:
        golden = json.load(f)
    assert ints == golden["ints"]
    assert sorted(vectors) == sorted(golden["vectors"])
    wrong = {k: (v, golden["vectors"][k]) for k, v in vectors.items() if v != golden["vectors"][k]}
    assert not wrong, wrong
