"""csrc/launch_plan.h, the arithmetic of the ARU engine's layer launchers, checked on the host: tests/launch_plan_check.cpp is compiled with the
host C++ compiler under the address and undefined-behaviour sanitizers and run as a child process (no GPU, nothing loaded into Python).  Against
brute-force restatements: the cut of a problem list into launches of at most MAXP, the tile numbering of every tile shape the engine uses on all
pages up to 70 x 70 and on mixed lists, the 1-D block ranges, the padding rule of the one-shot kernels under their block -> unit rule, and the
XCD order of the persistent kernels."""
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


def test_launch_plan_numbers_every_unit_once(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path / "launch_plan_check")
    # the sanitizers' runtimes are linked into the program (clang's default), so that it does not depend on what else the environment loads first
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), "-I", CSRC, os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("launch plan ok:"), ran.stdout
