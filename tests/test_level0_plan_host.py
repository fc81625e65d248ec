"""csrc/level0_plan.h, the page geometry of the level-0 strip walkers, checked on the host: tests/level0_plan_check.cpp is compiled with the
host C++ compiler under the address and undefined-behaviour sanitizers and run as a child process (no GPU, nothing loaded into Python).  It
sweeps the page sizes around the `fits` thresholds and the bench's pyramid levels: the f32s frame units / bf16 border tiles plus the walker's
rectangle cover every pixel, the border bands fit one tile, the band rule yields items that cover the region."""
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


def test_level0_plan_covers_every_page(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path / "level0_plan_check")
    # the sanitizers' runtimes are linked into the program (clang's default), so that it does not depend on what else the environment loads first
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), "-I", CSRC, os.path.join(ROOT, "tests", "level0_plan_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("level0 plan ok:"), ran.stdout
