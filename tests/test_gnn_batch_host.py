"""The host side of the relation net's pages-per-call path, without a GPU: the page-table builders csrc/launch_plan.h gained
(same_pad3, fmap_dims, fmap_plan, page_unit_table, page_of_unit, arena_offsets) and the parsing of --pages_per_call.

tests/gnn_batch_tables_check.cpp is a stand-alone program (its own main) compiled with the host C++ compiler under the address and
undefined-behaviour sanitizers and run as a child process: nothing sanitized is loaded into Python.  It checks the builders against
brute-force restatements and prints the tables of the sizes it is given, which are compared here with a numpy restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")

# the maps the GPU test's pages (64 x 96, 96 x 64, 71 x 53, 128 x 80) leave at up_1 (half size, rounded up), a single pixel and an empty map
MAPS = [(32, 48), (48, 32), (36, 27), (64, 40), (1, 1), (0, 7)]


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path_factory.mktemp("gnn_batch") / "gnn_batch_tables_check")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), "-I", CSRC, os.path.join(ROOT, "tests", "gnn_batch_tables_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def test_table_builders_hold_against_their_restatements_under_the_sanitizers(check_program):
    ran = subprocess.run([check_program], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.strip().endswith("gnn batch tables ok"), ran.stdout


def _same_pad3(n, stride):
    """TensorFlow's SAME for a 3-tap window by enumeration: one cell per position 0, stride, ... below n; the padding is what the windows'
    span exceeds n by, the front part the largest that does not exceed the part behind (an empty map: as the engine's closed form leaves it)"""
    out = len(range(0, n, stride))
    if out == 0:
        return 0, max(3 - stride - n, 0) // 2
    pad = max((out - 1) * stride + 3 - n, 0)
    return out, max(f for f in range(pad + 1) if f <= pad - f)


@pytest.mark.parametrize("stride,co", [(1, 6), (2, 6), (2, 2)])
def test_tables_of_the_test_pages_equal_the_numpy_restatement(check_program, stride, co):
    args = [str(v) for hw in MAPS for v in hw]
    ran = subprocess.run([check_program, str(stride), str(co), *args], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    lines = ran.stdout.splitlines()
    dims = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("dims")]
    begin = [int(v) for v in next(ln for ln in lines if ln.startswith("begin")).split()[1:]]
    page_of = [int(v) for v in next(ln for ln in lines if ln.startswith("page_of")).split()[1:]]
    want_dims, items = [], []
    for ih, iw in MAPS:
        (oh, pt), (ow, pl) = _same_pad3(ih, stride), _same_pad3(iw, stride)
        want_dims.append([ih, iw, oh, ow, pt, pl])
        items.append(oh * ow * co)
    assert dims == want_dims
    assert want_dims[4][2:4] == [1, 1] and want_dims[5][2] == 0          # the single pixel stays one cell, the empty map stays empty
    units = -(-np.asarray(items) // 256)
    assert begin == [0, *np.cumsum(units).tolist()]
    assert page_of == np.repeat(np.arange(len(MAPS)), units).tolist()    # pages without a unit own no block


def test_pages_per_call_flag_defaults_to_one_and_refuses_zero_and_negatives(capsys):
    from citlab_article_separation_new_amd import lav_rel, run_gnn_clustering
    for mod in (run_gnn_clustering, lav_rel):
        parse = lambda argv: mod.build_parser().parse_known_args(argv)[0]                 # noqa: E731
        assert parse([]).pages_per_call == 1
        assert parse(["--pages_per_call", "3"]).pages_per_call == 3
        for bad in ("0", "-2", "two"):
            with pytest.raises(SystemExit):
                parse(["--pages_per_call", bad])
            err = capsys.readouterr().err
            assert "--pages_per_call" in err and ("at least one page" in err or "whole number" in err), err
