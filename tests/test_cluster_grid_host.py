"""Host side of the clustering grid: numpy's mean as restated by csrc/cluster_grid_kernels.h (np_mean, compiled with the host
C++ compiler into a stand-alone program and compared bit for bit with np.mean), the command lines' argument parsing and the grid
range syntax, and ClusterGrid without a GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")
sys.path.insert(0, ROOT)

WIDTH = 300


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def sum_check(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path_factory.mktemp("clg") / "cluster_grid_sum_check")
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC,
                            os.path.join(ROOT, "tests", "cluster_grid_sum_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def _rows(dtype):
    rng = np.random.default_rng(20240)
    dt = np.dtype(dtype)
    ties = np.array([0.25, 0.5, 0.75, np.nextafter(dt.type(0), dt.type(1)), np.nextafter(dt.type(1), dt.type(0))], dt)
    rows = [rng.random(WIDTH), rng.uniform(0.55, 0.999, WIDTH), rng.random(WIDTH) * 1e-3,
            rng.choice(ties, WIDTH), rng.choice(ties, WIDTH), np.full(WIDTH, 0.5),
            np.where(rng.random(WIDTH) < 0.5, rng.choice(ties, WIDTH), rng.random(WIDTH))]
    return np.ascontiguousarray(np.stack(rows).astype(dt))


@pytest.mark.parametrize("dtype,flag", [("float32", "f32"), ("float64", "f64")])
def test_np_mean_bit_patterns(sum_check, tmp_path, dtype, flag):
    rows = _rows(dtype)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rows.tofile(src)
    ran = subprocess.run([sum_check, flag, src, dst, str(WIDTH)], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0 and ran.stdout.startswith("cluster grid sum ok:"), ran.stdout + ran.stderr
    got = np.fromfile(dst, dtype).reshape(len(rows), WIDTH)
    bits = np.uint32 if dtype == "float32" else np.uint64
    for r, row in enumerate(rows):
        want = np.array([np.mean(row[:n]) for n in range(1, WIDTH + 1)])
        assert want.dtype == np.dtype(dtype)
        bad = np.flatnonzero(got[r].view(bits) != want.view(bits))
        assert bad.size == 0, f"row {r}, lengths {bad[:8] + 1}: {got[r][bad[:8]]} != {want[bad[:8]]}"


def test_threshold_comparison_rule():
    """what the kernel assumes: numpy compares a float32 array / scalar with a Python float in float32"""
    thr = 0.6
    t32 = np.float32(thr)
    around = np.array([np.nextafter(t32, np.float32(0)), t32, np.nextafter(t32, np.float32(1))], np.float32)
    assert (around > thr).tolist() == [False, False, True]
    assert [bool(v > thr) for v in around] == [False, False, True]
    assert bool(np.mean(around[1:2]) > thr) is False and float(t32) > thr     # in float64 the middle value would pass


def test_grid_range_syntax():
    from citlab_article_separation_new_amd import run_cluster_grid_search as gs
    assert gs.parse_values("0.3,0.5, 0.7") == [0.3, 0.5, 0.7]
    assert gs.parse_values("0.2:0.6:0.2") == [0.2, 0.4, 0.6]
    assert gs.parse_values("0:1:0.05") == [round(0.05 * i, 10) for i in range(21)]
    assert gs.parse_values("0.5:0.5:0.1") == [0.5]
    assert gs.parse_values("1:3:1", int) == [1, 2, 3] and gs.parse_values("1,2", int) == [1, 2]
    for bad in ("0:1", "0:1:0", "1:0:0.1", "a,b"):
        with pytest.raises(Exception):
            gs.parse_values(bad)
    for bad in ("1.5", "1,2.5", "1:2:0.5"):
        with pytest.raises(Exception, match="not an integer"):
            gs.parse_values(bad, int)
    settings, infos = gs.grid_settings([0.5, 0.6], [0.4], [1])
    assert infos == ["dbscan_conf0.5_cluster0.4", "dbscan_conf0.6_cluster0.4"]
    assert settings[1] == {"min_neighbors_for_cluster": 1, "confidence_threshold": 0.6, "cluster_agreement_threshold": 0.4}
    _, infos = gs.grid_settings([0.5], [0.4], [1, 2])
    assert infos == ["dbscan_conf0.5_cluster0.4_nb1", "dbscan_conf0.5_cluster0.4_nb2"]


def test_command_line_parsers():
    from citlab_article_separation_new_amd import run_cluster_grid_search as gs, run_compare as rc, run_conf_to_cluster as c2c
    f = c2c.build_parser().parse_known_args(["--eval_list", "a.lst", "--clustering_method", "greedy", "--clustering_params",
                                             "max_iteration=7", "confidence_threshold=0.25", "--out_dir", "o", "--num_workers", "3"])[0]
    assert (f.eval_list, f.clustering_method, f.out_dir, f.num_workers) == ("a.lst", "greedy", "o", 3)
    assert f.clustering_params == {"max_iteration": 7, "confidence_threshold": 0.25}
    d = c2c.build_parser().parse_known_args([])[0]
    assert (d.eval_list, d.clustering_method, d.clustering_params, d.out_dir, d.num_workers) == ("", "dbscan", {}, "", 1)
    with pytest.raises(SystemExit):
        c2c.build_parser().parse_known_args(["--clustering_method", "kmeans"])
    a = rc.build_parser().parse_args(["--gt_list", "g.lst", "--work_dir", "w", "--out_dir", "o", "--name", "n", "--exclude", "x,y"])
    assert (a.gt_list, a.gt_dir, a.exclude, a.work_dir, a.out_dir, a.name) == ("g.lst", None, "x,y", "w", "o", "n")
    with pytest.raises(SystemExit):
        rc.build_parser().parse_args(["--gt_list", "g.lst"])
    g = gs.build_parser().parse_args(["--eval_list", "e", "--gt_list", "g", "--out_dir", "o", "--confidence_thresholds", "0.4:0.6:0.1",
                                      "--cluster_agreement_thresholds", "0.5", "--min_neighbors", "1,2", "--write_winner"])
    assert g.confidence_thresholds == [0.4, 0.5, 0.6] and g.cluster_agreement_thresholds == [0.5] and g.min_neighbors == [1, 2]
    assert g.write_winner is True
    g = gs.build_parser().parse_args(["--eval_list", "e", "--gt_list", "g", "--out_dir", "o"])
    assert len(g.confidence_thresholds) == 21 and len(g.cluster_agreement_thresholds) == 21 and g.min_neighbors == [1]


def test_cluster_grid_needs_a_gpu():
    """no CPU fallback: without a device (or without the built library) the constructor raises"""
    from citlab_article_separation_new_amd import _lib
    from citlab_article_separation_new_amd.clustering.cluster_grid import ClusterGrid
    try:
        have_gpu = os.path.exists(_lib.LIB_PATH) and _lib.load_library().asep_device_count() > 0
    except Exception:
        have_gpu = False
    if have_gpu:
        assert ClusterGrid(0).max_nodes >= 1024
    else:
        with pytest.raises(_lib.AsepError):
            ClusterGrid(0)


def test_setting_array_defaults():
    from citlab_article_separation_new_amd.clustering.cluster_grid import setting_array
    arr = setting_array([{}, {"min_neighbors_for_cluster": 3, "confidence_threshold": 0.3, "cluster_agreement_threshold": 0.7,
                              "assign_noise_clusters": False}])
    assert (arr[0].min_neighbors, arr[0].assign_noise, arr[0].conf_thr, arr[0].agree_thr) == (1, 1, 0.5, 0.5)
    assert (arr[1].min_neighbors, arr[1].assign_noise, arr[1].conf_thr, arr[1].agree_thr) == (3, 0, 0.3, 0.7)
