"""Host side of the clustering methods on the device (csrc/cluster_grid_kernels.h: cluster_std_kernel, cluster_greedy_kernel):
the restatement of sklearn's dbscan that the kernel is written to, pinned against sklearn.cluster.dbscan; the grid search's
new flags; and the ctypes view of asep_cluster_method_setting against the header."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import clustering_cases as cc  # noqa: E402


def dbscan_std_restated(dist, eps, min_samples):
    """sklearn.cluster.dbscan(dist, metric='precomputed', eps, min_samples) as cluster_std_kernel computes it.  It rests on this
    behaviour of sklearn: the neighbourhood of i is row i of the matrix, {j : dist[i, j] <= eps}, compared in the matrix dtype
    (NearestNeighbors.radius_neighbors on a precomputed matrix), the point itself included through the zero diagonal; i is a
    core point when it has >= min_samples neighbours; clusters are numbered from 0 by their seed, the lowest core point without
    a label, and hold what is reachable from the seed along neighbourhoods of core points; a non-core point keeps the first
    cluster that reaches it and is not expanded; the rest is -1.  The set reached does not depend on the walking order."""
    dist = np.asarray(dist)
    n = dist.shape[0]
    near = dist <= dist.dtype.type(eps)
    core = near.sum(axis=1) >= min_samples
    labels = np.full(n, -1, np.int64)
    label = 0
    for seed in range(n):
        if labels[seed] != -1 or not core[seed]:
            continue
        labels[seed] = label
        queue = [seed]
        for owner in queue:                                  # (grows while it is walked)
            for j in np.flatnonzero(near[owner] & (labels == -1)):
                labels[j] = label
                if core[j]:
                    queue.append(int(j))
        label += 1
    return labels


def _dist_mats(case, symmetry_fn):
    from citlab_article_separation_new_amd.clustering import TextblockClustering

    class _F:
        clustering_params = {}
    tb = TextblockClustering(_F())
    if symmetry_fn == "default":
        tb.set_confs(cc.make_confs(**case))
    else:
        tb.set_confs(cc.make_confs(**case), symmetry_fn=symmetry_fn)
    return tb._dist_mat


def _eps_values(dist):
    n = dist.shape[0]
    entry = np.float32(dist[1, n - 1])                       # an off-diagonal entry, and its float32 neighbours
    return [0.2, 0.5, 0.7, float(dist[1, n - 1]), float(np.nextafter(entry, np.float32(0))),
            float(np.nextafter(entry, np.float32(np.inf)))]


@pytest.mark.parametrize("symmetry_fn", ["default", None])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dbscan_std_restatement_equals_sklearn(dtype, symmetry_fn):
    from sklearn.cluster import dbscan as sk_dbscan
    cases = [c for c in cc.CASES if c["n"] in (3, 12, 50) and c["dtype"] == dtype]
    assert len(cases) == 12
    n_noise = n_asym = 0
    for case in cases:
        dist = _dist_mats(case, symmetry_fn)
        assert dist.dtype == np.dtype(dtype)
        n_asym += not np.array_equal(dist, dist.T)
        for eps in _eps_values(dist):
            for min_samples in range(1, 6):
                _, want = sk_dbscan(dist, metric="precomputed", eps=eps, min_samples=min_samples)
                got = dbscan_std_restated(dist, eps, min_samples)
                assert got.tolist() == want.tolist(), f"{case}, eps {eps!r}, min_samples {min_samples}"
                n_noise += int((want == -1).any())
    assert n_noise > 0 and (n_asym > 0) == (symmetry_fn is None)


def test_grid_settings_of_three_methods():
    from citlab_article_separation_new_amd import run_cluster_grid_search as gs
    from citlab_article_separation_new_amd.clustering import TextblockClustering
    settings, infos = gs.grid_settings([0.5, 0.6], [0.4], [1], ("greedy", "dbscan", "dbscan_std"), [0.3, 0.5], [1, 2], [1000, 5])
    assert settings == [
        {"min_neighbors_for_cluster": 1, "confidence_threshold": 0.5, "cluster_agreement_threshold": 0.4},
        {"min_neighbors_for_cluster": 1, "confidence_threshold": 0.6, "cluster_agreement_threshold": 0.4},
        {"clustering_method": "greedy", "max_iteration": 1000}, {"clustering_method": "greedy", "max_iteration": 5},
        {"clustering_method": "dbscan_std", "epsilon": 0.3, "min_samples": 1},
        {"clustering_method": "dbscan_std", "epsilon": 0.3, "min_samples": 2},
        {"clustering_method": "dbscan_std", "epsilon": 0.5, "min_samples": 1},
        {"clustering_method": "dbscan_std", "epsilon": 0.5, "min_samples": 2}]

    class _F:
        clustering_params = {}
    for params, info in zip(settings, infos):
        method = params.get("clustering_method", "dbscan")
        _F.clustering_params = {k: v for k, v in params.items() if k != "clustering_method"}
        assert info == TextblockClustering(_F()).get_info(method)
    assert infos[2:5] == ["greedy_iter1000", "greedy_iter5", "dbscan_std_eps0.3_samples1"]
    only_std, infos = gs.grid_settings([0.5], [0.5], [1], ("dbscan_std",))
    assert only_std == [{"clustering_method": "dbscan_std", "epsilon": 0.5, "min_samples": 1}] and infos == ["dbscan_std_eps0.5_samples1"]


def test_new_flags_and_the_default_command_line():
    from citlab_article_separation_new_amd import run_cluster_grid_search as gs
    base = ["--eval_list", "e", "--gt_list", "g", "--out_dir", "o"]
    d = gs.build_parser().parse_args(base)
    assert (d.methods, d.epsilons, d.min_samples, d.max_iterations) == (None, [0.5], [1], [1000])
    # the default command line: today's settings, and today's ranking header and rows
    settings, infos = gs.grid_settings(d.confidence_thresholds, d.cluster_agreement_thresholds, d.min_neighbors, d.methods or ("dbscan",),
                                       d.epsilons, d.min_samples, d.max_iterations)
    assert (settings, infos) == gs.grid_settings(d.confidence_thresholds, d.cluster_agreement_thresholds, d.min_neighbors)
    assert len(settings) == 441 and all(set(s) == {"min_neighbors_for_cluster", "confidence_threshold", "cluster_agreement_threshold"}
                                        for s in settings)
    assert gs.ranking_row(infos[22], settings[22], np.int64(7)) == ["dbscan_conf0.05_cluster0.05", 1, "0.05", "0.05", 7]
    a = gs.build_parser().parse_args(base + ["--methods", "dbscan, greedy,dbscan_std", "--epsilons", "0.2:0.6:0.2", "--min_samples", "1,3",
                                             "--max_iterations", "10,1000"])
    assert (a.methods, a.epsilons, a.min_samples, a.max_iterations) == (["dbscan", "greedy", "dbscan_std"], [0.2, 0.4, 0.6], [1, 3],
                                                                        [10, 1000])
    assert gs.METHOD_COLUMNS == ["clustering_method", "epsilon", "min_samples", "max_iteration"]
    assert gs.ranking_row("i", {"clustering_method": "dbscan_std", "epsilon": 0.2, "min_samples": 3}, 4, True) == \
        ["i", "", "", "", 4, "dbscan_std", "0.2", 3, ""]
    assert gs.ranking_row("i", settings[0], 4, True)[4:] == [4, "dbscan", "", "", ""]
    for bad in ("linkage", "dbscan,kmeans", "greedy,greedy", ""):
        with pytest.raises(SystemExit):
            gs.build_parser().parse_args(base + ["--methods", bad])
    with pytest.raises(SystemExit):
        gs.build_parser().parse_args(base + ["--min_samples", "1.5"])


def test_method_setting_struct_matches_the_header():
    import ctypes as C
    from citlab_article_separation_new_amd import _lib
    with open(os.path.join(ROOT, "include", "asep_hip.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct asep_cluster_method_setting \{(.*?)\} asep_cluster_method_setting;", src, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(name, ctype[t]) for t, name in fields] == list(_lib.ClusterMethodSetting._fields_)
    assert C.sizeof(_lib.ClusterMethodSetting) == 32 and _lib.ClusterMethodSetting.conf_thr.offset == 16
    for name, value in _lib.CLUSTER_METHODS.items():
        assert re.search(rf"#define ASEP_CLUSTER_{name.upper()} {value}\b", src)
    res, args = _lib.SIGNATURES["asep_cluster_grid_run_methods"]
    decl = re.search(r"int asep_cluster_grid_run_methods\((.*?)\);", src, re.S).group(1)
    assert res is C.c_int and len(args) == len(decl.split(",")) == 18


def test_method_setting_array():
    from citlab_article_separation_new_amd.clustering.cluster_grid import method_setting_array
    arr = method_setting_array([{}, {"clustering_method": "dbscan_std", "epsilon": 0.3, "min_samples": 4, "confidence_threshold": 0.7},
                                {"clustering_method": "greedy"}, {"clustering_method": "greedy", "max_iteration": 0},
                                {"clustering_method": "dbscan", "min_neighbors_for_cluster": 2, "assign_noise_clusters": False,
                                 "cluster_agreement_threshold": 0.25}])
    got = [(a.method, a.count, a.assign_noise, a.reserved, a.conf_thr, a.param) for a in arr]
    assert got == [(0, 1, 1, 0, 0.5, 0.5), (1, 4, 1, 0, 0.7, 0.3), (2, 1000, 1, 0, 0.5, 0.0), (2, 0, 1, 0, 0.5, 0.0),
                   (0, 2, 0, 0, 0.5, 0.25)]
    with pytest.raises(ValueError, match="TextblockClustering"):
        method_setting_array([{"clustering_method": "linkage"}])
    with pytest.raises(ValueError, match="kmeans"):
        method_setting_array([{"clustering_method": "kmeans"}])
