"""The ``dbscan``, ``dbscan_std`` and ``greedy`` clusterings of many pages under many settings in one call
(``asep_cluster_grid_run`` for ``dbscan`` alone, ``asep_cluster_grid_run_methods`` for the three mixed), and behind them the
split / merge counts of ``as_eval`` and ``rel_LLH`` for every (page, setting).

``ClusterGrid`` prepares each page's matrix with the host classes' own code (``TextblockClustering.set_confs`` and
``DBScanRelation.initialize_clustering``), so the device sees what ``DBScanRelation.confidences`` holds; the labels it returns
equal ``TextblockClustering.calc('dbscan')``'s, integer for integer (a page of two nodes follows ``calc``'s special rule: it is
uploaded as ``_conf_mat``, not made symmetric, and the kernel tests ``conf[0, 1] >= confidence_threshold``).  A setting dict
may carry ``"clustering_method"`` (``"dbscan"`` when absent; ``"method"`` is linkage's parameter): ``"dbscan_std"`` reads
``epsilon`` / ``min_samples`` and runs on the page's ``_dist_mat``, ``"greedy"`` reads ``max_iteration`` and runs on
``_delta_mat``; their labels equal ``calc('dbscan_std')``'s and ``calc('greedy')``'s.  ``"linkage"`` stays with the host class.
There is no CPU fallback: without a GPU the constructor raises.
"""
import ctypes as C

import numpy as np
from scipy.stats import gmean

from .. import _lib
from .dbscan import DBScanRelation
from .textblock_clustering import DEFAULT_PARAMS, TextblockClustering


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    np.cumsum(counts, out=off[1:])
    return off


def _per_page(row, node_off):
    return [row[node_off[k]:node_off[k + 1]] for k in range(len(node_off) - 1)]


class _Flags:
    clustering_params = {}


def setting_array(settings):
    """clustering_params dicts (missing keys: TextblockClustering's defaults) -> ctypes array of asep_cluster_setting"""
    arr = (_lib.ClusterSetting * max(1, len(settings)))()
    for i, given in enumerate(settings):
        p = dict(DEFAULT_PARAMS)
        p.update(given)
        arr[i] = _lib.ClusterSetting(int(p["min_neighbors_for_cluster"]), 1 if p["assign_noise_clusters"] else 0,
                                     float(p["confidence_threshold"]), float(p["cluster_agreement_threshold"]))
    return arr


def _method_of(given):
    method = given.get("clustering_method", "dbscan")
    if method == "linkage":
        raise ValueError("clustering_method 'linkage' does not run on the device: use TextblockClustering.calc('linkage')")
    if method not in _lib.CLUSTER_METHODS:
        raise ValueError(f"clustering_method '{method}': the clustering grid runs {', '.join(_lib.CLUSTER_METHODS)}")
    return method


def method_setting_array(settings):
    """clustering_params dicts with an optional "clustering_method" -> ctypes array of asep_cluster_method_setting"""
    arr = (_lib.ClusterMethodSetting * max(1, len(settings)))()
    for i, given in enumerate(settings):
        method = _method_of(given)
        p = dict(DEFAULT_PARAMS)
        p.update(given)
        count, param = {"dbscan": ("min_neighbors_for_cluster", "cluster_agreement_threshold"),
                        "dbscan_std": ("min_samples", "epsilon"), "greedy": ("max_iteration", None)}[method]
        arr[i] = _lib.ClusterMethodSetting(_lib.CLUSTER_METHODS[method], int(p[count]), 1 if p["assign_noise_clusters"] else 0, 0,
                                           float(p["confidence_threshold"]), float(p[param]) if param else 0.0)
    return arr


class ClusterGrid:
    def __init__(self, device=0):
        from ..textblock import _handle
        self._lib, self._h = _handle(device)            # raises without the library or a GPU
        self.max_nodes = self._lib.asep_cluster_grid_max_nodes()
        self.mats = []
        self.dists = []                                 # _dist_mat and _delta_mat of the pages, next to mats
        self.deltas = []
        self.dtype = None
        self.kernel_us = 0.0

    def add_page(self, confs, symmetry_fn=gmean):
        """One page's raw confidences [N, N] (as the net or a confidence json gives them) -> its index in this grid."""
        tb = TextblockClustering(_Flags())
        tb.set_confs(confs, symmetry_fn=symmetry_fn)
        n = tb._mat_dim
        scanner = DBScanRelation()
        scanner.initialize_clustering(n, tb._conf_mat)
        # calc() does not cluster a page of two nodes: it tests _conf_mat[0, 1], which initialize_clustering has not made
        # symmetric; the kernel applies that rule to the matrix it is given, so such a page travels as _conf_mat
        mat = np.ascontiguousarray(tb._conf_mat if n == 2 else scanner.confidences)
        if mat.dtype not in (np.float32, np.float64):
            raise ValueError(f"confidences of dtype {mat.dtype}: the clustering grid takes float32 or float64 matrices")
        if self.dtype is not None and mat.dtype != self.dtype:
            raise ValueError(f"page {len(self.mats)} has a {mat.dtype} matrix, the pages before it {self.dtype}: the pages of one "
                             f"run share one dtype (the thresholds are compared in it)")
        if n > self.max_nodes:
            raise ValueError(f"page {len(self.mats)} has {n} nodes, the device engine clusters at most {self.max_nodes}")
        self.dtype = mat.dtype
        self.mats.append(mat)
        self.dists.append(np.ascontiguousarray(tb._dist_mat, mat.dtype))
        self.deltas.append(np.ascontiguousarray(tb._delta_mat, mat.dtype))
        return len(self.mats) - 1

    def clear(self):
        self.mats = []
        self.dists = []
        self.deltas = []
        self.dtype = None

    # -- launches --------------------------------------------------------------------------------------------------
    def _run(self, settings, tables=None, llh=False):
        node_off = _offsets([m.shape[0] for m in self.mats])
        flat = lambda mats: np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0, np.float32)   # noqa: E731
        conf = flat(self.mats)
        methods = [_method_of(given) for given in settings]
        labels = np.zeros((len(settings), int(node_off[-1])), np.int32)
        counts = None
        args = [None] * 6
        if tables is not None:
            line_off = _offsets([len(t["line_node"]) for t in tables])
            blocks = [b for t in tables for b in t["blocks"]]
            args = [line_off, np.concatenate([t["line_node"] for t in tables] + [np.zeros(0, np.int32)]).astype(np.int32),
                    np.concatenate([t["line_gt"] for t in tables] + [np.zeros(0, np.int32)]).astype(np.int32),
                    _offsets([len(t["blocks"]) for t in tables]), _offsets([len(b) for b in blocks]),
                    np.asarray([i for b in blocks for i in b], np.int32)]
            counts = np.zeros((len(settings), len(self.mats), 4), np.int32)
        is_f64 = 1 if conf.dtype == np.float64 else 0
        rel_llh = None
        if not llh and all(m == "dbscan" for m in methods):
            _lib.check(self._lib.asep_cluster_grid_run(self._h, len(self.mats), _ptr(node_off), _ptr(conf), is_f64, len(settings),
                                                       setting_array(settings), *[_ptr(a) for a in args], _ptr(labels),
                                                       _ptr(counts)),
                       "asep_cluster_grid_run")
        else:
            if "greedy" in methods:
                for k, d in enumerate(self.deltas):
                    if np.isnan(d).any() or (d == np.inf).any():
                        raise ValueError(f"page {k}: its _delta_mat holds NaN or +inf, greedy needs finite entries off the diagonal "
                                         f"(confidences in [0, 1])")
            dist = flat(self.dists) if "dbscan_std" in methods else None
            delta = flat(self.deltas) if llh or "greedy" in methods else None
            if llh:
                rel_llh = np.zeros((len(settings), len(self.mats)), np.float64)
            _lib.check(self._lib.asep_cluster_grid_run_methods(self._h, len(self.mats), _ptr(node_off), is_f64, _ptr(conf),
                                                               _ptr(dist), _ptr(delta), len(settings),
                                                               method_setting_array(settings), *[_ptr(a) for a in args],
                                                               _ptr(labels), _ptr(counts), _ptr(rel_llh)),
                       "asep_cluster_grid_run_methods")
        self.kernel_us = self._lib.asep_cluster_grid_last_kernel_us()
        return node_off, labels, counts, rel_llh

    def run_array(self, settings):
        """-> (node_off int32 [pages + 1], labels int32 [settings, nodes of all pages])"""
        node_off, labels, _, _ = self._run(list(settings))
        return node_off, labels

    def run(self, settings):
        """-> labels[setting][page]: int32 array of the page's labels, as the setting's method numbers them: dbscan from 1 (-1:
        noise left unassigned), dbscan_std from 0 (-1: noise), greedy from 0"""
        node_off, labels = self.run_array(settings)
        return [_per_page(row, node_off) for row in labels]

    def run_llh(self, settings):
        """-> (labels[setting][page], rel_LLH float64 [settings, pages]): ``TextblockClustering.rel_LLH`` of the labels, each
        term formed in the matrix dtype and the sum taken in float64 (the host class adds in the matrix dtype)"""
        node_off, labels, _, rel_llh = self._run(list(settings), llh=True)
        return [_per_page(row, node_off) for row in labels], rel_llh

    def run_compare_array(self, settings, tables):
        """``tables``: one ``as_eval.comparison_tables`` dict per page.  -> (node_off, labels, counts int32 [settings, pages, 4]
        = hypNIs, n_inf, corrects, 0)"""
        if len(tables) != len(self.mats):
            raise ValueError(f"{len(tables)} comparison tables for {len(self.mats)} pages")
        return self._run(list(settings), list(tables))[:3]

    def run_compare(self, settings, pages, on_inconsistent="raise"):
        """``pages``: per page (hypothesis PAGE-XML whose text regions are the page's nodes, ground truth PAGE-XML), paths or
        ``Page`` objects.  -> (comparisons[setting][page]: ``as_eval.SepPageComparison``, labels[setting][page]).  A page whose
        ground truth lines are a strict subset of the hypothesis lines raises AssertionError as ``SepPageBlComper`` does, or
        yields None entries with ``on_inconsistent='none'``."""
        from ..as_eval import SepPageComparison, comparison_tables
        tables = [comparison_tables(hyp, gt) for hyp, gt in pages]
        for k, t in enumerate(tables):
            if len(t["line_node"]) and int(t["line_node"].max()) >= self.mats[k].shape[0]:
                raise ValueError(f"page {k}: its PAGE-XML has more text regions with lines than the matrix has nodes")
            if t["inconsistent"] and on_inconsistent == "raise":
                raise AssertionError(f"cannot compare page {k}: inconsistent baselines")
        node_off, labels, counts = self.run_compare_array(settings, tables)
        comps = [[None if t["inconsistent"] else SepPageComparison.from_counts(t["gtNIs"], c[0], c[1], c[2])
                  for t, c in zip(tables, row.tolist())] for row in counts]
        return comps, [_per_page(row, node_off) for row in labels]
