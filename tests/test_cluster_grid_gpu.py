"""The clustering grid on the device (clustering/cluster_grid.py, csrc/cluster_grid_kernels.h): labels equal to the host class
TextblockClustering(...).calc('dbscan') integer for integer, the split / merge counts equal to as_eval.SepPageBlComper on
PAGE-XMLs written from the device labels, the three command lines, and bad arguments.  Equality is exact everywhere."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import as_eval_cases  # noqa: E402
import clustering_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

GRID_SIZES = (7, 12, 20, 33, 50, 70)
GRID = [{"confidence_threshold": c, "cluster_agreement_threshold": a} for c in (0.3, 0.45, 0.5, 0.6, 0.75)
        for a in (0.3, 0.4, 0.5, 0.6, 0.7)]


class _Flags:
    def __init__(self, params):
        self.clustering_params = dict(params)


def host_labels(confs, params, symmetry_fn="default"):
    from citlab_article_separation_new_amd.clustering import TextblockClustering
    tb = TextblockClustering(_Flags(params))
    if symmetry_fn == "default":
        tb.set_confs(confs)
    else:
        tb.set_confs(confs, symmetry_fn=symmetry_fn)
    tb.calc("dbscan")
    return [int(v) for v in tb.tb_labels]


def device_labels(mats, settings, **kw):
    from citlab_article_separation_new_amd.clustering.cluster_grid import ClusterGrid
    grid = ClusterGrid(0)
    for m in mats:
        grid.add_page(m, **kw)
    return [[lab.tolist() for lab in row] for row in grid.run(settings)]


def check(mats, settings, **kw):
    got = device_labels(mats, settings, **kw)
    host_kw = {"symmetry_fn": kw["symmetry_fn"]} if "symmetry_fn" in kw else {}
    for s, params in enumerate(settings):
        for k, m in enumerate(mats):
            want = host_labels(m, params, **host_kw)
            assert got[s][k] == want, f"setting {s} {params}, page {k} (n={len(m)}): {got[s][k]} != {want}"


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_golden_cases_all_variants(dtype):
    cases = [c for c in cc.CASES if c["n"] in (3, 12, 50) and c["dtype"] == dtype]
    assert len(cases) == 12
    check([cc.make_confs(**c) for c in cases], list(cc.DBSCAN_VARIANTS))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_blocks_200(dtype):
    case = next(c for c in cc.CASES if c["n"] == 200 and c["kind"] == "blocks" and c["dtype"] == dtype)
    check([cc.make_confs(**case)], list(cc.DBSCAN_VARIANTS))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ties_cross_the_unroll(dtype):
    mats = [cc.make_confs("ties", n, 40 + n, dtype) for n in (9, 17)]
    settings = [{"confidence_threshold": c, "cluster_agreement_threshold": a, "min_neighbors_for_cluster": nb}
                for c in (0.25, 0.5) for a in (0.25, 0.5, 0.75) for nb in (1, 2)]
    check(mats, settings)
    check(mats, settings, symmetry_fn=None)          # the avg path: means of 0.25 / 0.5 / 0.75 land exactly on the thresholds


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_single_article_of_300(dtype):
    rng = np.random.default_rng(300)
    a = rng.uniform(0.55, 0.999, (300, 300))
    m = ((a + a.T) / 2).astype(dtype)
    settings = [{"confidence_threshold": 0.5, "cluster_agreement_threshold": 0.5},
                {"confidence_threshold": 0.5, "cluster_agreement_threshold": 0.775},      # the mean of the planted confidences
                {"confidence_threshold": 0.8, "cluster_agreement_threshold": 0.77, "min_neighbors_for_cluster": 2}]
    got = device_labels([m], settings, symmetry_fn=None)
    assert got[0][0] == [1] * 300
    check([m], settings, symmetry_fn=None)


def test_thresholds_next_to_the_values():
    """float32 values one step below, at and above the thresholds: the comparison is float32's, as numpy's is"""
    t = np.float32(0.6)
    near = np.array([np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))], np.float32)
    rng = np.random.default_rng(5)
    m = near[rng.integers(0, 3, (24, 24))]
    m = np.minimum(m, m.T)
    settings = [{"confidence_threshold": c, "cluster_agreement_threshold": a} for c in (0.6, float(near[0]), 0.5) for a in (0.6, float(near[0]))]
    check([m, m.astype(np.float64)[:11, :11].astype(np.float32)], settings, symmetry_fn=None)
    check([m.astype(np.float64)], settings, symmetry_fn=None)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_no_neighbours_and_tiny_pages(dtype):
    low = np.full((10, 10), 0.1, dtype)
    tiny = [np.zeros((0, 0), dtype), np.full((1, 1), 0.9, dtype), np.array([[0.9, 0.7], [0.7, 0.9]], dtype),
            np.array([[0.9, 0.2], [0.2, 0.9]], dtype), np.array([[0.5, 0.5], [0.5, 0.5]], dtype),
            np.array([[0.9, 0.7], [0.2, 0.9]], dtype), np.array([[0.9, 0.2], [0.7, 0.9]], dtype)]   # calc() tests [0, 1] as given
    settings = [{"assign_noise_clusters": True}, {"assign_noise_clusters": False}, {"min_neighbors_for_cluster": 0},
                {"confidence_threshold": 0.7, "assign_noise_clusters": False}]
    got = device_labels([low] + tiny, settings, symmetry_fn=None)
    assert got[0][0] == list(range(1, 11)) and got[1][0] == [-1] * 10
    assert got[0][1] == [] and got[0][2] == [1] and got[1][2] == [-1]
    assert got[0][6] == [1, 1] and got[0][7] == [1, 2]        # not the average 0.45 of the two directions
    check([low] + tiny, settings, symmetry_fn=None)
    check([low] + tiny[1:], settings)


def test_mixed_dtypes_are_refused():
    from citlab_article_separation_new_amd.clustering.cluster_grid import ClusterGrid
    grid = ClusterGrid(0)
    grid.add_page(np.full((3, 3), 0.5, np.float32))
    with pytest.raises(ValueError, match="share one dtype"):
        grid.add_page(np.full((3, 3), 0.5, np.float64))


# ---- six pages, a 5 x 5 grid: indexing, counts, command lines -----------------------------------------------------------------
def _planted(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, max(1, n // 6), size=n)


@pytest.fixture(scope="module")
def grid_pages(tmp_path_factory):
    """six `blocks` pages: confidences (asymmetric float32), PAGE-XMLs (one region per node, 1-3 lines each), ground truth
    PAGE-XMLs from the planted labels with 10 % of the regions reassigned, and the confidence jsons.  Behind them a page of
    two regions with asymmetric confidences (its json keeps them asymmetric) and a page of one region (two lines) whose
    ground truth has three articles (article indices above the number of hypothesis lines).  Page 3's ground truth lines are
    a strict subset of its hypothesis lines (`gt`); `gt_full` is the same ground truth with every line."""
    from scipy.stats import gmean
    from citlab_article_separation_new_amd import gnn_results
    from citlab_article_separation_new_amd.page_xml import Page
    root = tmp_path_factory.mktemp("grid")
    os.makedirs(root / "set" / "page")
    os.makedirs(root / "gt" / "page")
    os.makedirs(root / "gt_full" / "page")
    rng = np.random.default_rng(99)
    pages = []
    for k, n in enumerate(GRID_SIZES + (2, 1)):
        seed = 700 + n
        confs = cc.make_confs("blocks", n, seed, "float32")
        if n == 2:
            confs = np.array([[0.9, 0.7], [0.2, 0.9]], np.float32)
        assert n == 1 or not np.array_equal(confs, confs.T)
        lab = _planted(n, seed).copy()
        moved = rng.choice(n, max(1, n // 10), replace=False)
        lab[moved] = rng.integers(0, max(1, n // 6) + 1, size=len(moved))
        lines = [[f"r{r}l{j}" for j in range(1 + (r + k) % 3)] for r in range(n)]
        hyp_regions = [[(l, None) for l in reg] for reg in lines]
        gt_regions = [[(l, f"g{lab[r]}") for l in reg] for r, reg in enumerate(lines)]
        if k in (1, 5):                      # two ground truth lines the hypothesis lacks
            gt_regions[0] += [(f"p{k}_extra0", f"g{lab[0]}")]
            gt_regions[n - 1] += [(f"p{k}_extra1", "g_own")]
        if n == 1:                           # three ground truth articles, the hypothesis has the lines of the last one only
            gt_regions = [[("other0", "g7")], [("other1", "g8")], gt_regions[0]]
        name = f"page{k}"
        gt_full = as_eval_cases.write_page(root / "gt_full" / "page" / f"{name}.xml", gt_regions, Page)
        if k in (3, 5):                      # one hypothesis line the ground truth lacks (k == 3: a strict subset)
            gt_regions[2] = gt_regions[2][1:]
        page_path = as_eval_cases.write_page(root / "set" / "page" / f"{name}.xml", hyp_regions, Page)
        gt_path = as_eval_cases.write_page(root / "gt" / "page" / f"{name}.xml", gt_regions, Page)
        json_path = gnn_results.save_conf_to_json(confs, page_path, "", symmetry_fn=None if n == 2 else gmean)
        pages.append({"name": name, "confs": confs, "page": page_path, "gt": gt_path, "gt_full": gt_full, "json": json_path})
    with open(root / "confs.lst", "w") as f:
        f.write("\n".join(p["json"] for p in pages) + "\n")
    with open(root / "gt.lst", "w") as f:
        f.write("\n".join(p["gt"] for p in pages) + "\n")
    return root, pages


def test_grid_over_the_pages(grid_pages):
    _, pages = grid_pages
    check([p["confs"] for p in pages], GRID, symmetry_fn=None)


def test_counts_equal_host_comparison(grid_pages, tmp_path, monkeypatch):
    from citlab_article_separation_new_amd import as_eval, gnn_results
    from citlab_article_separation_new_amd.clustering.cluster_grid import ClusterGrid
    root, pages = grid_pages
    monkeypatch.chdir(root)
    grid = ClusterGrid(0)
    for p in pages:
        grid.add_page(p["confs"], symmetry_fn=None)
    pairs = [(p["page"], p["gt"]) for p in pages]
    with pytest.raises(AssertionError, match="inconsistent baselines"):
        grid.run_compare(GRID, pairs)
    comps, labels = grid.run_compare(GRID, pairs, on_inconsistent="none")
    n_raised = 0
    for k, p in enumerate(pages):
        comper = as_eval.SepPageBlComper()
        comper.loadGT(p["gt"])
        for s in range(len(GRID)):
            hyp = gnn_results.save_clustering_to_page(labels[s][k].tolist(), p["page"], str(tmp_path), info=f"s{s}")
            try:
                want = comper.compareTo(hyp)
            except AssertionError:
                want = None
                n_raised += 1
            got = comps[s][k]
            assert got == want, f"page {k}, setting {s}: {got} != {want}"
    assert n_raised == len(GRID)                               # page 3 only
    assert as_eval.comparison_tables(pages[7]["page"], pages[7]["gt"])["gtNIs"] == 3 and comps[0][7].gtNIs == 3


def _stable(path):
    with open(path, "rb") as f:
        return re.sub(rb"<LastChange>[^<]*</LastChange>", b"<LastChange/>", f.read())     # (the time of writing)


def test_run_conf_to_cluster(grid_pages, tmp_path, monkeypatch):
    from citlab_article_separation_new_amd import gnn_results, run_conf_to_cluster as c2c
    from citlab_article_separation_new_amd.clustering import TextblockClustering
    root, pages = grid_pages
    monkeypatch.chdir(root)
    params = {"confidence_threshold": 0.6, "cluster_agreement_threshold": 0.4}
    args = ["--eval_list", str(root / "confs.lst"), "--clustering_params", "confidence_threshold=0.6", "cluster_agreement_threshold=0.4"]
    written = c2c.main(args + ["--out_dir", str(tmp_path / "one")])
    written2 = c2c.main(args + ["--out_dir", str(tmp_path / "two"), "--num_workers", "2"])
    greedy = c2c.main(["--eval_list", str(root / "confs.lst"), "--clustering_method", "greedy", "--out_dir", str(tmp_path / "one")])
    assert len(written) == len(written2) == len(greedy) == len(pages)
    for p, got, got2, got_greedy in zip(pages, written, written2, greedy):
        _, confs = c2c.load_confidences(p["json"])
        for method, path in (("dbscan", got), ("greedy", got_greedy)):
            tb = TextblockClustering(_Flags(params))
            tb.set_confs(confs, symmetry_fn=None)
            tb.calc(method)
            want = gnn_results.save_clustering_to_page(tb.tb_labels, p["page"], str(tmp_path / "host"), info=tb.get_info(method))
            assert os.path.relpath(path, tmp_path / "one") == os.path.relpath(want, tmp_path / "host")
            assert _stable(path) == _stable(want), f"{path} differs from the host class's file"
        assert os.path.relpath(got2, tmp_path / "two") == os.path.relpath(got, tmp_path / "one") and _stable(got2) == _stable(got)
    two = c2c.load_confidences(pages[6]["json"])[1]
    assert two[0, 1] >= 0.6 > (two[0, 1] + two[1, 0]) / 2         # calc()'s rule and the symmetrised matrix disagree on this page
    assert _stable(written[6]).count(b"id:a1;") == 3 and b"id:a2;" not in _stable(written[6])


def test_grid_search_names_run_compare_winner(grid_pages, tmp_path, monkeypatch):
    import csv
    from citlab_article_separation_new_amd import run_cluster_grid_search as gs, run_compare as rc, run_conf_to_cluster as c2c
    root, pages = grid_pages
    monkeypatch.chdir(root)
    # every page; page 3 with the ground truth that has all its lines (run_compare raises on the strict subset, checked below)
    keep = [dict(p, gt=p["gt_full"]) if k == 3 else p for k, p in enumerate(pages)]
    with open(tmp_path / "confs.lst", "w") as f:
        f.write("\n".join(p["json"] for p in keep) + "\n")
    with open(tmp_path / "gt.lst", "w") as f:
        f.write("\n".join(p["gt"] for p in keep) + "\n")
    with pytest.raises(AssertionError, match="inconsistent baselines"):
        gs.main(["--eval_list", str(root / "confs.lst"), "--gt_list", str(root / "gt.lst"), "--out_dir", str(tmp_path / "bad"),
                 "--confidence_thresholds", "0.5", "--cluster_agreement_thresholds", "0.5"])
    out = str(tmp_path / "out")
    conf_thrs, agree_thrs = [0.3, 0.4, 0.45], [0.3, 0.4, 0.7]
    for c in conf_thrs:
        for a in agree_thrs:
            c2c.main(["--eval_list", str(tmp_path / "confs.lst"), "--out_dir", out, "--clustering_params",
                      f"confidence_threshold={c}", f"cluster_agreement_threshold={a}"])
    results = rc.compare([p["gt"] for p in keep], rc.find_dirs("clustering", root=out))
    csv_ref, _, _, evaler = rc.write_outputs(results, str(tmp_path / "eval"), "ref")
    assert gs.main(["--eval_list", str(tmp_path / "confs.lst"), "--gt_list", str(tmp_path / "gt.lst"), "--out_dir", out,
                    "--confidence_thresholds", "0.3,0.4,0.45", "--cluster_agreement_thresholds", "0.3,0.4,0.7", "--write_winner"]) == 0
    with open(csv_ref) as f:
        want_rows = sorted(tuple(r.items()) for r in csv.DictReader(f))
    with open(os.path.join(out, "grid_comparison.csv")) as f:
        got_rows = sorted(tuple(r.items()) for r in csv.DictReader(f))
    assert got_rows == want_rows and len(got_rows) == 9 * len(keep)
    stat = evaler.winnerStatDict[rc.DATA_SET]
    with open(os.path.join(out, "grid_ranking.csv")) as f:
        ranking = list(csv.DictReader(f))
    method = {r["info"]: next(m for m in stat if m.endswith("/" + r["info"])) for r in ranking}
    assert {r["info"]: int(r["all"]) for r in ranking} == {r["info"]: stat[method[r["info"]]]["all"] for r in ranking}
    best = max(v["all"] for v in stat.values())
    assert int(ranking[0]["all"]) == best
    table = evaler.winnerDict[rc.DATA_SET]
    first = max((m for m in table if not m.startswith("_")), key=lambda m: len(table[m]))      # run_compare's winner
    # the thresholds are chosen so that one setting is ahead of all others: no tie rule decides the winner
    assert sum(v["all"] == best for v in stat.values()) == 1, sorted(v["all"] for v in stat.values())
    assert method[ranking[0]["info"]] == first
    for p in keep:                                              # --write_winner: the winner's files are run_conf_to_cluster's
        name = os.path.basename(p["page"])[:-4] + "_clustering.xml"
        assert os.path.isfile(os.path.join(out, "set", "clustering", ranking[0]["info"], name))


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------
def _call(lib, h, node_off, conf=None, settings=None, tables=None, n_settings=1):
    from citlab_article_separation_new_amd import _lib
    from citlab_article_separation_new_amd.clustering.cluster_grid import setting_array
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    node_off = np.asarray(node_off, np.int32)
    tables = [None if t is None else np.asarray(t, np.int32) for t in (tables or [None] * 6)]
    labels = np.zeros(max(1, int(max(node_off[-1], 0))) * n_settings, np.int32)
    counts = np.zeros(4 * n_settings * (len(node_off) - 1), np.int32)
    rc = lib.asep_cluster_grid_run(h, len(node_off) - 1, p(node_off), p(conf), 0, n_settings, setting_array(settings or [{}]),
                                   *[p(t) for t in tables], p(labels), p(counts) if tables[0] is not None else None)
    return rc, _lib.last_error()


def test_bad_arguments_return_an_error():
    from citlab_article_separation_new_amd.clustering.cluster_grid import ClusterGrid
    grid = ClusterGrid(0)
    lib, h = grid._lib, grid._h
    conf = np.full(9 + 16, 0.7, np.float32)
    rc, why = _call(lib, h, [0, 3, 2], conf)
    assert rc == -1 and "decreasing" in why
    rc, why = _call(lib, h, [1, 4], conf)
    assert rc == -1 and "start at 0" in why
    rc, why = _call(lib, h, [0, grid.max_nodes + 1])
    assert rc == -1 and f"at most {grid.max_nodes}" in why
    good = [[0, 2, 4], [0, 2, 0, 3], [0, 0, 1, -1], [0, 1, 1], [0, 2], [0, 1]]
    rc, why = _call(lib, h, [0, 3, 7], conf, tables=good)
    assert rc == 0, why
    bad_node = [t if i != 1 else [0, 3, 0, 3] for i, t in enumerate(good)]
    rc, why = _call(lib, h, [0, 3, 7], conf, tables=bad_node)
    assert rc == -1 and "hangs in node 3, the page has 3 nodes" in why
    bad_line = [t if i != 5 else [0, 2] for i, t in enumerate(good)]
    rc, why = _call(lib, h, [0, 3, 7], conf, tables=bad_line)
    assert rc == -1 and "lists line 2, the page has 2 lines" in why
    rc, why = _call(lib, h, [0, 3, 7], None)
    assert rc == -1 and "null argument" in why
    assert grid.run([{}]) == [[]]                              # the handle still works: no pages, nothing launched
