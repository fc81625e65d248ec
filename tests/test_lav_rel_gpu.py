"""Relation net evaluation on the GPU (asep_releval_*, lav_rel.RelationEval / LavGNN) against the installed sklearn.

Raw arrays: thresholds / tps / fps equal, as bit patterns and integers, to sklearn's _binary_clf_curve as its public
precision_recall_curve and roc_curve(drop_intermediate=False) show it; accuracy equal to accuracy_score;
|AUC - roc_auc_score| <= (K + 2) 2^-53, K = the points of sklearn's ROC curve (sklearn adds K float64 trapezoids that sum to
at most 1, each addition off by at most half an ulp of 1; the device value is one correctly rounded division of exact
integers).  End to end: LavGNN.evaluate()'s log against sklearn on the probabilities the host-returning forward gives.
"""
import json
import logging
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TILE = 4096            # keys per block of the sort and curve kernels (RELEV_TILE)


def _scores(rng, n, kind):
    y = (rng.random(n) < 0.3).astype(np.int32)
    if n >= 2:
        y[0], y[1] = 0, 1                                            # both classes
    p = (1.0 / (1.0 + np.exp(-(rng.normal(0, 1, n) + 1.5 * (2 * y - 1))))).astype(np.float32)
    if kind == "quantised":
        p = (np.round(p * 4) / 4).astype(np.float32)
    elif kind == "all_equal":
        p[:] = 0.5
    elif kind == "zeros_ones":
        k = rng.random(n)
        p[k < 0.25] = 0.0
        p[k > 0.75] = 1.0
    elif kind == "denormals":
        tiny = np.array([1e-45, 3e-45, 1e-40, 1e-39, 1.1754942e-38, 1.17549435e-38, 0.0], np.float32)
        k = rng.random(n) < 0.5
        p[k] = tiny[rng.integers(0, len(tiny), size=int(k.sum()))]
    return p, y


def _check_against_sklearn(curve, p, y, label):
    import sklearn.metrics as sk
    n_pos, n = int(y.sum()), len(y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prec, rec, thr = sk.precision_recall_curve(y, p)
        mine = curve.precision_recall_curve()
    assert len(curve.thresholds) == len(thr), label
    assert np.array_equal(curve.thresholds[::-1].view(np.uint32), thr.view(np.uint32)), label
    if 0 < n_pos < n:
        fpr, tpr, rthr = sk.roc_curve(y, p, drop_intermediate=False)
        tps, fps = np.rint(tpr[1:] * n_pos).astype(np.int64), np.rint(fpr[1:] * (n - n_pos)).astype(np.int64)
        assert np.array_equal(rthr[1:].view(np.uint32), curve.thresholds.view(np.uint32)), label
        assert np.array_equal(curve.tps, tps) and np.array_equal(curve.fps, fps), label
        assert np.array_equal(tpr[1:], curve.tps / n_pos) and np.array_equal(fpr[1:], curve.fps / (n - n_pos)), label
    for a, b in zip(mine, (prec, rec, thr)):                          # the same float64 divisions of the same integers
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), label
    assert curve.n == n and curve.n_pos == n_pos
    acc = sk.accuracy_score(y, p > 0.5)
    print(f"{label}: n {n}, thresholds {len(thr)}, accuracy {curve.accuracy!r} (sklearn {acc!r})", end="")
    assert curve.accuracy == acc, label
    if 0 < n_pos < n:
        auc = sk.roc_auc_score(y, p)
        K = len(sk.roc_curve(y, p)[0])
        print(f", auc {curve.auc_roc!r} (sklearn {auc!r}, diff {abs(curve.auc_roc - auc):.3g}, bound {(K + 2) * 2.0 ** -53:.3g})")
        assert abs(curve.auc_roc - auc) <= (K + 2) * 2.0 ** -53, label
    else:
        print()


@pytest.fixture(scope="module")
def acc():
    from citlab_article_separation_new_amd.lav_rel import RelationEval
    a = RelationEval(0)
    yield a
    a.close()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 17, 100003])
def test_sizes_against_sklearn(acc, n):
    rng = np.random.default_rng(n)
    p, y = _scores(rng, n, "plain")
    acc.reset()
    acc.append(p, y)
    _check_against_sklearn(acc.finish(), p, y, f"n={n}")


@pytest.mark.parametrize("kind", ["quantised", "all_equal", "zeros_ones", "denormals"])
@pytest.mark.parametrize("n", [TILE + 5, 300007])
def test_ties_and_special_values(acc, kind, n):
    rng = np.random.default_rng(len(kind) * 1000 + n)
    p, y = _scores(rng, n, kind)
    acc.reset()
    acc.append(p, y)
    _check_against_sklearn(acc.finish(), p, y, f"{kind} n={n}")


def test_one_class_lists(acc):
    rng = np.random.default_rng(3)
    p, _ = _scores(rng, 5000, "plain")
    for y in (np.zeros(5000, np.int32), np.ones(5000, np.int32)):
        acc.reset()
        acc.append(p, y)
        curve = acc.finish()
        _check_against_sklearn(curve, p, y, f"labels all {y[0]}")
        with pytest.warns(UserWarning, match="Only one class"):
            assert np.isnan(curve.auc_roc)


def test_pieces_reset_and_reuse(acc):
    """appends in uneven pieces give what one piece gives, bit for bit; a reset accumulator is as good as a new one"""
    rng = np.random.default_rng(77)
    n = 3 * TILE + 1234
    p, y = _scores(rng, n, "zeros_ones")
    acc.reset()
    acc.append(p, y)
    one = acc.finish()
    again = acc.finish()                                             # nothing appended since: the same results
    assert np.array_equal(one.tps, again.tps) and one.a2 == again.a2
    acc.reset()
    assert len(acc) == 0
    cuts = [0, 1, 2, 65, 66, TILE + 3, 2 * TILE + 3, n - 1, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc.append(p[a:b], y[a:b])
    assert len(acc) == n
    many = acc.finish()
    for k in ("thresholds", "tps", "fps"):
        assert getattr(one, k).tobytes() == getattr(many, k).tobytes(), k
    assert (one.a2, one.n_correct, one.n_pos) == (many.a2, many.n_correct, many.n_pos)
    acc.reset()
    p2, y2 = _scores(rng, 1000, "plain")
    acc.append(p2, y2)
    _check_against_sklearn(acc.finish(), p2, y2, "after reset")


def test_refusals_on_the_device(acc):
    from citlab_article_separation_new_amd import _lib
    acc.reset()
    with pytest.raises(ValueError, match="at least one pair"):
        acc.finish()
    for bad in (np.nan, -0.25, 1.5, np.inf):
        acc.reset()
        acc.append(np.array([0.1, bad, 0.9], np.float32), [0, 1, 1])
        with pytest.raises(ValueError, match="outside"):
            acc.finish()
    acc.reset()
    with pytest.raises(ValueError):
        acc.append(np.array([0.1, 0.2], np.float32), [0, 2])
    with pytest.raises(ValueError, match="2\\^31"):
        acc.reserve(1 << 31)
    lib = _lib.load_library()
    rc = lib.asep_releval_reserve(acc._h, 1 << 31, None)
    assert rc == -4 and "2^31" in _lib.last_error()                  # ASEP_ERR_UNSUPPORTED, with the reason
    acc.reset()


def test_append_page_builds_the_labels_of_build_full_relations(acc):
    """the device-resident page append: last class column, labels from gt rows (duplicates harmless), three classes"""
    import torch
    from citlab_article_separation_new_amd.gnn_input import build_full_relations
    rng = np.random.default_rng(9)
    acc.reset()
    ps, ys = [], []
    for N, nc in ((1, 2), (7, 2), (40, 3), (131, 2)):
        probs = rng.random((N * N, nc)).astype(np.float32)
        pairs = rng.integers(0, N, size=(max(1, N * N // 5), 2))
        gt = np.concatenate([np.full((len(pairs), 1), 5), pairs], axis=1).astype(np.int32)
        gt = np.concatenate([gt, gt[:3]])                            # duplicates
        _, _, lab = build_full_relations(N, gt)
        acc.append_page(torch.from_numpy(probs).cuda(), N, gt)
        ps.append(probs[:, -1])
        ys.append(lab)
    N = 5
    acc.append_page(torch.from_numpy(np.full((N * N, 2), 0.25, np.float32)).cuda(), N, np.zeros((0, 3), np.int32))   # no GT rows
    ps.append(np.full(N * N, 0.25, np.float32))
    ys.append(np.zeros(N * N, np.int32))
    _check_against_sklearn(acc.finish(), np.concatenate(ps), np.concatenate(ys), "append_page")
    with pytest.raises(IndexError):
        acc.append_page(torch.zeros(4, 2).cuda(), 2, np.array([[0, 1, 2]], np.int32))
    acc.reset()
    acc.append_page(torch.zeros(4, 2).cuda(), 2, torch.tensor([[0, 1, 2]], dtype=torch.int32).cuda())   # unchecked on the host
    with pytest.raises(IndexError):
        acc.finish()
    acc.reset()


@pytest.mark.parametrize("n", [(1 << 24) + 3, 40_000_000])
def test_large_lists(n):
    """2^24 + 3 pairs, and the 40 M pairs a 1000-page list of 200-block pages reaches"""
    from citlab_article_separation_new_amd.lav_rel import RelationEval
    rng = np.random.default_rng(n % 1000)
    y = (rng.random(n) < 0.05).astype(np.int32)
    p = rng.random(n, dtype=np.float32)
    p = np.where(y == 1, np.sqrt(p), p * p).astype(np.float32)
    p[::1000] = 0.5                                                  # a long run of ties in the middle
    acc = RelationEval(0)
    acc.reserve(n)
    acc.append(p, y)
    curve = acc.finish()
    print({k: round(v, 1) for k, v in acc.stage_us().items()})
    acc.close()
    _check_against_sklearn(curve, p, y, f"n={n}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------
_NOT_RESULTS = ("Time: ", "Using pb_path", "Could not find gpu-model-pb-file")     # wall time and model resolution


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _gt_rows(member):
    same = (member[:, None] == member[None, :]) & (member[:, None] >= 0) & ~np.eye(len(member), dtype=bool)
    i, j = np.nonzero(same)
    rows = np.stack([np.zeros_like(i), i, j], axis=1)
    return np.concatenate([rows, rows[:2]]).tolist()                 # with two duplicates


def _expected_lines(argv, num=20, separated=True):
    """sklearn (as lav_rel.py:190-229 calls it) on the probabilities of the host-returning forward of the same pages"""
    import sklearn.metrics as sk
    from citlab_article_separation_new_amd import gnn_io, lav_rel
    from citlab_article_separation_new_amd.gnn_input import build_full_relations
    flags = lav_rel.parse_flags(argv)
    from citlab_article_separation_new_amd.run_gnn_clustering import resolve_model_path
    graph = gnn_io.load_graph(resolve_model_path(flags), visual_layers=flags.visual_layers or None)
    targets, probs = [], []
    for path in [p for p in open(flags.eval_list).read().split("\n") if p]:
        feed, n, gt = lav_rel._prepare_eval_page(tuple(argv), path)
        a = lav_rel._feed_arrays(feed, graph.cfg)
        if graph.cfg.visual_dims:
            out = gnn_io.gnn_forward_visual(graph, n, a["edges"], a["u"], a["ef"], a["image"], a["regions"], a["npts"])
        else:
            out = gnn_io.gnn_forward(graph, n, a["edges"], a["u"], a["ef"])
        targets.append(build_full_relations(n, gt)[2][None])
        probs.append(out[None][:, :, -1])
    graph.close()
    full_targets = np.squeeze(np.concatenate(targets, axis=-1))
    full_probs = np.squeeze(np.concatenate(probs, axis=-1))
    prec, rec, thr = sk.precision_recall_curve(full_targets, full_probs)
    lines = lav_rel.table_lines(prec, rec, thr, num)
    lines.append(f"AUC-ROC: {sk.roc_auc_score(full_targets, full_probs):12f}")
    lines.append(f"Accuracy: {sk.accuracy_score(full_targets, full_probs > 0.5):12f}")
    assert 0 < full_targets.sum() < len(full_targets)
    if separated:                                                    # planted articles: the net tells them apart, mostly
        assert 0.05 < full_targets.mean() < 0.95 and len(thr) > 100
    return lines, full_targets, full_probs


def _evaluate(argv):
    from citlab_article_separation_new_amd import lav_rel
    cap = _Capture()
    root = logging.getLogger()
    level = root.level
    root.addHandler(cap)
    root.setLevel(logging.INFO)
    try:
        curve = lav_rel.LavGNN(argv=argv).evaluate()
    finally:
        root.removeHandler(cap)
        root.setLevel(level)
    return curve, cap.lines


def _geometric_inputs(tmp_path):
    from citlab_article_separation_new_amd import pb_import
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import gnn_article_cases as gac
    from oracle import gnn_cases
    case = next(c for c in gac.CASES if c["name"] == "n60")
    g0, w, cfg, _ = gac.build(case)
    model = tmp_path / "model" / "export"
    model.mkdir(parents=True)
    (model / "gnn_best_2026.pb").write_bytes(pb_import.weights_to_graphdef(w, "graph/", meta={"num_transition_steps": 3}))
    data = tmp_path / "data" / "json15d2bb"
    data.mkdir(parents=True)
    mask = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
    keep = [i for i, m in enumerate(mask) if m]
    graphs = [g0, gnn_cases.planted_graph(91, N=25, n_pairs=150, n_articles=3, n_outliers=1),
              gnn_cases.planted_graph(92, N=9, n_pairs=20, n_articles=2, n_outliers=1),
              gnn_cases.planted_graph(93, N=41, n_pairs=300, n_articles=4, n_outliers=2)]
    paths = []
    for k, g in enumerate(graphs):
        n = int(g["num_nodes"])
        feats15 = np.random.default_rng(k).random((n, 15)).astype(np.float32)
        feats15[:, keep] = g["node_features"]
        gt = _gt_rows(np.asarray(g["planted"]))
        jp = data / f"page{k}.json"
        jp.write_text(json.dumps({"num_nodes": n, "interacting_nodes": g["interacting_nodes"].tolist(),
                                  "num_interacting_nodes": int(g["interacting_nodes"].shape[0]), "node_features": feats15.tolist(),
                                  "edge_features": g["edge_features"].tolist(), "gt_relations": gt, "gt_num_relations": len(gt)}))
        paths.append(str(jp))
    lst = tmp_path / "eval.lst"
    lst.write_text("\n".join(paths) + "\n")
    return ["--model_dir", str(tmp_path / "model"), "--eval_list", str(lst), "--input_params", "node_feature_dim=15",
            "edge_feature_dim=2", "node_input_feature_mask=" + str(mask).replace(" ", "")]


def test_evaluate_end_to_end_geometric_net(tmp_path):
    argv = _geometric_inputs(tmp_path)
    expect, y, p = _expected_lines(argv)
    curve, lines = _evaluate(argv + ["--gpu_devices", "0"])
    body = [ln for ln in lines if not ln.startswith(_NOT_RESULTS)]
    assert body == ["Start evaluation..."] + expect + ["Evaluation finished."]
    _check_against_sklearn(curve, p, y, "end to end")
    # host workers around the GPU owner, a page limit, another number of table rows
    expect7, _, _ = _expected_lines(argv, num=7)
    _, lines = _evaluate(argv + ["--num_workers", "2", "--num_p_r_thresholds", "7"])
    assert [ln for ln in lines if not ln.startswith(_NOT_RESULTS)] == ["Start evaluation..."] + expect7 + ["Evaluation finished."]
    _, lines = _evaluate(argv + ["--batch_limiter", "2"])
    assert [ln for ln in lines if not ln.startswith(_NOT_RESULTS)][1] == "Stop validation after 2 batches with"
    with pytest.raises(ValueError, match="sample_relations"):
        _evaluate(argv + ["--sample_relations", "True"])


def test_command_line_in_a_child_process(tmp_path):
    argv = _geometric_inputs(tmp_path)
    expect, _, _ = _expected_lines(argv)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "citlab_article_separation_new_amd.lav_rel"] + argv + ["--gpu_devices", "0"], env=env,
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    logged = [ln.split(":", 2)[2] if ln.startswith("INFO:root:") else ln for ln in r.stderr.split("\n")]
    at = logged.index("Relative Thresholds:")
    assert logged[at:at + len(expect)] == expect
    assert "Running Evaluation." in logged and "Evaluation finished." in logged


def test_evaluate_end_to_end_visual_net(tmp_path):
    from citlab_article_separation_new_amd import synth
    N = 14
    argv = synth.write_gnn_cli_inputs(str(tmp_path), 3, visual=True, W=300, H=450, N=N)
    rng = np.random.default_rng(4)
    for k in range(3):
        jp = tmp_path / "data" / "json15d2bb" / f"p{k:03d}.json"
        d = json.loads(jp.read_text())
        gt = _gt_rows(rng.integers(-1, 3, size=N))
        d["gt_relations"], d["gt_num_relations"] = gt, len(gt)
        jp.write_text(json.dumps(d))
    expect, y, p = _expected_lines(argv, separated=False)
    curve, lines = _evaluate(argv)
    body = [ln for ln in lines if not ln.startswith(_NOT_RESULTS)]
    assert body == ["Start evaluation..."] + expect + ["Evaluation finished."]
    _check_against_sklearn(curve, p, y, "end to end, visual")
