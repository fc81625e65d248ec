"""Host side of the article separation measure (no GPU): the tolerance rule, the sparse greedy alignment against the
dense argmax loop, weighting and greedy sums from the reference's recorded matrices (tests/golden/measure_golden.json),
f_measure, the early returns and prints of run_eval fed with recorded matrices, the list filter / sort, the parser's
defaults, the ValueError cases and run_measure's stdout from recorded tuples."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from citlab_article_separation_new_amd import measure, run_measure  # noqa: E402
import measure_cases as mc  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "measure_golden.json")))
CASE_MODES = [(c, m) for c in GOLD["cases"] for m in c["modes"]]
IDS = [f"{c['name']}-{m}" for c, m in CASE_MODES]


def test_tolerance_rule():
    # 250 ("not below max_d") and an exact 0 both take the mean of the others; larger ones are cut to the mean
    assert measure.tols_from_distances([250.0, 30.0, 0.0, 50.0, 100.0]) == [15.0, 7.5, 15.0, 12.5, 15.0]
    assert measure.tols_from_distances([250.0, 250.0]) == [62.5, 62.5]
    assert measure.tols_from_distances([]) == []
    assert measure.tols_from_distances([10.0, 20.0], rel_tol=1.0) == [10.0, 15.0]
    s = (0.1 + 0.2 + 0.7) / 3                       # summed in list order, as the reference does
    assert measure.tols_from_distances([0.1, 0.2, 0.7]) == [0.1 * 0.25, 0.2 * 0.25, s * 0.25]


def _dense_greedy(matrix):
    """eval_measure.py:108-123 / run_measure.py:115-135 on a dense matrix: chosen (row, col) in order"""
    m, out = np.array(matrix, float), []
    while True:
        r, c = np.unravel_index(np.argmax(m), m.shape)
        if m[r, c] < 0:
            return out
        out.append((int(r), int(c)))
        m[r, :] = -1.0
        m[:, c] = -1.0


@pytest.mark.parametrize("seed", range(8))
def test_sparse_greedy_equals_dense(seed):
    rng = np.random.default_rng(seed)
    shape = (int(rng.integers(1, 30)), int(rng.integers(1, 30)))
    dense = np.zeros(shape)
    k = int(rng.integers(0, shape[0] * shape[1]))
    rows, cols = rng.integers(0, shape[0], k), rng.integers(0, shape[1], k)
    dense[rows, cols] = rng.choice([0.0, 0.25, 0.5, 1.0, 0.123, 0.77], k)          # many ties, zeros among the candidates
    rr, cc = np.nonzero(dense >= 0)
    keep = (dense[rr, cc] > 0) | (rng.random(len(rr)) < 0.1)                        # candidates: all non-zero entries, some zeros
    rr, cc = rr[keep], cc[keep]
    ref = _dense_greedy(dense)
    precision_ref = np.zeros(shape[0])
    for r, c in ref:
        precision_ref[r] = dense[r, c]
    got = measure.precision_from_pairs(1, shape[0], rr, cc, dense[rr, cc][:, None])
    assert np.array_equal(got[0], precision_ref)
    chosen = [(int(rr[i]), int(cc[i])) for i in measure.greedy_alignment(rr, cc, dense[rr, cc], inclusive=True)]
    assert chosen == [e for e in ref if dense[e] > 0]
    s = 0
    for e in ref:
        s += dense[e]
    assert measure.get_greedy_sum(dense) == s


def _jobs(c, mode):
    """(bd tuple, r_matrix, p_matrix) as the reference recorded them"""
    g = c["modes"][mode]
    jobs = list(g["jobs"])
    n_gt, n_hy = sum(len(v) for _, v in c["gt"]), sum(len(v) for _, v in c["hy"])
    n_gt_id = sum(len(v) for k, v in c["gt"] if k is not None)
    n_hy_id = sum(len(v) for k, v in c["hy"] if k is not None)
    bd = []
    for nt, nr in ((n_gt, n_hy), (n_gt_id, n_hy_id)):
        if nt == 0:
            bd += [None, None]
        elif nr == 0:
            bd += [0, 0]
        else:
            j = jobs.pop(0)
            assert (j["n_truth"], j["n_reco"]) == (nt, nr)
            bd += [j["R"], j["P"]]
    a_gt, a_hy = sum(k is not None for k, _ in c["gt"]), sum(k is not None for k, _ in c["hy"])
    shape = (a_gt, a_hy) if jobs else (0, 0)
    return tuple(bd), np.array([j["R"] for j in jobs]).reshape(shape), np.array([j["P"] for j in jobs]).reshape(shape)


@pytest.mark.parametrize("c,mode", CASE_MODES, ids=IDS)
def test_run_eval_from_recorded_matrices(c, mode):
    """evaluate() fed with the recorded page values: the reference's prints, early returns, weighting, greedy sums and
    tuples, bit for bit"""
    g = c["modes"][mode]
    bd, r_matrix, p_matrix = _jobs(c, mode)
    prep = measure._Prepared(mc.as_dict(c["gt"]), mc.as_dict(c["hy"]), 5, mode == "dyn")
    gt_w = [float(len(v)) for k, v in c["gt"] if k is not None]
    hy_w = [float(len(v)) for k, v in c["hy"] if k is not None]
    if g["weighted"]:
        wr, wp = measure.weight_matrices(r_matrix, p_matrix, gt_w, hy_w)
        assert wr.tolist() == g["weighted"][0] and wp.tolist() == g["weighted"][1]
        assert measure.get_greedy_sum(wr) == g["tuples"][2][0] and measure.get_greedy_sum(wp) == g["tuples"][2][1]
    lines = []
    tuples = measure.evaluate(prep, None, log=lambda *a: lines.append(" ".join(str(x) for x in a)),
                              matrices=(lambda p, r: bd, lambda p, r: (r_matrix, p_matrix, gt_w, hy_w)))
    assert "\n".join(lines) + "\n" == g["stdout"]
    assert [None if t is None else [float(v) for v in t] for t in tuples] == g["tuples"]


def test_early_returns_are_covered():
    kinds = {tuple(t is None for t in c["modes"][m]["tuples"]) for c, m in CASE_MODES}
    assert kinds == {(True, True, True), (False, True, True), (False, False, False)}
    assert any(c["modes"][m]["tuples"][2] == [0, 0, 0] and c["modes"][m]["tuples"][0][0] > 0 for c, m in CASE_MODES)   # no HY articles
    assert any(c["modes"][m]["tuples"][0] == [0, 0, 0] for c, m in CASE_MODES)                                         # no HY baselines


def test_f_measure():
    assert measure.f_measure(0, 0) == 0.0 and measure.f_measure(precision=0.0, recall=0.0) == 0.0
    assert measure.f_measure(precision=0.5, recall=1.0) == 2.0 * 0.5 * 1.0 / 1.5
    for c, m in CASE_MODES:
        for t in c["modes"][m]["tuples"]:
            if t is not None:
                assert measure.f_measure(recall=t[0], precision=t[1]) == t[2]


def test_baseline_measure_averaging():
    bm = measure.BaselineMeasure()
    job = GOLD["cases"][0]["modes"]["fix"]["jobs"][0]
    bm.add_per_dist_tol_tick_per_line_recall(np.array(job["recall"]))
    bm.add_per_dist_tol_tick_per_line_precision(np.array(job["precision"]))
    bm.add_per_dist_tol_tick_per_line_recall(np.ones((5, 3)))
    r = bm.result
    assert r.page_wise_recall[0] == job["R"] and r.page_wise_precision[0] == job["P"]
    assert r.recall == (0.0 + job["R"] + 1.0) / 2 and r.precision == job["P"]
    assert r.page_wise_per_dist_tol_tick_recall[1].tolist() == [1.0] * 5
    assert len(r.page_wise_per_dist_tol_tick_per_line_precision) == 1


def test_filter_and_sort():
    gt = ["/d/gt/b_page.xml", "/d/gt/a_page.xml"]
    hy = ["/x/hy/c_other.xml", "/x/hy/b_page_clustered.xml", "/x/hy/a_page.xml", "/x/hy/zz_a_page.xml"]
    g, h = run_measure.filter_and_sort(gt, hy)
    assert g == ["/d/gt/a_page.xml", "/d/gt/b_page.xml"]
    assert h == ["/x/hy/a_page.xml", "/x/hy/b_page_clustered.xml", "/x/hy/zz_a_page.xml"]


def test_parser_defaults_and_line_files(tmp_path):
    f = run_measure.build_parser().parse_args(["--path_to_gt_xml_lst", "g", "--path_to_hy_xml_lst", "h"])
    assert (f.min_tol, f.max_tol, f.rel_tol, f.poly_tick_dist, f.verbose, f.num_threads) == (-1, -1, 0.25, 5, True, 1)
    cfg = tmp_path / "flags"
    cfg.write_text("--path_to_gt_xml_lst = g # the ground truth\n--path_to_hy_xml_lst h\n--verbose false\n--min_tol 10 --max_tol 30\n")
    f = run_measure.build_parser().parse_args(["@" + str(cfg)])
    assert (f.path_to_gt_xml_lst, f.verbose, f.min_tol, f.max_tol) == ("g", False, 10, 30)
    with pytest.raises(SystemExit):
        run_measure.build_parser().parse_args(["--path_to_gt_xml_lst", "g"])


@pytest.mark.parametrize("lo,hi", [(0, 0), (0, 10), (-1, 5), (-2, -2), (-5, -1), (20, 10)])
def test_unsupported_tolerances(lo, hi):
    with pytest.raises(ValueError, match="not restated"):
        measure.BaselineMeasureEval(lo, hi)
    with pytest.raises(ValueError):
        run_measure.run_measure([], [], lo, hi, 0.25, 5, log=lambda *a: None)


def test_supported_tolerances():
    assert measure.BaselineMeasureEval(-1, -1).max_tols.tolist() == [-1]
    assert measure.BaselineMeasureEval().max_tols.tolist() == list(range(10, 31))
    assert measure.BaselineMeasureEval(7, 7).max_tols.tolist() == [7]
    with pytest.raises(AssertionError):
        measure.BaselineMeasureEval(10, 30, rel_tol=0.0)


@pytest.mark.parametrize("key", sorted(GOLD["file_lists"]))
def test_run_measure_stdout_from_recorded_tuples(key, monkeypatch):
    """run_measure's per-file blocks, table rows, dashes, averages and counters, with the device part replaced by the
    recorded run_eval output of each file"""
    rec = GOLD["file_lists"][key]
    cases = {c["name"]: c for c in GOLD["cases"]}
    names = iter(rec["names"])
    monkeypatch.setattr(measure, "get_data_from_pagexml", lambda path: path)
    monkeypatch.setattr(measure, "run_eval_dicts", lambda pairs, *a, **k: [(p, None) for p in pairs])

    def evaluate(prep, res, log=print):
        g = cases[next(names)]["modes"][rec["mode"]]
        log(g["stdout"][:-1])
        return [None if t is None else tuple(t) for t in g["tuples"]]
    monkeypatch.setattr(measure, "evaluate", evaluate)
    lines = []
    run_measure.run_measure([f"gt/{n}.xml" for n in rec["names"]], [f"hy/{n}.xml" for n in rec["names"]], *mc.MODES[rec["mode"]],
                            0.25, 5, rec["verbose"], log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    # (the reference's run_eval prints its count lines in quiet mode too: evaluate() above printed them)
    assert "\n".join(lines) + "\n" == rec["stdout"]


def test_lists_of_different_length_exit_1():
    lines = []
    with pytest.raises(SystemExit) as e:
        run_measure.run_measure(["a.xml", "b.xml"], ["a.xml"], -1, -1, 0.25, 5, log=lines.append)
    assert e.value.code == 1 and lines == ["Length of GT list (2) has to match length of HY list (1)!"]
