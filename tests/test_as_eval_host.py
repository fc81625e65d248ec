"""as_eval.py against the reference's asCompTools (tests/golden/as_eval_golden.json, made by make_as_eval_golden.py): every
golden page pair as real PAGE-XML files, the winner tables, the CSV / sqlite round trips and the numpy ranking."""
import json
import os
import sqlite3
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN_DIR)

import as_eval_cases  # noqa: E402
from citlab_article_separation_new_amd import as_eval  # noqa: E402
from citlab_article_separation_new_amd.page_xml import Page  # noqa: E402

with open(os.path.join(GOLDEN_DIR, "as_eval_golden.json")) as _f:
    GOLDEN = json.load(_f)
FIELDS = ("gtNIs", "hypNIs", "corrects", "splits", "merges", "dist")


def _regions(table, per_region=3):
    """the table's lines in document order, a few per text region"""
    return [table[i:i + per_region] for i in range(0, len(table), per_region)]


def test_golden_matches_case_tables():
    cases = as_eval_cases.cases()
    assert [c["name"] for c in GOLDEN["cases"]] == [c[0] for c in cases] and len(cases) >= 30
    for g, (_, gt, hyp) in zip(GOLDEN["cases"], cases):
        assert [tuple(e) for e in g["gt"]] == gt and [tuple(e) for e in g["hyp"]] == hyp


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_comparison_equals_reference(case, tmp_path):
    gt = as_eval_cases.write_page(tmp_path / "gt.xml", _regions([tuple(e) for e in case["gt"]]), Page)
    hyp = as_eval_cases.write_page(tmp_path / "hyp.xml", _regions([tuple(e) for e in case["hyp"]], 2), Page)
    comper = as_eval.SepPageBlComper()
    comper.loadGT(gt)
    if "error" in case["expect"]:
        with pytest.raises(AssertionError, match=case["expect"]["message"]):
            comper.compareTo(hyp)
        assert as_eval.comparison_tables(hyp, gt)["inconsistent"]
        return
    res = comper.compareTo(hyp)
    assert {k: getattr(res, k) for k in FIELDS} == case["expect"]
    assert res.checkConsistency()
    assert comper.compareTo(hyp) == res                       # a second comparison re-uses the reduced ground truth
    # the tables the device comparison reads give the same counts when they are evaluated the way the kernel does
    t = as_eval.comparison_tables(hyp, gt)
    assert not t["inconsistent"]
    labels = [tl.get_article_id() for reg in Page(hyp).get_regions().get("TextRegion", []) for tl in reg.text_lines]
    pairs = {(int(g), l) for g, l in zip(t["line_gt"], labels) if g >= 0}
    corrects = sum(1 for b in t["blocks"] if len({labels[i] for i in b}) == 1 and labels.count(labels[b[0]]) == len(b))
    assert as_eval.SepPageComparison.from_counts(t["gtNIs"], len(set(labels)), len(pairs), corrects) == res


def _winner_dict():
    d = as_eval.SepPageCompDict()
    for p, row in enumerate(as_eval_cases.WINNER_TABLE):
        for m, (dist, corrects) in zip(as_eval_cases.WINNER_METHODS, row):
            c = as_eval.SepPageComparison()
            c.loadDict({"gtNIs": 5, "hypNIs": 5 - dist, "corrects": corrects, "splits": 0, "merges": -dist, "dist": dist})
            d.addItem("set", as_eval_cases.WINNER_GT.format(p=p), as_eval_cases.WINNER_HYP.format(m=m, p=p), c)
    return d


def test_winner_tables_equal_reference():
    d = _winner_dict()
    assert as_eval.SepPageCompDict.path2method(as_eval_cases.WINNER_HYP.format(m=as_eval_cases.WINNER_METHODS[0], p=0)) == \
        GOLDEN["winner"]["method_of_first"]
    ev = as_eval.CompDictEvaler(d)
    ev.calcWinnerDict()
    assert ev.winnerStatDict == GOLDEN["winner"]["winnerStatDict"]
    assert ev.winnerDict == GOLDEN["winner"]["winnerDict"]
    with pytest.raises(NotImplementedError, match="openpyxl"):
        ev.winnerStat2xlsx("x.xlsx")
    rows = ev.winner_csv_rows()
    assert rows[0][:2] == ["set", "run1/greedy_iter1000"] and rows[0][2:] == GOLDEN["winner"]["winnerDict"]["set"]["run1/greedy_iter1000"]


def test_numpy_ranking_equals_evaler():
    want = GOLDEN["winner"]["winnerStatDict"]["set"]
    table = np.array(as_eval_cases.WINNER_TABLE)
    got = as_eval.winner_all_counts(table[:, :, 0], table[:, :, 1])
    assert got.tolist() == [want["run1/" + m]["all"] for m in as_eval_cases.WINNER_METHODS]
    rng = np.random.default_rng(7)                               # a larger table with many ties, against the double loop
    dist, corrects = rng.integers(-3, 4, (9, 25)), rng.integers(0, 5, (9, 25))
    d = as_eval.SepPageCompDict()
    for p in range(9):
        for m in range(25):
            c = as_eval.SepPageComparison.from_counts(10, 10 - dist[p, m], 10, corrects[p, m])
            c.dist = int(dist[p, m])
            d.addItem("set", f"/gt/page/p{p}.xml", f"/w/run/a/b/clustering/m{m}/p{p}_clustering.xml", c)
    ev = as_eval.CompDictEvaler(d)
    ev.countWinnerStat()
    assert as_eval.winner_all_counts(dist, corrects).tolist() == [ev.winnerStatDict["set"][f"run/m{m}"]["all"] for m in range(25)]


def test_csv_sqlite_and_cleanup(tmp_path):
    d = _winner_dict()
    path = tmp_path / "comparison.csv"
    d.expCsv(path)
    lines = path.read_text().splitlines()
    assert lines[0] == "dataSet,method,gtXML,hypXML,gtNIs,hypNIs,corrects,splits,merges,dist" and len(lines) == 13
    methods = ["run1/" + m.lower() for m in as_eval_cases.WINNER_METHODS]
    back = as_eval.SepPageCompDict()
    back.loadCSV(path, methods)
    assert back == d
    part = as_eval.SepPageCompDict()
    part.loadCSV(path, methods[:1])
    assert sum(len(g) for g in part["set"].values()) == 3
    db = tmp_path / "c.sqlite"
    d.expSqlite(db, "allComps")
    con = sqlite3.connect(str(db))
    rows = con.execute("SELECT method, dist, corrects FROM allComps").fetchall()
    con.close()
    assert len(rows) == 12 and rows[0] == ("run1/" + as_eval_cases.WINNER_METHODS[0], 0, 5)
    d.cleanup(["run1/greedy_iter1000"])
    assert sum(c is not None for g in d["set"].values() for c in g.values()) == 3
    ev = as_eval.CompDictEvaler(d)
    ev.countWinnerStat()
    assert ev.winnerStatDict == {"set": {"run1/greedy_iter1000": {"all": 3, "run1/greedy_iter1000": 3}}}
