"""Host side of the relation net evaluation (lav_rel): flags, curve / F scores / tables / log text from (thresholds, tps, fps)
counts against the golden of the imported reference (tests/golden/lav_rel_golden.json, sklearn 1.7.2) and against the
installed sklearn called directly, the key packing, the refusals, and the error without a GPU."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import lav_rel_cases as lc  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "lav_rel_golden.json")))
CASES = {c["name"]: c for c in lc.cases()}


def _bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _curve(gold):
    from citlab_article_separation_new_amd.lav_rel import RelationCurve
    return RelationCurve(np.array(gold["thresholds_desc"], np.float32), gold["tps"], gold["fps"], gold["n_correct"])


def _report(curve, num):
    from citlab_article_separation_new_amd import lav_rel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lav_rel.report_lines(curve, num)


def test_flags_match_the_reference():
    from citlab_article_separation_new_amd import lav_rel
    flags = lav_rel.parse_flags([])
    for name, default in GOLD["flags"].items():
        assert getattr(flags, name) == default, name
    f = lav_rel.parse_flags(["--gpu_devices", "1", "0", "--image_input", "--mvn", "False", "--num_p_r_thresholds", "7",
                             "--input_params", "node_feature_dim=15", "node_input_feature_mask=[1,0,1]", "--gpu_memory_fraction", "0.5"])
    assert f.try_gpu is True and f.gpu_devices == [1, 0] and f.image_input is True and f.mvn is False
    assert f.num_p_r_thresholds == 7 and f.input_params == {"node_feature_dim": 15, "node_input_feature_mask": [1, 0, 1]}


@pytest.mark.parametrize("gold", GOLD["cases"], ids=[c["name"] for c in GOLD["cases"]])
def test_curve_tables_and_log_equal_the_reference(gold):
    """from the recorded counts: precision / recall / thresholds bit-equal to what the reference's sklearn call returned, AUC
    and accuracy too, and every log line text for text"""
    from citlab_article_separation_new_amd import lav_rel
    curve = _curve(gold)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        prec, rec, thr = curve.precision_recall_curve()
        auc = curve.auc_roc
    assert prec.dtype == np.float64 and rec.dtype == np.float64 and thr.dtype == np.float32
    assert np.array_equal(_bits64(prec), _bits64(gold["precision"]))
    assert np.array_equal(_bits64(rec), _bits64(gold["recall"]))
    assert np.array_equal(thr.view(np.uint32), np.array(gold["thresholds"], np.float32).view(np.uint32))
    assert sorted({str(w.message) for w in caught}) == gold["warnings"]
    assert curve.accuracy == gold["accuracy"]
    k = len(gold["tps"]) + 1                                          # points of sklearn's ROC curve
    if np.isnan(gold["auc_roc"]):
        assert np.isnan(auc)
    else:
        assert abs(auc - gold["auc_roc"]) <= (k + 2) * 2.0 ** -53
    lines = _report(curve, gold["flags"]["num_p_r_thresholds"])
    body = [ln for ln in gold["log"] if ln not in ("Start evaluation...", "Evaluation finished.") and not ln.startswith("Stop validation")]
    assert lines == body
    assert lav_rel.f_scores(prec, rec).tolist() == lav_rel.f_scores(np.array(gold["precision"]), np.array(gold["recall"])).tolist()


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_and_text_equal_the_installed_sklearn(name):
    """the cases again, with sklearn called here as lav_rel.py:190-229 calls it: the golden's counts are what the public
    functions imply, and the report built from them equals one built from sklearn's own arrays"""
    import sklearn.metrics as sk
    from citlab_article_separation_new_amd import lav_rel
    gold = next(c for c in GOLD["cases"] if c["name"] == name)
    y, p = lc.concatenated(CASES[name])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prec, rec, thr = sk.precision_recall_curve(y, p)
        acc = sk.accuracy_score(y, p > 0.5)
        auc = sk.roc_auc_score(y, p)
    curve = _curve(gold)
    assert curve.n == len(y) and curve.n_pos == int(y.sum())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mine = curve.precision_recall_curve()
    for a, b in zip(mine, (prec, rec, thr)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    f = (2 * prec * rec) / np.where(prec + rec == 0, np.nan, prec + rec)
    f[np.isnan(f)] = 0
    assert lav_rel.f_scores(prec, rec).tobytes() == f.tobytes()
    num = gold["flags"]["num_p_r_thresholds"]
    expect = lav_rel.table_lines(prec, rec, thr, num) + [f"AUC-ROC: {auc:12f}", f"Accuracy: {acc:12f}"]
    assert _report(curve, num) == expect
    assert curve.accuracy == acc


def test_table_index_walks():
    from citlab_article_separation_new_amd import lav_rel
    assert lav_rel.relative_rows(6, 20) == [0] * 21                     # fewer thresholds than rows: every row is the first
    assert lav_rel.relative_rows(101, 20) == list(range(0, 101, 5))
    assert lav_rel.relative_rows(100, 20) == [4 * j for j in range(21)]
    thr = np.array([0.01, 0.04, 0.26, 0.5, 0.74, 0.76, 0.99], np.float32)
    assert lav_rel.fixed_rows(thr, 4) == [0, 2, 3, 5]                   # >= 0, 0.25, 0.5, 0.75; stops when j * step reaches 1
    assert lav_rel.fixed_rows(thr[:3], 4) == [0, 2]


def test_key_order_is_the_order_of_score_and_label():
    from citlab_article_separation_new_amd import lav_rel
    rng = np.random.default_rng(5)
    special = np.array([0.0, -0.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 0.5, np.nextafter(np.float32(0.5), np.float32(1)),
                        np.nextafter(np.float32(1), np.float32(0)), 1.0], np.float32)
    p = np.concatenate([special, special, rng.random(500).astype(np.float32), np.round(rng.random(200) * 4).astype(np.float32) / 4])
    y = rng.integers(0, 2, size=p.size)
    keys = lav_rel.pack_keys(p, y)
    assert keys.dtype == np.uint32
    p2, y2 = lav_rel.unpack_keys(keys)
    assert np.array_equal(p2, p) and np.array_equal(y2, y)              # (-0.0 == 0.0)
    order = np.argsort(keys, kind="stable")
    expect = np.lexsort((y, p))                                          # by score, then label
    assert np.array_equal(p[order], p[expect]) and np.array_equal(y[order], y[expect])
    lt = (p[:, None] < p[None, :]) | ((p[:, None] == p[None, :]) & (y[:, None] < y[None, :]))
    assert np.array_equal(keys[:, None] < keys[None, :], lt)
    for bad in (np.nan, -1e-3, 1.0000001, np.inf, -np.inf):
        with pytest.raises(ValueError):
            lav_rel.pack_keys(np.array([0.5, bad], np.float32), [0, 1])


def test_refusals():
    from citlab_article_separation_new_amd import lav_rel
    with pytest.raises(ValueError, match="at least one pair"):
        lav_rel.RelationCurve(np.zeros(0, np.float32), [], [], 0)
    with pytest.raises(ValueError, match="sample_relations"):
        lav_rel.check_flags(lav_rel.parse_flags(["--sample_relations", "True"]))
    with pytest.raises(ValueError, match="ModelRelation"):
        lav_rel.check_flags(lav_rel.parse_flags(["--model_type", "ModelOther"]))
    lav_rel.check_flags(lav_rel.parse_flags(["--gpu_memory_fraction", "0.3"]))
    # one class only: sklearn 1.7.2 (the yardstick) warns and returns nan; so does the curve
    one = lav_rel.RelationCurve(np.array([0.9, 0.1], np.float32), [0, 0], [1, 2], 1)
    with pytest.warns(lav_rel.UndefinedMetricWarning, match="Only one class"):
        assert np.isnan(one.auc_roc)
    with pytest.warns(UserWarning, match="No positive class"):
        prec, rec, _ = one.precision_recall_curve()
    assert rec.tolist() == [1.0, 1.0, 0.0] and prec.tolist() == [0.0, 0.0, 1.0]


def test_a_run_without_a_gpu_fails_with_the_engine_error(tmp_path):
    """no CPU fallback: with no device visible the command ends with the package's error (a child process, so that the
    test does the same on a machine that has a GPU)"""
    (tmp_path / "m.pb").write_bytes(b"")
    (tmp_path / "e.lst").write_text("")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "citlab_article_separation_new_amd.lav_rel", "--model_dir", str(tmp_path / "m.pb"),
                        "--eval_list", str(tmp_path / "e.lst")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "AsepError" in r.stderr and "no CPU fallback" in r.stderr, r.stderr[-2000:]
