"""Article separation measure on the GPU: the distance histograms of both kernels against a loop-for-loop numpy
restatement bit for bit (golden cases and fuzzed pages, several file pairs per call, empty and one-polygon sides); the
per-line precision / recall, page values, article matrices and result tuples against the reference's Python path
(tests/golden/measure_golden.json) within the derived bound; the sparse-candidates claim at the 3 * tol_max border;
determinism; run_measure end to end; and run_baseline_clustering's output scored against itself.

Accuracy bound (derived, not measured): a per-line value is a sum of n terms in [0, 1] divided by n, each term carrying
at most three roundings, so |gpu - ref| <= (n + 3) * 2^-52 for a polygon of n points; page values, matrices and tuples
get the same bound with n = the largest polygon plus the number of values averaged.
Every GPU step runs in a child process (this file, run as a script) under a time limit."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPS = 2.0 ** -52


def _child(check, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), check, *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, f"{check} failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def test_histograms_golden_cases():
    assert "ok" in _child("hist_golden")


def test_histograms_fuzz():
    assert "ok" in _child("hist_fuzz", timeout=1200)


def test_golden_values():
    out = _child("golden")
    print(out)
    assert "ok" in out


def test_sparse_border():
    assert "ok" in _child("border")


def test_determinism():
    assert "ok" in _child("determinism")


def test_baseline_measure_eval_class():
    assert "ok" in _child("eval_class")


def test_run_measure_command_line(tmp_path):
    assert "ok" in _child("cli", str(tmp_path), timeout=900)


def test_clustering_output_scores_one(tmp_path):
    assert "ok" in _child("chain", str(tmp_path), timeout=900)


# ---- the checks, run in the child -------------------------------------------------------------------------------------

def _gold():
    return json.load(open(os.path.join(HERE, "golden", "measure_golden.json")))


def _slow(prep, dmax):
    """eval_measure.py:125-258 restated loop for loop on the prepared pair: {(i, j): histogram}, {(j, a): histogram},
    [j][2] histograms; histograms over min(d, dmax + 1)."""
    import numpy as np
    T, R = prep.truth, prep.reco

    def cand(a, b):
        gx = max(a[0], b[0]) - min(a[0] + a[2] - 1, b[0] + b[2] - 1)
        gy = max(a[1], b[1]) - min(a[1] + a[3] - 1, b[1] + b[3] - 1)
        return gx <= dmax and gy <= dmax

    def mins(count, ref):
        dx = abs(np.asarray(count[0]) - np.expand_dims(np.asarray(ref[0]), 1))
        dy = abs(np.asarray(count[1]) - np.expand_dims(np.asarray(ref[1]), 1))
        return np.amin(dx + dy, axis=0)

    def hist(d):
        return np.bincount(np.minimum(d, dmax + 1), minlength=dmax + 2).astype(np.uint32)
    pairs, recs, truth = {}, {}, []
    for i in range(R.n):
        for j in range(T.n):
            if cand(R.boxes[i], T.boxes[j]):
                pairs[(i, j)] = hist(mins(R.polys[i], T.polys[j]))
    for j in range(T.n):
        n = len(T.polys[j][0])
        m_all, m_id = np.full(n, dmax + 1), np.full(n, dmax + 1)
        for a in range(len(prep.hy_ids)):
            members = [i for i in np.flatnonzero(prep.r_art == a) if cand(T.boxes[j], R.boxes[i])]
            if not members:
                continue
            m = np.full(n, dmax + 1)
            for i in members:
                m = np.minimum(m, mins(T.polys[j], R.polys[i]))
            recs[(j, a)] = hist(m)
            m_all = np.minimum(m_all, m)
            if prep.hy_ids[a] is not None:
                m_id = np.minimum(m_id, m)
        truth.append([hist(m_all), hist(m_id)])
    return pairs, recs, truth


def _compare_hist(preps, results):
    """the histograms of device_rel_hits(preps, want_hist=True) against _slow, exactly (shared with
    test_measure_seams_gpu.py, which sets tolerances of its own on the prepared pairs).  Returns the number of candidate
    pairs and _slow's three results per file pair."""
    import numpy as np
    n_pairs, slow = 0, []
    for prep, res in zip(preps, results):
        sp, sr, st = _slow(prep, res.dmax)
        slow.append((sp, sr, st))
        got_p = {(int(i), int(j)): h for i, j, h in zip(res.pair_i, res.pair_j, res.pair_hist)}
        got_r = {(int(j), int(a)): h for j, a, h in zip(res.rec_j, res.rec_a, res.rec_hist)}
        assert sorted(got_p) == sorted(sp) and list(got_p) == sorted(got_p), "candidate pairs differ"
        assert sorted(got_r) == sorted(sr) and list(got_r) == sorted(got_r), "candidate records differ"
        assert all(np.array_equal(got_p[k], sp[k]) for k in sp), "pair histograms differ"
        assert all(np.array_equal(got_r[k], sr[k]) for k in sr), "record histograms differ"
        assert all(np.array_equal(res.truth_hist[j][u], st[j][u]) for j in range(prep.truth.n) for u in (0, 1)), "truth histograms differ"
        n_pairs += len(sp)
    return n_pairs, slow


def _check_hist(pairs, mode):
    from citlab_article_separation_new_amd import measure
    import measure_cases as mc
    preps = measure.prepare(pairs, *mc.MODES[mode], 0.25, 5)
    return _compare_hist(preps, measure.device_rel_hits(preps, want_hist=True))[0]


def check_hist_golden():
    import measure_cases as mc
    cases = _gold()["cases"]
    pairs = [(mc.as_dict(c["gt"]), mc.as_dict(c["hy"])) for c in cases]
    n = _check_hist(pairs, "dyn") + _check_hist(pairs, "fix") + sum(_check_hist([p], "fix_wide") for p in pairs[:3])
    print("ok", n, "pairs")


def check_hist_fuzz():
    import random
    import measure_cases as mc
    import textblock_cases as tc
    rng = random.Random(2020)
    total = 0
    for rnd, sizes in enumerate([(2, 1, 0, 17), (60, 5, 33), (400,), (1, 120, 3)]):
        pairs = []
        for k, n in enumerate(sizes):
            page = tc.random_page(1000 * rnd + k, n, 1200 + 4 * n, 1600 + 6 * n, 300) if n else []
            gt, hy = mc.make_pair(page, rng.randint(0, 10 ** 6), per_article=rng.randint(1, 9), regroup=rng.randint(1, 9),
                                  drop=rng.choice([0.0, 0.1, 0.5]), extra=rng.randint(0, 3), far=rng.random() < 0.5, dup=n > 1)
            if n == 1:
                hy = hy[:1] and [[hy[0][0], hy[0][1][:1]]]        # a one-polygon side
            if k % 3 == 2:
                gt, hy = hy, gt
            pairs.append((mc.as_dict(gt), mc.as_dict(hy)))
        pairs.append(({}, pairs[0][1]))                           # empty truth
        pairs.append((pairs[0][0], {}))                           # empty reco
        total += _check_hist(pairs, "dyn" if rnd % 2 == 0 else "fix")
    print("ok", total, "pairs")


def _bound(n_points, n_values=0):
    return (n_points + 3 + n_values) * EPS


def check_golden():
    import numpy as np
    from citlab_article_separation_new_amd import measure
    import measure_cases as mc
    worst = {"per_line": 0.0, "page": 0.0, "matrix": 0.0, "tuple": 0.0}

    def close(got, ref, bound, key, what):
        got, ref = np.asarray(got, float), np.asarray(ref, float)
        assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
        d = np.abs(got - ref)
        if d.size:
            worst[key] = max(worst[key], float(d.max()))
        assert np.all(d <= bound), f"{what}: |gpu - ref| = {float((d - bound).max() + np.max(bound)):.3e} above the bound"
    for mode in mc.MODES:
        cases = [c for c in _gold()["cases"] if mode in c["modes"]]
        pairs = [(mc.as_dict(c["gt"]), mc.as_dict(c["hy"])) for c in cases]
        for c, (prep, res) in zip(cases, measure.run_eval_dicts(pairs, *mc.MODES[mode], 0.25, 5)):
            g = c["modes"][mode]
            what = f"{c['name']}/{mode}"
            if "normed_truth" in c:
                assert [[list(map(int, xs)), list(map(int, ys))] for xs, ys in prep.truth.polys] == c["normed_truth"], what
                assert [[list(map(int, xs)), list(map(int, ys))] for xs, ys in prep.reco.polys] == c["normed_reco"], what
            t_n = np.array([len(xs) for xs, _ in prep.truth.polys] or [0])
            r_n = np.array([len(xs) for xs, _ in prep.reco.polys] or [0])
            n_max = int(max(t_n.max(), r_n.max()))
            jobs = iter(g["jobs"])
            subsets = [(np.arange(prep.truth.n), np.arange(prep.reco.n)), (np.flatnonzero(prep.t_has_id), np.flatnonzero(prep.r_has_id))]
            for kind, (ti, ri) in enumerate(subsets):
                if len(ti) == 0 or len(ri) == 0:
                    continue
                job = next(jobs)
                if job["tols"] is not None:
                    assert prep.tols[ti, kind].tolist() == job["tols"], f"{what}: tolerances of job {kind}"
                p, r = measure.job_matrices(prep, res, ti, ri, kind)
                close(p, job["precision"], _bound(r_n[ri])[None, :], "per_line", what + " precision")
                close(r, job["recall"], _bound(t_n[ti])[None, :], "per_line", what + " recall")
                rr, pp = measure._page_rp(p, r)
                close([rr, pp], [job["R"], job["P"]], _bound(n_max, max(len(ti), len(ri)) + p.shape[0]), "page", what + " page")
            rest = list(jobs)
            if rest:
                rm, pm, gw, hw = measure.article_matrices(prep, res)
                ref_r = np.array([j["R"] for j in rest]).reshape(rm.shape)
                ref_p = np.array([j["P"] for j in rest]).reshape(pm.shape)
                if rest[0]["tols"] is not None:
                    for g_idx, gid in enumerate(k for k in prep.gt_ids if k is not None):
                        ti = np.flatnonzero(prep.t_art == prep.gt_ids.index(gid))
                        assert prep.tols[ti, 2].tolist() == rest[g_idx * rm.shape[1]]["tols"], f"{what}: tolerances of article {gid}"
                nv = n_max + int(max(gw + hw)) + len(mc.MODES[mode])
                close(rm, ref_r, _bound(nv), "matrix", what + " r_matrix")
                close(pm, ref_p, _bound(nv), "matrix", what + " p_matrix")
                wr, wp = measure.weight_matrices(rm, pm, gw, hw)
                close(wr, g["weighted"][0], _bound(nv), "matrix", what + " weighted r_matrix")
                close(wp, g["weighted"][1], _bound(nv), "matrix", what + " weighted p_matrix")
            lines = []
            tuples = measure.evaluate(prep, res, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
            assert "\n".join(lines) + "\n" == g["stdout"], f"{what}: stdout of run_eval"
            for got, ref in zip(tuples, g["tuples"]):
                assert (got is None) == (ref is None), what
                if ref is not None:
                    close(got, ref, _bound(n_max, prep.truth.n + prep.reco.n + 21), "tuple", what + " tuple")
    print("ok largest differences:", json.dumps(worst))


def check_border():
    """fixed tolerance 10..12: 3 * tol_max = 36.  A reco line 36 px from the truth line in x (or y) is a candidate whose
    nearest point scores (36 - 36) / 24 = 0 at tol 12; at 37 px it is no candidate.  Both score exactly 0, as the dense form does."""
    from citlab_article_separation_new_amd import measure
    truth = ([100, 300], [500, 500])
    for axis in "xy":
        for gap, expect in ((36, True), (37, False), (30, True)):
            reco = ([300 + gap, 500 + gap], [500, 500]) if axis == "x" else ([100, 300], [500 + gap, 500 + gap])
            prep = measure.prepare([({"a": [truth]}, {"h": [reco]})], 10, 12, 0.25, 5)[0]
            res = measure.device_rel_hits([prep], want_hist=True)[0]
            assert res.dmax == 36 and (len(res.pair_i) == 1) == expect, (axis, gap, res.pair_i)
            p, r = measure.job_matrices(prep, res, [0], [0], 0)
            if gap >= 36:
                assert not p.any() and not r.any(), (axis, gap, p, r)
            else:
                assert p.any() and r.any(), (axis, gap)
            if expect:
                assert int(res.pair_hist[0][:gap].sum()) == 0 and int(res.pair_hist[0][gap]) >= 1, (axis, gap)
    print("ok")


def check_determinism():
    import numpy as np
    from citlab_article_separation_new_amd import measure
    import measure_cases as mc
    c = next(c for c in _gold()["cases"] if c["name"] == "cols3")
    gt, hy = mc.as_dict(c["gt"]), mc.as_dict(c["hy"])
    first = hy["h0"][0]
    hy["h0"] = hy["h0"] + [first, (first[0][::-1], first[1][::-1])]          # a duplicate and a reversed duplicate
    n_reco = sum(len(v) for v in hy.values())
    for mode in ("dyn", "fix"):
        runs = []
        for _ in range(2):
            prep = measure.prepare([(gt, hy)], *mc.MODES[mode], 0.25, 5)[0]
            res = measure.device_rel_hits([prep])[0]
            runs.append((res.pair_i, res.pair_j, res.pair_hits, res.rec_j, res.rec_a, res.rec_hits, res.truth_hits))
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs differ"
        rows = {}
        for i, j, h in zip(*runs[0][:3]):
            rows.setdefault(int(i), {})[int(j)] = h.tobytes()
        dup = [i for i in range(prep.reco.n) if sorted(zip(*map(list, prep.reco.polys[i]))) == sorted(zip(*map(list, prep.reco.polys[0])))]
        assert len(dup) >= 3 and prep.reco.n == n_reco, dup
        assert all(rows[i] == rows[dup[0]] for i in dup), "duplicated baselines score differently"
    print("ok")


def check_eval_class():
    import numpy as np
    from citlab_article_separation_new_amd import measure
    import measure_cases as mc
    c = next(c for c in _gold()["cases"] if c["name"] == "cols2")
    truth = [q for _, v in c["gt"] for q in v]
    reco = [q for _, v in c["hy"] for q in v]
    for mode in ("dyn", "fix"):
        ev = measure.BaselineMeasureEval(*mc.MODES[mode])
        ev.calc_measure_for_page_baseline_polys(truth, reco)
        ev.calc_measure_for_page_baseline_polys(truth, truth)
        job = c["modes"][mode]["jobs"][0]
        res = ev.measure.result
        assert np.abs(res.page_wise_per_dist_tol_tick_per_line_recall[0] - np.array(job["recall"])).max() <= 1e-12
        assert abs(res.page_wise_recall[0] - job["R"]) <= 1e-12 and abs(res.page_wise_precision[0] - job["P"]) <= 1e-12
        assert res.page_wise_recall[1] == 1.0 and res.page_wise_precision[1] == 1.0
        assert abs(res.recall - (job["R"] + 1.0) / 2) <= 1e-12 and len(res.page_wise_per_dist_tol_tick_precision) == 2
    print("ok")


def _write_page(path, side):
    from citlab_article_separation_new_amd.page_xml import Page
    import xml.etree.ElementTree as ET
    page = Page(img_filename=os.path.basename(path)[:-4] + ".jpg", img_w=4000, img_h=6000)
    ns = page.page_node.tag.split("}")[0] + "}" if "}" in page.page_node.tag else ""
    region = ET.SubElement(page.page_node, ns + "TextRegion", {"id": "r1"})
    ET.SubElement(region, ns + "Coords", {"points": "0,0 3999,0 3999,5999 0,5999"})
    k = 0
    for aid, polys in side:
        for xs, ys in polys:
            k += 1
            attrs = {"id": f"l{k}"}
            if aid is not None:
                attrs["custom"] = "structure {id:%s; type:article;}" % aid
            line = ET.SubElement(region, ns + "TextLine", attrs)
            ET.SubElement(line, ns + "Coords", {"points": "0,0 1,0 1,1"})
            ET.SubElement(line, ns + "Baseline", {"points": " ".join(f"{x},{y}" for x, y in zip(xs, ys))})
    page.write_page_xml(path)


def _run_cli(cwd, *args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "citlab_article_separation_new_amd.run_measure", *args], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=timeout)


def check_cli(tmp):
    gold = _gold()
    cases = {c["name"]: c for c in gold["cases"]}
    os.makedirs(os.path.join(tmp, "gt"))
    os.makedirs(os.path.join(tmp, "hy"))
    import measure_cases as mc
    for key, rec in gold["file_lists"].items():
        for n in rec["names"]:
            _write_page(os.path.join(tmp, "gt", n + ".xml"), cases[n]["gt"])
            _write_page(os.path.join(tmp, "hy", n + ".xml"), cases[n]["hy"])
        # the lists in another order and with a HY file that matches no GT name: filtered and sorted as the reference does
        open(os.path.join(tmp, "gt.lst"), "w").write("".join(f"gt/{n}.xml\n" for n in reversed(sorted(rec["names"]))))
        open(os.path.join(tmp, "hy.lst"), "w").write("".join(f"hy/{n}.xml\n" for n in sorted(rec["names"]) + ["zzz_unrelated"]))
        lo, hi = mc.MODES[rec["mode"]]
        r = _run_cli(tmp, "--path_to_gt_xml_lst", "gt.lst", "--path_to_hy_xml_lst", "hy.lst", "--min_tol", str(lo), "--max_tol", str(hi),
                     "--verbose", str(rec["verbose"]), "--num_threads", "4")
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout == rec["stdout"], f"{key}: stdout differs\n--- got\n{r.stdout}\n--- expected\n{rec['stdout']}"
    # lists of different length: the message and exit status 1
    open(os.path.join(tmp, "gt.lst"), "w").write("gt/cols2.xml\ngt/cols3.xml\n")
    open(os.path.join(tmp, "hy.lst"), "w").write("hy/cols2.xml\n")
    r = _run_cli(tmp, "--path_to_gt_xml_lst", "gt.lst", "--path_to_hy_xml_lst", "hy.lst")
    assert r.returncode == 1 and r.stdout == "Length of GT list (2) has to match length of HY list (1)!\n", (r.returncode, r.stdout, r.stderr)
    # a .txt name: the reference's message, dashes, and the file counts as not valid
    open(os.path.join(tmp, "gt.lst"), "w").write("gt/cols2.txt\n")
    open(os.path.join(tmp, "hy.lst"), "w").write("hy/cols2.xml\n")
    r = _run_cli(tmp, "--path_to_gt_xml_lst", "gt.lst", "--path_to_hy_xml_lst", "hy.lst")
    assert r.returncode == 0 and "!! Ground truth and hypotheses file have to be in Page XML format !!\n" in r.stdout, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "{:<50s} {:>10s} {:>10s} {:>10s} {:>25d} {:>10d}".format(
        "article / block segmentation measure", "-", "-", "-", 0, 1)
    print("ok")


def check_chain(tmp):
    """baseline-only PAGE-XML -> run_baseline_clustering (article ids) -> scored against a copy of itself: 1, 1, 1"""
    import shutil
    import textblock_cases as tc
    from citlab_article_separation_new_amd import measure
    path = os.path.join(tmp, "page.xml")
    _write_page(path, [[None, [[list(xs), list(ys)] for xs, ys in tc.columns_page(21, n_cols=3, n_lines=10, extras=False)]]])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "citlab_article_separation_new_amd.run_baseline_clustering", "--path_to_xml_file", path],
                       cwd=tmp, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    shutil.copy(path, os.path.join(tmp, "copy.xml"))
    for lo, hi in ((-1, -1), (10, 30)):
        tuples = measure.run_eval(path, os.path.join(tmp, "copy.xml"), lo, hi, log=lambda *a: None)
        # the two baseline measures are sums of ones divided by their count: exactly 1.  The article measure sums the
        # block weights 1 / sum(w) * w_k (run_measure.py:224-232), two roundings per article, so 1 within the module's bound
        n_articles = len(measure.get_data_from_pagexml(path))
        assert all(t is not None for t in tuples) and all(float(v) == 1.0 for t in tuples[:2] for v in t), tuples
        assert n_articles >= 2 and all(abs(float(v) - 1.0) <= _bound(n_articles) for v in tuples[2]), tuples
    print("ok")


if __name__ == "__main__":
    {"hist_golden": check_hist_golden, "hist_fuzz": check_hist_fuzz, "golden": check_golden, "border": check_border,
     "determinism": check_determinism, "eval_class": check_eval_class, "cli": check_cli, "chain": check_chain}[sys.argv[1]](*sys.argv[2:])
