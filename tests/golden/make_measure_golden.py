"""Generates measure_golden.json from the REFERENCE's article_separation_measure package (use_java_code=False):
eval_measure.py, baseline_measure.py and run_measure.py on the seeded pairs of measure_cases.py, in both tolerance
modes, plus the complete stdout of run_measure for a few file lists.  Also writes the reference's wall time per case to
profiles/measure/reference_cpu.json.

Run in the build container only (ref_import stubs what the reference imports at module level; np.float is aliased for
this process; get_data_from_pagexml is replaced by a lookup of the case's dictionaries; no JVM exists or is started).

    python tests/golden/make_measure_golden.py

Asserted here, so that no test leaves anything out: in every greedy step of every recorded alignment the chosen entry
differs from every other remaining entry of its row and column by at least 1e-9, or is bit-equal to it with identical
point sets or a value of exactly 0 or 1; no printed value lies within 1e-9 of a rounding boundary of its six decimals.
"""
import contextlib
import io
import json
import os
import platform
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

ref_import.install_stubs()

import numpy as np  # noqa: E402

if not hasattr(np, "float"):
    np.float = float

from python_util.geometry.polygon import Polygon, norm_poly_dists  # noqa: E402
from article_separation_measure import eval_measure as em  # noqa: E402
from article_separation_measure import run_measure as rm  # noqa: E402

import measure_cases as mc  # noqa: E402

Eval = em.BaselineMeasureEval
Eval.calc_measure_for_page_baseline_polys.__defaults__ = (False,)

LOG = {"jobs": None, "weighted": None}


def _poly(q):
    return Polygon(list(q[0]), list(q[1]), len(q[0]))


def _ref_dict(side):
    return {k: [_poly(q) for q in polys] for k, polys in side}


# ---- recording wrappers around the reference's functions ----------------------------------------------------------------

_calc_tols, _count, _calc, _greedy = em.calc_tols, Eval.count_rel_hits, Eval.calc_measure_for_page_baseline_polys, rm.get_greedy_sum


def calc_tols(polys, *a, **k):
    out = _calc_tols(polys, *a, **k)
    LOG["tols"] = [float(v) for v in out]
    return out


def count_rel_hits(self, poly_to_count, poly_ref, tols):
    out = _count(self, poly_to_count, poly_ref, tols)
    LOG["hits"].append(np.array(out))
    LOG["pts"].setdefault(id(poly_to_count), (tuple(poly_to_count.x_points), tuple(poly_to_count.y_points)))
    LOG["pts"].setdefault(id(poly_ref), (tuple(poly_ref.x_points), tuple(poly_ref.y_points)))
    LOG["ids"].append((id(poly_to_count), id(poly_ref)))
    return out


def check_greedy(matrix, same=None, what=""):
    """the tie condition of the module docstring on one dense matrix (own simulation of the argmax loop)"""
    m = np.array(matrix, float)
    while True:
        r, c = np.unravel_index(np.argmax(m), m.shape)
        v = m[r, c]
        if v < 0:
            return
        for rr, cc in [(r, k) for k in range(m.shape[1]) if k != c] + [(k, c) for k in range(m.shape[0]) if k != r]:
            o = m[rr, cc]
            if o < 0 or abs(o - v) >= 1e-9:
                continue
            assert o == v and (v in (0.0, 1.0) or (same is not None and same((r, c), (rr, cc)))), \
                f"{what}: near tie {v!r} / {o!r} at {(r, c)} / {(rr, cc)}: choose another seed"
        m[r, :] = -1.0
        m[:, c] = -1.0


def calc_measure(self, polys_truth, polys_reco, use_java_code=False):
    LOG.update(tols=None, hits=[], pts={}, ids=[])
    _calc(self, polys_truth, polys_reco, False)
    res = self.measure.result
    n_t, n_r = len(polys_truth), len(polys_reco)
    hits = np.array(LOG["hits"]).reshape(n_r, n_t, -1)
    ids = LOG["ids"]

    def same(e1, e2):
        a, b = ids[e1[0] * n_t + e1[1]], ids[e2[0] * n_t + e2[1]]
        return LOG["pts"][a[0]] == LOG["pts"][b[0]] and LOG["pts"][a[1]] == LOG["pts"][b[1]]
    for t in range(hits.shape[2]):
        check_greedy(hits[:, :, t], same, "precision alignment")
    LOG["jobs"].append({"n_truth": n_t, "n_reco": n_r, "tols": LOG["tols"],
                        "precision": res.page_wise_per_dist_tol_tick_per_line_precision[-1].tolist(),
                        "recall": res.page_wise_per_dist_tol_tick_per_line_recall[-1].tolist(),
                        "P": float(res.page_wise_precision[-1]), "R": float(res.page_wise_recall[-1])})


def get_greedy_sum(array):
    check_greedy(array, None, "greedy sum")
    LOG["weighted"].append(np.array(array).tolist())
    return _greedy(array)


em.calc_tols = calc_tols
Eval.count_rel_hits = count_rel_hits
Eval.calc_measure_for_page_baseline_polys = calc_measure
rm.get_greedy_sum = get_greedy_sum

DICTS = {}
rm.get_data_from_pagexml = lambda path_to_pagexml: dict(DICTS[path_to_pagexml])


def assert_rounding(values, what):
    for v in values:
        if v is None:
            continue
        frac = abs(v) * 1e6 % 1.0
        assert abs(frac - 0.5) >= 1e-3, f"{what}: {v!r} is too close to a rounding boundary of its six decimals"


def _tuples(t):
    return [None if x is None else [float(v) for v in x] for x in t]


def main():
    cases, timing = [], []
    for k in range(len(mc.golden_cases())):
        for shift in range(50):
            try:
                one_case(*mc.golden_cases(shift)[k], shift, cases, timing)
                break
            except AssertionError as e:
                print("   shift", shift, "rejected:", e, flush=True)
        else:
            raise SystemExit("no seed without near ties")
    write(cases, timing)


def one_case(name, gt, hy, modes, with_normed, shift, cases, timing):
    timing_case = []
    rec = {"name": name, "seed_shift": shift, "gt": gt, "hy": hy, "modes": {}}
    if with_normed:
        for key, side in (("normed_truth", gt), ("normed_reco", hy)):
            n = norm_poly_dists([_poly(q) for _, polys in side for q in polys], 5)
            rec[key] = [[list(map(int, p.x_points)), list(map(int, p.y_points))] for p in n]
    DICTS["gt/%s.xml" % name], DICTS["hy/%s.xml" % name] = _ref_dict(gt), _ref_dict(hy)
    for mode in modes:
        min_tol, max_tol = mc.MODES[mode]
        LOG.update(jobs=[], weighted=[])
        buf = io.StringIO()
        t0 = time.time()
        with contextlib.redirect_stdout(buf):
            tup = rm.run_eval("gt/%s.xml" % name, "hy/%s.xml" % name, min_tol, max_tol, 0.25, 5)
        dt = time.time() - t0
        jobs = LOG["jobs"]
        n_hy = sum(k is not None for k, _ in hy)
        for n, j in enumerate(jobs[2:]):            # the article pairs: page values only (they are the r / p matrices),
            del j["precision"], j["recall"]         # the GT article's tolerances once per row
            if n % n_hy:
                del j["tols"]
        rec["modes"][mode] = {"min_tol": min_tol, "max_tol": max_tol, "tuples": _tuples(tup), "jobs": jobs,
                              "weighted": LOG["weighted"], "stdout": buf.getvalue()}
        for x in tup:
            assert_rounding(x or (), name)
        n_lines = sum(len(v) for _, v in gt)
        timing_case.append({"case": name, "mode": mode, "gt_baselines": n_lines, "hy_baselines": sum(len(v) for _, v in hy),
                       "seconds": round(dt, 3)})
        print(f"{name:24s} {mode:9s} {dt:7.2f} s  {tup}", flush=True)
    if name not in mc.TIMED_ONLY:
        cases.append(rec)
    timing.extend(timing_case)


def write(cases, timing):
    lists = {}
    LOG.update(jobs=[], weighted=[])
    by_name = {c["name"]: c for c in cases}
    for lname, (names, runs) in mc.FILE_LISTS.items():
        for mode, verbose in runs:
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rm.run_measure(["gt/%s.xml" % n for n in names], ["hy/%s.xml" % n for n in names], *mc.MODES[mode], 0.25, 5, verbose)
            lists[f"{lname}/{mode}/{'verbose' if verbose else 'quiet'}"] = {"names": names, "mode": mode, "verbose": verbose,
                                                                         "stdout": buf.getvalue()}
            for k in range(3):                          # the printed averages, in run_measure's arithmetic
                tups = [t for t in (by_name[n]["modes"][mode]["tuples"][k] for n in names) if t is not None]
                total = [0, 0, 0]
                for t in tups:
                    total = [total[i] + t[i] for i in range(3)]
                assert_rounding([1 / len(tups) * v for v in total] if tups else [], f"{lname}/{mode} averages")
    out = os.path.join(HERE, "measure_golden.json")
    json.dump({"source": "article_separation_measure (use_java_code=False), rel_tol 0.25, poly_tick_dist 5", "cases": cases,
               "file_lists": lists}, open(out, "w"), separators=(",", ":"))
    print("wrote", out, os.path.getsize(out), "bytes")
    prof = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "measure")
    os.makedirs(prof, exist_ok=True)
    json.dump({"what": "wall time of the reference's run_eval, Python path (use_java_code=False), one file pair, one process",
               "machine": f"{platform.processor() or platform.machine()}, {os.cpu_count()} CPUs, python {platform.python_version()}, "
                          f"numpy {np.__version__}", "runs": timing}, open(os.path.join(prof, "reference_cpu.json"), "w"))


if __name__ == "__main__":
    main()
