"""Relation net evaluation on one MI355X: the device scorer (asep_releval_finish) against sklearn on the same arrays.

Per size (1 M, 4 M, 16 M, 40 M pairs): the device time of every kernel of finish (device events, warmed, the median of
--repeats runs), the achieved bytes/s of the four sort passes against their algorithmic bytes (``sort_bytes``: the form that
was built reads the keys once for the digit histograms of a pass and once more for its scatter, which writes them: 12 B per
pair and pass, 48 B per pair; a single histogram pre-pass for all four digits would make it 36 B per pair) and against the
8 TB/s of HBM, and the wall time of the whole finish (sort, curve, fetch of the thresholds / tps / fps arrays, the host's
float64 divisions).  In the same call and alternating with it: precision_recall_curve, roc_auc_score and accuracy_score of
the installed sklearn on the same arrays, on the CPUs this command may use -- the reference's way.

With --evaluate PAGES: LavGNN.evaluate() on a list of PAGES synthetic 200-node pages (the geometric net): wall time and
the shares of net, appends and finish.

Usage:  python scripts/relation_eval_bench.py --out profiles/relation_eval/gpu.json
"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
PASSES, KEY_BYTES = 4, 4


def sort_bytes(n_pairs, histogram_per_pass=True):
    """algorithmic bytes of the radix sort of n_pairs 32-bit keys: per pass the scatter reads and writes every key; the
    digit histograms read them once per pass (the form that was built) or once for all passes"""
    scatter = PASSES * 2 * KEY_BYTES * n_pairs
    hist = (PASSES if histogram_per_pass else 1) * KEY_BYTES * n_pairs
    return scatter + hist


def make(n, seed=0):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.05).astype(np.int32)
    p = rng.random(n, dtype=np.float32)
    return np.where(y == 1, np.sqrt(p), p * p).astype(np.float32), y


def med(xs):
    return float(np.median(xs))


def bench_size(n, repeats, with_sklearn):
    import sklearn.metrics as sk
    from citlab_article_separation_new_amd.lav_rel import RelationEval
    p, y = make(n, n % 97)
    acc = RelationEval(0)
    acc.reserve(n)
    stages, finish_s, sk_s = [], [], {"precision_recall_curve": [], "roc_auc_score": [], "accuracy_score": []}
    curve = None
    for it in range(repeats + 1):                                     # the first run warms up (allocations, code objects)
        acc.reset()
        acc.append(p, y)
        t0 = time.perf_counter()
        curve = acc.finish()
        prec, rec, thr = curve.precision_recall_curve()
        auc, accuracy = curve.auc_roc, curve.accuracy
        dt = time.perf_counter() - t0
        if it:
            finish_s.append(dt)
            stages.append(acc.stage_us())
        if with_sklearn and it < max(1, min(repeats, 2)):            # alternating with the device runs
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for name, fn in (("precision_recall_curve", lambda: sk.precision_recall_curve(y, p)),
                                 ("roc_auc_score", lambda: sk.roc_auc_score(y, p)),
                                 ("accuracy_score", lambda: sk.accuracy_score(y, p > 0.5))):
                    t0 = time.perf_counter()
                    out = fn()
                    sk_s[name].append(time.perf_counter() - t0)
                    if name == "precision_recall_curve":
                        assert out[0].tobytes() == prec.tobytes() and out[2].tobytes() == thr.tobytes()
                    elif name == "accuracy_score":
                        assert out == accuracy
                    else:
                        assert abs(out - auc) <= 1e-12
    acc.close()
    us = {k: med([s[k] for s in stages]) for k in stages[0]}
    sort_us = sum(v for k, v in us.items() if k.startswith("pass"))
    curve_us = sum(v for k, v in us.items() if not k.startswith("pass"))
    res = {"pairs": n, "thresholds": int(len(curve.thresholds)), "kernel_us": us, "sort_kernels_us": sort_us, "curve_kernels_us": curve_us,
           "sort_bytes_built_48": sort_bytes(n), "sort_bytes_prepass_36": sort_bytes(n, False),
           "sort_bytes_per_s": sort_bytes(n) / (sort_us * 1e-6), "sort_share_of_hbm": sort_bytes(n) / (sort_us * 1e-6) / HBM_BYTES_PER_S,
           "finish_wall_s": med(finish_s), "repeats": repeats}
    per_pass = {}
    for k in ("hist", "scatter"):
        t = sum(us[f"pass{q}_{k}"] for q in range(PASSES)) * 1e-6
        per_pass[k + "_bytes_per_s"] = PASSES * (1 if k == "hist" else 2) * KEY_BYTES * n / t
    res.update(per_pass)
    if with_sklearn:
        res["sklearn_s"] = {k: med(v) for k, v in sk_s.items()}
        res["sklearn_total_s"] = sum(res["sklearn_s"].values())
        res["sklearn_over_finish"] = res["sklearn_total_s"] / res["finish_wall_s"]
    return res


def bench_evaluate(n_pages):
    import torch
    from citlab_article_separation_new_amd import lav_rel, synth
    with tempfile.TemporaryDirectory() as tmp:
        argv = synth.write_gnn_cli_inputs(tmp, n_pages, visual=False, N=200)
        rng = np.random.default_rng(1)
        for k in range(min(4, n_pages)):                              # ground truth: random articles (the weights are random too)
            path = os.path.join(tmp, "data", "json15d2bb", f"p{k:03d}.json")
            d = json.load(open(path))
            member = rng.integers(0, 8, 200)
            i, j = np.nonzero((member[:, None] == member[None, :]) & ~np.eye(200, dtype=bool))
            d["gt_relations"] = np.stack([np.zeros_like(i), i, j], 1).tolist()
            d["gt_num_relations"] = len(i)
            json.dump(d, open(path, "w"))
        out = {}
        for workers in (1, 8):
            lav = lav_rel.LavGNN(argv=argv + ["--gpu_devices", "0", "--num_workers", str(workers)])
            t0 = time.perf_counter()
            curve = lav.evaluate()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            tm = dict(lav.timings)
            tm.pop("stage_us", None)
            out[f"workers_{workers}"] = {"pages": n_pages, "pairs": curve.n, "wall_s": wall, **tm,
                                         "share_prepare_wait": tm["prepare_wait_s"] / wall, "share_net_enqueue": tm["net_s"] / wall,
                                         "share_appends": tm["append_s"] / wall, "share_finish": tm["finish_s"] / wall}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 4_000_000, 16_000_000, 40_000_000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no_sklearn", action="store_true")
    ap.add_argument("--evaluate", type=int, default=100, help="pages of the evaluate() run (0: skip)")
    a = ap.parse_args()
    import sklearn
    res = {"sklearn": sklearn.__version__, "cpus": int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0)),
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "sizes": []}
    for n in a.sizes:
        r = bench_size(n, a.repeats, not a.no_sklearn)
        print(json.dumps(r), flush=True)
        res["sizes"].append(r)
    if a.evaluate:
        res["evaluate"] = bench_evaluate(a.evaluate)
        print(json.dumps(res["evaluate"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
