"""Article separation measure timings on synthetic file pairs of about 200, 360 and 1,500 baselines.

    python scripts/measure_bench.py [--out profiles/measure/gpu.json] [--reps 5]

Reports per size and tolerance mode (dynamic / fixed 10..30), for one file pair per call: the device time of the three
kernels (asep_measure_last_kernel_us, median of repeats), the wall time of the whole evaluation after the files have
been read (norming, tolerances, device call, alignments, weighting), the candidate polygon pairs and records, the point
pairs evaluated by the pair kernel and by the recall kernel, and the integer point-pair rate of the two kernels.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import measure_cases as mc  # noqa: E402

SIZES = {"lines200": (5, 40), "lines360": (6, 60), "lines1500": (10, 150)}
MODES = {"dynamic": (-1, -1), "fixed_10_30": (10, 30)}


def point_pairs(prep, res):
    import numpy as np
    t_n = np.array([len(xs) for xs, _ in prep.truth.polys])
    r_n = np.array([len(xs) for xs, _ in prep.reco.polys])
    pair = int((r_n[res.pair_i] * t_n[res.pair_j]).sum())
    return pair, pair                    # the recall kernel walks the same candidate pairs from the truth side


def bench(gt, hy, tol, reps):
    from citlab_article_separation_new_amd import measure
    pair = (mc.as_dict(gt), mc.as_dict(hy))
    quiet = (lambda *a: None)
    measure.evaluate(*measure.run_eval_dicts([pair], *tol, 0.25, 5)[0], log=quiet)          # warm-up
    wall, dev, kern = [], [], [[], [], []]
    for _ in range(reps):
        t0 = time.perf_counter()
        preps = measure.prepare([pair], *tol, 0.25, 5)
        t1 = time.perf_counter()
        res = measure.device_rel_hits(preps)
        t2 = time.perf_counter()
        for k in range(3):
            kern[k].append(measure.last_kernel_us(k))
        tuples = measure.evaluate(preps[0], res[0], log=quiet)
        t3 = time.perf_counter()
        wall.append(t3 - t0)
        dev.append((t1 - t0, t2 - t1, t3 - t2))
    prep, r = preps[0], res[0]
    pp_pair, pp_recall = point_pairs(prep, r)
    med = [statistics.median(k) for k in kern]
    return {"gt_baselines": prep.truth.n, "hy_baselines": prep.reco.n, "n_tols": int(prep.tols.shape[1]), "dmax": r.dmax,
            "candidate_pairs": len(r.pair_i), "candidate_records": len(r.rec_j), "dense_pairs": prep.truth.n * prep.reco.n,
            "point_pairs_pair_kernel": pp_pair, "point_pairs_recall_kernel": pp_recall,
            "kernel_us": {"count": med[0], "pair": med[1], "recall": med[2]},
            "point_pairs_per_s": {"pair": pp_pair / (med[1] * 1e-6) if med[1] else None,
                                  "recall": pp_recall / (med[2] * 1e-6) if med[2] else None},
            "wall_s_per_file_pair": statistics.median(wall),
            "wall_split_s": {"prepare_and_tolerances": statistics.median(d[0] for d in dev),
                             "device_call": statistics.median(d[1] for d in dev),
                             "alignments_and_tuples": statistics.median(d[2] for d in dev)},
            "tuples": [None if t is None else [float(v) for v in t] for t in tuples]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure", "gpu.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    out = {"what": "run_eval per file pair on one MI355X, files already read; kernel times from hipEvents", "runs": {}}
    for name, (n_cols, n_lines) in SIZES.items():
        gt, hy = mc.bench_pair(n_cols, n_lines)
        for mode, tol in MODES.items():
            out["runs"][f"{name}/{mode}"] = r = bench(gt, hy, tol, args.reps)
            print(name, mode, json.dumps({k: r[k] for k in ("candidate_pairs", "kernel_us", "wall_s_per_file_pair")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
