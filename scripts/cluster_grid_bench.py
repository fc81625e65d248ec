"""Times the clustering grid (ClusterGrid: one device call for every (page, setting)) against the host class looping over the
same problems in a pool of worker processes, on synthetic `blocks` matrices (tests/golden/clustering_cases.make_confs).

    python scripts/cluster_grid_bench.py --out profiles/cluster_grid/gpu.json [--pages 24] [--grid 11] [--workers 16]
        [--methods dbscan,dbscan_std,greedy]

With ``--methods`` every method named is timed on its own grid (dbscan: the thresholds; dbscan_std: epsilon x min_samples 1..4 of
the same size; greedy: max_iteration 1000 and 5) under the key of its name, and the host class runs ``calc``'s method function.

Records the device time of the kernels (events around them), the wall time of the whole call (uploads, launch, labels and counts
back), and the wall time of the host loop; checks that both give the same labels.  Needs a GPU."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


class _Flags:
    def __init__(self, params):
        self.clustering_params = {k: v for k, v in params.items() if k != "clustering_method"}


def _host_page(args):
    """all settings of one page through the host class -> list of label lists"""
    from citlab_article_separation_new_amd.clustering import TextblockClustering
    confs, settings = args
    out = []
    for params in settings:
        tb = TextblockClustering(_Flags(params))       # (a fresh object per setting: the class keeps its scanner)
        tb.set_confs(confs, symmetry_fn=None)
        getattr(tb, "_" + params.get("clustering_method", "dbscan"))()
        out.append([int(v) for v in tb.tb_labels])
    return out


def method_settings(method, grid):
    thr = [round(0.2 + 0.6 * i / max(1, grid - 1), 10) for i in range(grid)]
    if method == "dbscan":
        return [{"confidence_threshold": c, "cluster_agreement_threshold": a} for c in thr for a in thr]
    if method == "dbscan_std":
        eps = [round(0.1 + 1.4 * i / max(1, grid - 1), 10) for i in range(grid)]
        return [{"clustering_method": method, "epsilon": e, "min_samples": k} for e in eps for k in (1, 2, 3, 4)]
    if method == "greedy":
        return [{"clustering_method": method, "max_iteration": it} for it in (1000, 5)]
    raise SystemExit(f"--methods: '{method}' is not dbscan, dbscan_std or greedy")


def measure(grid, mats, settings, workers, repeats):
    """the device call against the host class on the same problems -> result dict"""
    grid.run_array(settings)                                   # warm-up: code object load, buffer pool
    wall, kern = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        node_off, labels = grid.run_array(settings)
        wall.append(time.perf_counter() - t0)
        kern.append(grid.kernel_us)

    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(workers) as pool:
        t1 = time.perf_counter()
        host = pool.map(_host_page, [(m, settings) for m in mats], chunksize=1)
        host_s = time.perf_counter() - t1
    host_with_pool_s = time.perf_counter() - t0
    same = all(labels[s, node_off[k]:node_off[k + 1]].tolist() == host[k][s] for k in range(len(mats)) for s in range(len(settings)))
    return {"settings": len(settings), "problems": len(mats) * len(settings),
            "device_kernel_us_median": float(np.median(kern)), "device_kernel_us_all": kern,
            "device_call_wall_s_median": float(np.median(wall)), "device_call_wall_s_all": wall,
            "host_workers": workers, "host_loop_wall_s": host_s, "host_loop_with_pool_start_s": host_with_pool_s,
            "labels_identical": bool(same)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--pages", type=int, default=24)
    ap.add_argument("--grid", type=int, default=11, help="thresholds per axis")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--methods", default=None, help="comma list of dbscan, dbscan_std, greedy: one result per method")
    args = ap.parse_args(argv)
    import clustering_cases as cc
    from citlab_article_separation_new_amd.clustering.cluster_grid import ClusterGrid

    sizes = [40 + (37 * k) % 120 for k in range(args.pages)]
    mats = [cc.make_confs("blocks", n, 9000 + k, args.dtype) for k, n in enumerate(sizes)]
    mats = [((m + m.T) / 2).astype(args.dtype) for m in mats]

    grid = ClusterGrid(0)
    for m in mats:
        grid.add_page(m, symmetry_fn=None)
    result = {"pages": len(mats), "nodes_per_page": sizes, "dtype": args.dtype}
    if args.methods is None:
        result.update(measure(grid, mats, method_settings("dbscan", args.grid), args.workers, args.repeats))
        same = result["labels_identical"]
    else:
        for method in [m.strip() for m in args.methods.split(",") if m.strip()]:
            result[method] = measure(grid, mats, method_settings(method, args.grid), args.workers, args.repeats)
        same = all(v["labels_identical"] for v in result.values() if isinstance(v, dict))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
