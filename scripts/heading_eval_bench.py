"""Heading evaluation on one MI355X.  Default: the grid kernel, us per 64,152-setting launch (one fixed height of the reference's grid) at
16 and 64 pages of 60 and 120 lines, (settings x lines) / s, its share of the fp64 VALU bound, and the same scoring by
the numpy restatement of the tests on the host (a thread pool of the CPUs a command may use) for the ratio.

The fp64 operations per (setting, line) decision are counted below from the kernel's source (heading_eval_kernels.h):
4 compares of the OR clauses (+1 add, +1 mul for (sw + th) / 2), and on the path where no clause holds 3 muls + 2 adds
and the final compare: at most 12 fp64 VALU operations, counted as 12 (the bound is then an upper bound on the rate).

With --grid: the whole grid (449,064 settings) on --pages synthetic 3000 x 4500 scans of --lines lines, split into its
stages (heading_evaluation_grid_search.run_grid timings), without and with the setting logs, and with --parent DIR one
setting of the parent commit's run_heading on the same pages (median of 3), times 449,064, against the grid.

Usage:  python scripts/heading_eval_bench.py --out profiles/heading_eval/gpu.json
        python scripts/heading_eval_bench.py --grid --lines 60 --parent PARENT_TREE --out profiles/heading_eval/grid_60.json
"""
import argparse
import json
import os
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from citlab_article_separation_new_amd import heading_evaluation as he  # noqa: E402

FP64_OPS_PER_DECISION = 12
# MI355X_MICROARCH.md: 256 CUs x 4 SIMD x 16 lanes x 2 (FMA) x 2.4 GHz = 78.6 TFLOP/s fp64 vector; counted as 39.3 T ops/s
# (one op per lane and clock, an FMA counted as one operation as the decisions' operations are separate)
FP64_VALU_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def synth_pages(rng, n_pages, n_lines):
    pages = []
    for _ in range(n_pages):
        sw = rng.integers(2, 14, n_lines) / 2.0
        th = rng.integers(15, 40, n_lines)
        net = rng.integers(0, 11, n_lines) / 10.0
        ids = [f"l{i}" for i in range(n_lines)]
        s, t, n, use = he.heading_confidences(({i: float(a) for i, a in zip(ids, sw)}, {i: int(a) for i, a in zip(ids, th)},
                                               {i: float(a) for i, a in zip(ids, net)}),
                                              [types.SimpleNamespace(id=i) for i in ids])
        cuts = np.sort(rng.integers(0, n_lines + 1, n_lines // 4))
        regions = [list(range(a, b)) for a, b in zip(np.r_[0, cuts], np.r_[cuts, n_lines])]
        pages.append((s, t, n, use, regions, (rng.random(len(regions)) < 0.3).tolist(), None))
    return pages


def cpu_counts(pages, tenths, workers=16):
    """the tests' restatement, vectorised over settings, one page per task"""
    t = np.asarray(tenths, np.int64) / 10

    def page(p):
        sw, th, net, use, regions, gt, _ = p
        n = np.where(np.asarray(tenths)[:, 1:2] == 0, 0.0, net[None, :])
        orc = (sw[None] >= t[:, 5:6]) | (th[None] >= t[:, 6:7]) | (((sw + th) / 2)[None] >= t[:, 7:8]) | (n >= t[:, 4:5])
        conf = np.where(orc, 1.0, t[:, 1:2] * n + t[:, 2:3] * sw[None] + t[:, 3:4] * th[None])
        head = conf > t[:, 0:1]
        out = np.zeros((len(tenths), 4), np.int64)
        for r, g in zip(regions, gt):
            hyp = (head[:, r].sum(axis=1) / len(r) >= t[:, 8]) if r else np.zeros(len(tenths), bool)
            out[:, 0] += hyp & g
            out[:, 1] += hyp & (not g)
            out[:, 2] += ~hyp & g
            out[:, 3] += ~hyp & (not g)
        return out
    with ThreadPoolExecutor(workers) as ex:
        return np.stack(list(ex.map(page, pages)), axis=1)


def write_scans(root, n_pages, n_lines, W=3000, H=4500):
    """n_pages synthetic 3000 x 4500 scans with a PAGE-XML each: n_lines text lines in regions of 2-6 lines over 4
    columns, a third of the regions headings in the GT (taller lines) -> (image list file, image paths)"""
    from PIL import Image
    from citlab_article_separation_new_amd import synth
    os.makedirs(os.path.join(root, "page"), exist_ok=True)
    rng = np.random.default_rng(11)
    paths = []
    for k in range(n_pages):
        img = os.path.join(root, f"scan{k:02d}.png")
        Image.fromarray(synth.synth_page(k, W=W, H=H)).save(img)
        regs, done, col, y = [], 0, 0, 80
        colw = (W - 200) // 4
        while done < n_lines:
            nl = min(int(rng.integers(2, 7)), n_lines - done)
            head = rng.random() < 0.33
            pitch = 70 if head else 40
            if y + nl * pitch > H - 80:
                col, y = col + 1, 80
            x0 = 60 + col * (colw + 20)
            ls = "".join(f'<TextLine id="r{len(regs)}l{i}"><Coords points="{x0},{y + i * pitch} {x0 + colw},{y + i * pitch} '
                         f'{x0 + colw},{y + (i + 1) * pitch - 6} {x0},{y + (i + 1) * pitch - 6}"/></TextLine>' for i in range(nl))
            regs.append(f'<TextRegion id="r{len(regs)}" type="{"heading" if head else "paragraph"}"><Coords points="{x0},{y} '
                        f'{x0 + colw},{y} {x0 + colw},{y + nl * pitch} {x0},{y + nl * pitch}"/>{ls}</TextRegion>')
            y += nl * pitch + 30
            done += nl
        with open(os.path.join(root, "page", f"scan{k:02d}.xml"), "w") as f:
            f.write('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/'
                    '2013-07-15"><Metadata><Creator>t</Creator><Created>2020-01-01T00:00:00</Created><LastChange>2020-01-01T00:00:00'
                    f'</LastChange></Metadata><Page imageFilename="scan{k:02d}.png" imageWidth="{W}" imageHeight="{H}">'
                    + "".join(regs) + '</Page></PcGts>')
        paths.append(img)
    lst = os.path.join(root, "images.lst")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return lst, paths


def write_pb(path):
    import tf_aru_graph
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    cfg = AruConfig()
    with open(path, "wb") as f:
        f.write(tf_aru_graph.build_aru_pb(init_aru_weights(cfg, 91, bias_jitter=0.05, logit_scale=0.05), cfg))


PARENT_RUN = """
import json, sys, time
sys.path.insert(0, sys.argv[1])
from citlab_article_separation_new_amd.run_net_post_processing import run_heading
paths = open(sys.argv[2]).read().split()
out = []
for _ in range(int(sys.argv[5])):
    t0 = time.perf_counter()
    run_heading(paths, sys.argv[3], 900, None, 0.4, None, None, 0.8, gpu_devices='0', host_workers=int(sys.argv[4]))
    out.append(time.perf_counter() - t0)
print(json.dumps(out))
"""


def grid_bench(args):
    """whole grid (7 fixed heights, 449,064 settings) on synthetic scans with the stage split, with and without the setting
    logs, and one setting of the parent commit's run_heading on the same pages (its package tree in --parent)"""
    import shutil
    import subprocess
    import tempfile
    from citlab_article_separation_new_amd import heading_evaluation_grid_search as gs
    root = tempfile.mkdtemp(prefix="heval_bench_")
    try:
        lst, paths = write_scans(root, args.pages, args.lines)
        pb = os.path.join(root, "heading.pb")
        write_pb(pb)
        res = {"pages": args.pages, "lines_per_page": args.lines, "host_workers": args.workers, "fixed_heights": list(he.FIXED_HEIGHTS),
               "no_logs": [], "with_logs": []}
        for kind, n, logs in (("no_logs", args.runs, False), ("with_logs", args.log_runs, True)):
            for _ in range(n):
                logdir = tempfile.mkdtemp(dir=root)
                tm = {}
                gs.run_grid(paths, pb, he.FIXED_HEIGHTS, logdir, os.path.join(logdir, "grid_results.csv"), setting_logs=logs,
                            host_workers=args.workers, timings=tm)
                tm["n_files"] = len(os.listdir(logdir))
                shutil.rmtree(logdir)
                print(kind, json.dumps(tm), flush=True)
                res[kind].append(tm)
        if args.parent:
            r = subprocess.run([sys.executable, "-c", PARENT_RUN, args.parent, lst, pb, str(args.workers), "3"], capture_output=True,
                               text=True, check=True)
            runs = json.loads(r.stdout.strip().splitlines()[-1])
            res["parent_run_heading_s"] = runs
            med = float(np.median(runs))
            grid = float(np.median([t["total_s"] for t in res["no_logs"]]))
            res["parent_one_setting_median_s"] = med
            res["parent_times_449064_s"] = med * 449064
            res["grid_no_logs_median_s"] = grid
            res["ratio"] = med * 449064 / grid
            res["meets_100x"] = bool(res["ratio"] >= 100)
            print("parent", json.dumps(runs), "ratio", res["ratio"], flush=True)
            if not res["meets_100x"]:
                raise SystemExit(f"the grid is only {res['ratio']:.1f}x below 449,064 settings of the parent's run_heading (>= 100x required)")
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", action="store_true", help="the whole grid on synthetic scans instead of the kernel points")
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--lines", type=int, default=60)
    ap.add_argument("--workers", type=int, default=8, help="host decode workers of the grid and of the parent's run_heading")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--log_runs", type=int, default=1)
    ap.add_argument("--parent", default=None, help="package tree of the parent commit (built), for the comparison")
    args = ap.parse_args()
    if args.grid:
        res = grid_bench(args)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    _, tenths = he.grid_settings((600,))
    rng = np.random.default_rng(0)
    res = {"settings_per_launch": int(len(tenths)), "fp64_ops_per_decision": FP64_OPS_PER_DECISION, "points": []}
    for n_pages in (16, 64):
        for n_lines in (60, 120):
            pages = synth_pages(rng, n_pages, n_lines)
            gp = he.GridPages(pages)
            he.grid_eval(gp, tenths)                                     # warm-up
            us, wall = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                counts = he.grid_eval(gp, tenths)
                wall.append(time.perf_counter() - t0)
                us.append(he.last_kernel_us())
            cpu = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                ref = cpu_counts(pages, tenths)
                cpu.append(time.perf_counter() - t0)
            cpu_s = float(np.median(cpu))
            assert np.array_equal(counts, ref), "kernel and restatement differ"
            dec = len(tenths) * n_pages * n_lines
            med = float(np.median(us))
            pt = {"pages": n_pages, "lines_per_page": n_lines, "kernel_us": us, "kernel_us_median": med,
                  "call_wall_s": wall, "decisions_per_s": dec / (med * 1e-6),
                  "fp64_valu_share": dec * FP64_OPS_PER_DECISION / (med * 1e-6) / FP64_VALU_OPS_PER_S,
                  "cpu_restatement_s": cpu, "cpu_restatement_s_median": cpu_s,
                  "cpu_over_kernel_call": cpu_s / float(np.median(wall)),
                  "cpu_over_kernel_call_per_run": [c / w for c, w in zip(cpu, wall)]}
            print(json.dumps(pt))
            res["points"].append(pt)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
