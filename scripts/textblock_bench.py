"""Text block detection timings on synthetic baseline-only pages of about 360 and about 1,500 lines.

    python scripts/textblock_bench.py [--out profiles/textblock/gpu.json] [--pages 8] [--reference]

Reports per page size: the device time of each kernel per page (asep_textblock_last_kernel_us, median of repeats), the
host time of each stage, and the pages/s of both command lines (files read and rewritten in place, in-process).
With --reference and the reference checkout present (/root/reference, never on a GPU machine) it only times the
reference's Python path (use_java_code=False) on the same pages: get_list_of_interline_distances and the whole
DBSCANBaselines.  With --work-model it counts, on the host, the work per wave of the distance kernel.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import textblock_cases as tc  # noqa: E402

REFERENCE = "/root/reference"


def bench_pages():
    return {
        "lines360": tc.columns_page(101, n_cols=6, n_lines=60, col_w=440, gap=40, pitch=64, extras=False, heading=False),
        "lines1500": tc.columns_page(102, n_cols=10, n_lines=150, col_w=260, gap=30, pitch=27, extras=False,
                                     heading=False),
    }


def _write_page(path, page, W=3000, H=4500):
    ns = "http://schema.primaresearch.org/PAGE/gts/pagecontent/2013-07-15"
    lines = "".join('<TextLine id="tl_%d"><Baseline points="%s"/></TextLine>'
                    % (i, " ".join("%d,%d" % (x, y) for x, y in zip(xs, ys))) for i, (xs, ys) in enumerate(page))
    with open(path, "w") as f:
        f.write('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="%s"><Metadata><Creator>htr</Creator></Metadata>'
                '<Page imageFilename="p.png" imageWidth="%d" imageHeight="%d"><TextRegion id="r0">'
                '<Coords points="0,0 %d,0 %d,%d 0,%d"/>%s</TextRegion></Page></PcGts>'
                % (ns, W, H, W - 1, W - 1, H - 1, H - 1, lines))


def _t(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return r, time.perf_counter() - t0


def gpu_bench(page, n_pages, reps=5):
    from citlab_article_separation_new_amd import textblock, textblock_geometry as geo
    from citlab_article_separation_new_amd import run_baseline_clustering as rbc, run_textregion_generation as rtg
    res = {"baselines": len(page)}
    first, t_norm = _t(textblock.normed_pages, [page], 5)
    res["host_norm_angles_s"] = t_norm
    textblock.interline_distances(first, 5, 500)                      # warm-up (module load, buffers)
    k_us, calls = [], []
    for _ in range(reps):
        d, t = _t(textblock.interline_distances, first, 5, 500)
        k_us.append(textblock.last_kernel_us(0))
        calls.append(t)
    res["interline_kernel_us"] = statistics.median(k_us)
    res["interline_call_s"] = statistics.median(calls)
    prep = textblock.dbscan_prepare([page], 5, 500, 50)[0]
    n_us, calls = [], []
    for _ in range(reps):
        nb, t = _t(textblock.neighbour_lists, [prep["normed"]], [prep["dists"]], [prep["avg"]], 1.25)
        n_us.append(textblock.last_kernel_us(1))
        calls.append(t)
    res["neighbour_kernel_us"] = statistics.median(n_us)
    res["neighbour_call_s"] = statistics.median(calls)
    labels, t = _t(textblock.dbscan_labels, nb[0], 2)
    res["host_dbscan_s"] = t
    res["host_whole_dbscan_s"] = _t(textblock.cluster_baselines, [page])[1]
    lab, _ = textblock.cluster_of_polygons(labels, 1)
    art = {}
    for i, l in enumerate(lab):
        art.setdefault("a%d" % l, []).append("l%d" % i)
    n50 = geo.norm_poly_dists(page, 50)
    d_tr = textblock.interline_distances(textblock.normed_pages([page], 5), 5, 100)[0]
    geom = {"l%d" % i: (p, v) for i, (p, v) in enumerate(zip(n50, d_tr.tolist()))}
    regions, t = _t(textblock.create_text_regions, art, geom, 75, lambda s: None)
    res["host_alpha_regions_s"] = t
    res["regions"] = len(regions)
    # both command lines, in-process: files in, files rewritten in place
    tmp = tempfile.mkdtemp(prefix="tb_bench_")
    try:
        paths = [os.path.join(tmp, "p%03d.xml" % k) for k in range(n_pages)]
        for p in paths:
            _write_page(p, page)
        fb = rbc.build_parser().parse_args(["--num_threads", "16"])
        _, t = _t(rbc.process, paths, fb, 0, lambda s: None)
        res["baseline_clustering_pages_per_s"] = n_pages / t
        ft = rtg.build_parser().parse_args(["--num_threads", "16"])
        _, t = _t(rtg.process, paths, ft, 0, lambda s: None)
        res["textregion_generation_pages_per_s"] = n_pages / t
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def work_model(page):
    """Host replay of tb_interline_kernel's scan on one page (no GPU): per wave (baseline) the rounds Pa*Nb/64 and the
    pairs whose point loop runs, with the points those loops visit.  A lane runs its pair's loop alone, so a wave's
    dependent chain is at most the points of all its surviving pairs (pairs in one round overlap)."""
    import math
    import numpy as np
    from citlab_article_separation_new_amd import textblock
    pg = textblock.normed_pages([page], 5)[0]
    bx, by, bw, bh = (pg.boxes[:, k].astype(np.int64) for k in range(4))
    rounds, loops, iters = [], [], []
    for a, (xa, ya) in enumerate(pg.polys):
        ox, oy = pg.orient[a]
        dist, nl, ni = 500.0, 0, 0
        ends_a = ((xa[0], ya[0]), (xa[-1], ya[-1]))
        for px, py in zip(xa.tolist(), ya.tolist()):
            bd = (np.where(px < bx, bx - px, 0) + np.where(px > bx + bw, px - bx - bw, 0)
                  + np.where(py < by, by - py, 0) + np.where(py > by + bh, py - by - bh, 0))
            for b in np.flatnonzero(bd <= dist):
                if b == a or bd[b] > dist:
                    continue
                xb, yb = pg.polys[b]
                ins = [(p[0] - q[0]) * ox + (-p[1] + q[1]) * oy for p in ends_a for q in ((xb[0], yb[0]), (xb[-1], yb[-1]))]
                if all(v < 0 for v in ins) or all(v > 0 for v in ins):
                    continue
                nl, ni = nl + 1, ni + len(xb)
                dx, dy = px - xb, -py + yb
                ok = np.abs(dx * ox + dy * oy) <= 10
                if ok.any():
                    dist = min(dist, float(np.abs(dx * oy - dy * ox)[ok].min()))
        rounds.append(math.ceil(len(xa) * pg.n / 64))
        loops.append(nl)
        iters.append(ni)
    return dict(baselines=pg.n, mean_points=float(np.mean([len(x) for x, _ in pg.polys])), rounds_mean=float(np.mean(rounds)),
                rounds_max=int(max(rounds)), loop_pairs_mean=float(np.mean(loops)), chain_points_mean=float(np.mean(iters)),
                chain_points_max=int(max(iters)), points_total=int(sum(iters)))


def reference_bench(page, whole=True):
    import contextlib
    import io
    import ref_import
    ref_import.install_stubs()
    from python_util.geometry.polygon import Polygon
    from article_separation.baseline_clustering import dbscan_baselines as db
    polys = lambda: [Polygon(list(xs), list(ys), len(xs)) for xs, ys in page]   # noqa: E731
    res = {}
    with contextlib.redirect_stdout(io.StringIO()):
        _, res["ref_interline_distances_s"] = _t(db.get_list_of_interline_distances, polys(), 5, 500, False)
        if whole:
            _, res["ref_dbscan_baselines_s"] = _t(db.DBSCANBaselines, polys(), use_java_code=False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pages", type=int, default=8, help="files per command line run")
    ap.add_argument("--reference", action="store_true", help="time the reference's Python path instead (CPU only)")
    ap.add_argument("--work-model", action="store_true", help="count the distance kernel's work per wave on the host instead")
    ap.add_argument("--sizes", default="lines360,lines1500")
    a = ap.parse_args()
    pages = bench_pages()
    out = {"pages": {}}
    for name in a.sizes.split(","):
        page = pages[name]
        if a.work_model:
            out["pages"][name] = work_model(page)
        elif a.reference:
            if not os.path.isdir(REFERENCE):
                print("reference checkout not present: skipped")
                return 0
            out["pages"][name] = dict(baselines=len(page), **reference_bench(page))
        else:
            out["pages"][name] = gpu_bench(page, a.pages)
        print(name, json.dumps(out["pages"][name]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
