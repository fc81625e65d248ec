"""Alpha-shape text regions: host function against the device engine on the 360- and 1,500-line pages of textblock_bench.py.

    python scripts/alpha_shape_bench.py [--out profiles/alpha_shape/gpu.json] [--pages 4] [--reps 5]

Per page, as medians of ``--reps`` runs after one warm-up: the host triangulation of all its articles, the two kernels (hipEvent
times of asep_alpha_shapes_last_kernel_us), the engine call with its copies, the host function on the same articles, and
run_textregion_generation's pages/s over ``--pages`` files with and without --device_regions True (alternating, in-process,
files restored before each run).  Third column: the triangulation on the device too
(asep_alpha_shapes_points, --device_triangulation True): its kernel, its engine call against host triangulation +
asep_alpha_shapes on the same articles, its regions, its pages/s.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import textblock_bench as tbb  # noqa: E402


def _median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def page_bench(page, n_pages, reps):
    from citlab_article_separation_new_amd import textblock, textblock_geometry as geo
    from citlab_article_separation_new_amd import run_baseline_clustering as rbc, run_textregion_generation as rtg
    labels, _ = textblock.cluster_baselines([page])[0]
    art = {}
    for i, lab in enumerate(labels):
        art.setdefault("a%d" % lab, []).append("l%d" % i)
    n50 = geo.norm_poly_dists(page, 50)
    d_tr = textblock.interline_distances(textblock.normed_pages([page], 5), 5, 100)[0]
    geom = {"l%d" % i: (p, v) for i, (p, v) in enumerate(zip(n50, d_tr.tolist()))}
    jobs, end = textblock._region_jobs(art, geom, 75)
    assert end is None
    big = [pts for pts, _ in jobs if len(pts) > 3]
    quiet = lambda s: None      # noqa: E731
    host = textblock.create_text_regions(art, geom, 75, quiet)
    assert textblock.create_text_regions(art, geom, 75, quiet, device_regions=True) == host
    tris = [textblock.triangulate(p) for p in big]
    res = {"baselines": len(page), "articles": len(jobs), "articles_over_3_points": len(big),
           "points": int(sum(len(p) for p in big)), "triangles": int(sum(len(t[1]) for t in tris)),
           "largest_article_points": int(max(len(p) for p in big)), "reps": reps}
    dev_in = [[t + (75.0,) for t in tris]]
    got = textblock.alpha_shapes_device(dev_in)[0]
    res["ring_edges_min_max"] = [int(min(len(g[0]) for g in got)), int(max(len(g[0]) for g in got))]
    res["retries_total"] = int(sum(g[1] for g in got))
    res["triangulation_s"] = _median_time(lambda: [textblock.triangulate(p) for p in big], reps)
    k0, k1, calls = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        textblock.alpha_shapes_device(dev_in)
        calls.append(time.perf_counter() - t0)
        k0.append(textblock.last_alpha_shape_kernel_us(0))
        k1.append(textblock.last_alpha_shape_kernel_us(1))
    res["circum_kernel_us"] = [statistics.median(k0), min(k0), max(k0)]
    res["boundary_kernel_us"] = [statistics.median(k1), min(k1), max(k1)]
    res["engine_call_s"] = [statistics.median(calls), min(calls), max(calls)]
    # the triangulation on the device too: the same articles as point lists, the rings compared as cycles first
    def canon(p, ring):
        bp = p[ring].tolist()
        return textblock.canonical_ring(bp + [bp[0]])
    pts_in = [[(p, 75.0) for p in big]]
    got_p = textblock.alpha_shapes_points_device(pts_in)[0]
    assert all(g[3] == 0 and g[1] == w[1] and g[2] == w[2] and canon(p, g[0]) == canon(p, w[0]) for g, w, p in zip(got_p, got, big))
    kd, calls_p = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        textblock.alpha_shapes_points_device(pts_in)
        calls_p.append(time.perf_counter() - t0)
        kd.append(textblock.last_delaunay_kernel_us())
    res["delaunay_kernel_us"] = [statistics.median(kd), min(kd), max(kd)]
    res["points_engine_call_s"] = [statistics.median(calls_p), min(calls_p), max(calls_p)]
    res["host_triangulation_plus_engine_call_s"] = res["triangulation_s"][0] + res["engine_call_s"][0]
    res["device_triangulation_regions_s"] = _median_time(
        lambda: textblock.create_text_regions(art, geom, 75, quiet, device_regions=True, device_triangulation=True), reps)
    res["host_regions_s"] = _median_time(lambda: textblock.create_text_regions(art, geom, 75, quiet), reps)
    res["device_regions_s"] = _median_time(lambda: textblock.create_text_regions(art, geom, 75, quiet, device_regions=True), reps)
    # the command line, in-process: files clustered once, restored before every run, the two ways alternating
    tmp = tempfile.mkdtemp(prefix="as_bench_")
    try:
        paths = [os.path.join(tmp, "p%03d.xml" % k) for k in range(n_pages)]
        for p in paths:
            tbb._write_page(p, page)
        rbc.process(paths, rbc.build_parser().parse_args(["--num_threads", "16"]), 0, quiet)
        keep = os.path.join(tmp, "keep")
        os.makedirs(keep)
        for p in paths:
            shutil.copyfile(p, os.path.join(keep, os.path.basename(p)))
        rate = {"host": [], "device": [], "device_triangulation": []}
        for r in range(reps + 1):
            for which in rate:
                for p in paths:
                    shutil.copyfile(os.path.join(keep, os.path.basename(p)), p)
                flags = rtg.build_parser().parse_args(["--num_threads", "16", "--device_regions", str(which != "host"),
                                                       "--device_triangulation", str(which == "device_triangulation")])
                t0 = time.perf_counter()
                errs = rtg.process(paths, flags, 0, quiet)
                dt = time.perf_counter() - t0
                assert not errs, errs
                if r:                                    # the first round warms both ways up
                    rate[which].append(n_pages / dt)
        for which in rate:
            res["textregion_generation_pages_per_s_" + which] = [statistics.median(rate[which]), min(rate[which]), max(rate[which])]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return res


def size_bench(sizes, reps):
    """one article of n jittered lattice points: scipy on the host against the triangulation kernel (one workgroup)"""
    import alpha_shape_cases as ac
    from citlab_article_separation_new_amd import textblock
    out = {}
    for n in sizes:
        pts = ac.big_article(n)
        host = _median_time(lambda: textblock.triangulate(pts), reps)
        assert textblock.delaunay_device([pts])[0][2] == 0
        us = []
        for _ in range(reps):
            textblock.delaunay_device([pts])
            us.append(textblock.last_delaunay_kernel_us())
        out[str(n)] = {"host_triangulation_s": host, "delaunay_kernel_us": [statistics.median(us), min(us), max(us)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pages", type=int, default=4, help="files per command line run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="lines360,lines1500")
    ap.add_argument("--article_points", default="280,896,897,2000,4000,7681", help="single articles for the triangulation kernel")
    a = ap.parse_args()
    pages = tbb.bench_pages()
    out = {"method": "medians [median, min, max] of --reps runs after a warm-up run; seconds unless the key says us",
           "host_threads": 16, "pages": {}}
    for name in a.sizes.split(","):
        out["pages"][name] = page_bench(pages[name], a.pages, a.reps)
        print(name, json.dumps(out["pages"][name]), flush=True)
    if a.article_points:
        out["delaunay_by_article_points"] = size_bench([int(v) for v in a.article_points.split(",")], a.reps)
        print("by article points", json.dumps(out["delaunay_by_article_points"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
