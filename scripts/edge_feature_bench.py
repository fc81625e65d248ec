"""What the per-edge part of the feature generation costs, on the host and on the device.

    python scripts/edge_feature_bench.py --out profiles/edge_features/gpu.json

Synthetic pages from the package's own generator (synth.synth_regions_and_separators; 100 separators a page), three sizes: N = 50 and N = 200
with Delaunay edges, N = 200 fully connected (39 800 edges).  Per size: the kernels' device time (asep_edge_features_last_kernel_us), the wall
time of edge_features_device (packing included) and the wall time of the host loops on the same pages -- `bb` flags, `line` flags, hulls, mask --
each after a warm-up, repeated, with median / min / max.  Then the whole stage, generate_feature_jsons both ways on a small list.  Nothing is
asserted about speed; the results are compared for equality.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "runs": len(values)}


def timed(fn, runs, warmup=1):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, spread(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--pages", type=int, default=4, help="pages per call (the fully connected size: one page, its host loops take minutes)")
    ap.add_argument("--runs", type=int, default=10, help="timed device calls per size")
    ap.add_argument("--host_runs", type=int, default=2, help="timed runs of the host loops at N = 50 (N = 200 runs them once)")
    ap.add_argument("--stage_pages", type=int, default=20)
    args = ap.parse_args()
    from citlab_article_separation_new_amd import edge_features as ef, feature_generation as fg, synth
    result = {"separators_per_page": 100, "sizes": []}
    for name, n, interaction, n_pages in (("n50_delaunay", 50, "delaunay", args.pages), ("n200_delaunay", 200, "delaunay", args.pages),
                                          ("n200_fully", 200, "fully", 1)):
        pages = []
        for k in range(n_pages):
            regions, seps = synth.synth_regions_and_separators(k, n, 100)
            if interaction == "fully":
                edges = fg.fully_connected_edges(n)
            else:
                centers = np.array([[(min(p[0] for p in r.points) + max(p[0] for p in r.points)) / 2,
                                     (min(p[1] for p in r.points) + max(p[1] for p in r.points)) / 2] for r in regions])
                edges = fg.delaunay_edges(n, centers)
            pages.append(ef.EdgePage(regions, seps, edges))
        n_edges = sum(len(p.edges) for p in pages)
        rec = {"name": name, "regions_per_page": n, "edges_per_page": n_edges // n_pages, "pages": n_pages}
        host_runs = 1 if n > 50 else args.host_runs
        host = {}
        for rule, fn in (("bb", fg.get_edge_separator_feature_bb), ("line", fg.get_edge_separator_feature_line)):
            host[rule], rec[f"host_{rule}_ms"] = timed(lambda: [np.array([fn(p.text_regions[a], p.text_regions[b], p.separator_regions)
                                                                          for a, b in p.edges.tolist()]) for p in pages], host_runs, warmup=0)
        host["hull"], rec["host_hulls_ms"] = timed(lambda: [[fg.get_edge_visual_region(p.text_regions[a], p.text_regions[b])
                                                             for a, b in p.edges.tolist()] for p in pages], host_runs, warmup=0)

        def host_mask():
            out = []
            for p in pages:
                bits = np.zeros((n, n), np.uint8)
                for i in range(n):
                    for j in range(i + 1, n):
                        if fg.is_aligned_heading_separated(p.text_regions[i], p.text_regions[j]):
                            bits[i, j] = bits[j, i] = 1
                        if fg.is_aligned_horizontally_separated(p.text_regions[i], p.text_regions[j], p.separator_regions):
                            bits[i, j] |= 2
                            bits[j, i] |= 2
                out.append(bits)
            return out
        host["mask"], rec["host_mask_ms"] = timed(host_mask, host_runs, warmup=0)
        for rule in ("bb", "line"):
            kernel_us = []

            def call():
                res = ef.edge_features_device(pages, rule=rule, hulls=True, pair_bits=True)
                kernel_us.append(ef.last_kernel_us)
                return res
            dev, rec[f"device_{rule}_call_ms"] = timed(call, args.runs, warmup=2)
            rec[f"device_{rule}_kernel_us"] = spread(kernel_us[2:])
            rec[f"device_{rule}_launches"] = ef.last_launches
            same = all(np.array_equal(d["flags"], h) for d, h in zip(dev, host[rule]))
            same = same and all([d["hull"][e, :c].tolist() for e, c in enumerate(d["hull_n"])] == [[list(q) for q in v] for v in h]
                                for d, h in zip(dev, host["hull"]))
            same = same and all(np.array_equal(d["pair_bits"], h) for d, h in zip(dev, host["mask"]))
            rec[f"device_{rule}_equals_host"] = bool(same)
        # what the kernels have to move at least: tables in, results out
        t = ef.pack_pages(pages)
        rec["algorithmic_bytes"] = int(sum(v.nbytes for v in t.values() if hasattr(v, "nbytes")) + 2 * n_edges
                                       + sum(int(d["hull_n"].sum()) * 8 + 4 * len(d["hull_n"]) for d in dev) + n_pages * n * n)
        result["sizes"].append(rec)
        print(json.dumps(rec), flush=True)

    # the whole stage: PAGE-XML + scan -> json files, both ways (visual regions, `line` rule: generate_feature_jsons' defaults)
    from PIL import Image
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "page"))
        paths = []
        for k in range(args.stage_pages):
            Image.fromarray(synth.synth_page(k, W=1500, H=2250)).save(os.path.join(root, f"p{k:02d}.png"), compress_level=1)
            synth.synth_region_page_xml(os.path.join(root, "page", f"p{k:02d}.xml"), k, n_regions=60, n_separators=40, W=1500, H=2250,
                                        image_filename=f"p{k:02d}.png")
            paths.append(os.path.join(root, "page", f"p{k:02d}.xml"))
        stage = {"pages": len(paths), "regions_per_page": 60, "separators_per_page": 40, "interaction": "delaunay", "separators": "line"}
        fg.generate_feature_jsons(paths[:2], os.path.join(root, "warm_host"))
        fg.generate_feature_jsons(paths[:2], os.path.join(root, "warm_dev"), device_edges=True)
        times = {"host": [], "device": []}
        for r in range(3):                                          # alternating, as two versions in one run should be compared
            for which in ("host", "device"):
                t0 = time.perf_counter()
                fg.generate_feature_jsons(paths, os.path.join(root, f"{which}_{r}"), device_edges=which == "device")
                times[which].append((time.perf_counter() - t0) * 1e3)
        stage["host_ms"], stage["device_ms"] = spread(times["host"]), spread(times["device"])
        stage["files_identical"] = all(open(os.path.join(root, "host_0", f), "rb").read() == open(os.path.join(root, "device_0", f), "rb").read()
                                       for f in sorted(os.listdir(os.path.join(root, "host_0"))))
        result["whole_stage"] = stage
        print(json.dumps(stage), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
