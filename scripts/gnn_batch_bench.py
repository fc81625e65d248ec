"""What --pages_per_call gains from the command line: synthetic scans of four sizes (different aspect ratios) through
run_gnn_clustering's inline owner at N = 1, 2, 4, 8.

Per N: wall time per page and pages/s end to end (warm-up run, then REPEATS timed runs, median and min..max spread); the time between two
events on the engine's stream around every engine call, per page (what the device spends on a page's call, uploads included); and from
the backbone handle's launch records of one more run (asep_aru_profile mode 2, which serialises the launches: isolated kernel times) the
recorded launches per page and their device time per page, split into the backbone's layers and the rest of the visual stage (resize,
moments, generated maps, ROI / compression).  The graph part's launches are not in those records: its share is inside the event time only.

    python scripts/gnn_batch_bench.py [--pages 16] [--repeats 5] [--ns 1 2 4 8] [--out profiles/gnn_batch/gpu.json]
    python scripts/gnn_batch_bench.py --package_root <a checkout of the parent commit, built> --ns 1 --out parent.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCANS = [(1500, 1000), (1000, 1400), (1280, 1280), (800, 1540)]      # H x W: the resize (max side 1024, min side 256) leaves four sizes


def make_inputs(root, n_pages, nodes):
    from PIL import Image
    from citlab_article_separation_new_amd import gnn_input, synth
    argv = synth.write_gnn_cli_inputs(root, n_pages, visual=True, W=1000, H=1500, N=nodes)
    data = os.path.join(root, "data")
    sizes = []
    for k in range(n_pages):
        png = os.path.join(data, f"p{k:03d}.png")
        H, W = SCANS[k % 4]
        if k < 4:
            Image.fromarray(synth.cached_synth_page(k, W, H)).save(png, compress_level=1)
        sizes.append(gnn_input.compute_new_size(H, W, 256, 1024))
    return argv + ["--gpu_devices", "0", "--save_conf", "only_conf", "--out_dir", os.path.join(root, "out")], sorted(set(sizes))


def timed_session_loader(r, times):
    """r._load_session wrapped: every engine call of the sessions it loads is bracketed by two events on torch's current stream (the
    stream the session's calls go to); times receives the (start, stop) pairs"""
    import torch
    load = r._load_session

    def load_timed(fl, device):
        sess = load(fl, device)
        run = sess.run

        def timed_run(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = run(*args, **kw)
            e1.record()
            times.append((e0, e1))
            return out
        sess.run = timed_run
        return sess
    return load, load_timed


def profiled_run(json_paths, flags, r):
    """one run with the backbone's launch records on -> [(kernel, calls, total_ms)].  The session is held here until the report has been
    read: gnn_clustering drops its session on return, and a dropped session frees the backbone handle the report is read from"""
    import torch
    from citlab_article_separation_new_amd import _lib
    held = []
    load = r._load_session

    def load_profiled(fl, device):
        sess = load(fl, device)
        sess.graph.handle(0)
        h = sess.graph._backbones[0].handle(0)
        lib = _lib.init_device(0)
        _lib.check(lib.asep_aru_profile(h, 2), "asep_aru_profile")
        held.append((sess, lib, h))
        return sess
    r._load_session = load_profiled
    try:
        r.gnn_clustering(json_paths, flags, "0")
        sess, lib, h = held[0]
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 22)
        _lib.check(lib.asep_aru_profile_report(h, buf, len(buf)), "asep_aru_profile_report")
        lib.asep_aru_profile(h, 0)
        sess.graph.close()
    finally:
        r._load_session = load
    return [(x["kernel"], int(x["calls"]), float(x["total_ms"])) for x in json.loads(buf.value.decode())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=16)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ns", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--package_root", default=ROOT)                  # a built checkout whose package is measured (the parent commit's, for N = 1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnn_batch", "gpu.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from citlab_article_separation_new_amd import gnn_io
    from citlab_article_separation_new_amd import run_gnn_clustering as r
    from citlab_article_separation_new_amd.path_util import load_list_file
    result = {"package_root": os.path.relpath(os.path.abspath(a.package_root), ROOT), "pages": a.pages, "nodes": a.nodes, "repeats": a.repeats, "scans_hw": SCANS, "owner": "run_gnn_clustering.gnn_clustering (inline, host resize)",
              "compute_dtype": os.environ.get("ASEP_COMPUTE_DTYPE", "model default"), "per_n": {}}
    with tempfile.TemporaryDirectory() as root:
        argv, sizes = make_inputs(root, a.pages, a.nodes)
        result["image_sizes_hw"] = sizes
        rest_names = ("prep_resize", "moments", "fmap_conv", "gnn_roi")
        for n in a.ns:
            flags = r.build_parser().parse_known_args(argv + ["--pages_per_call", str(n)])[0]
            paths = [p for p in load_list_file(flags.eval_list) if p]
            r.gnn_clustering(paths, flags, "0")                          # warm-up: model load, arenas, file caches
            walls, events = [], []
            load, load_timed = timed_session_loader(r, events)
            run_pages = getattr(gnn_io, "run_pages", None)
            if run_pages is not None:                                    # N > 1 goes through run_pages, not through sess.run
                def timed_pages(sess, feeds, _f=run_pages):
                    if len(feeds) < 2 or not sess.graph.cfg.visual_dims:
                        return _f(sess, feeds)                           # (falls back to sess.run, which is timed)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = _f(sess, feeds)
                    e1.record()
                    events.append((e0, e1))
                    return out
                gnn_io.run_pages = timed_pages
            r._load_session = load_timed
            try:
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    r.gnn_clustering(paths, flags, "0")
                    walls.append((time.perf_counter() - t0) / len(paths))
            finally:
                r._load_session = load
                if run_pages is not None:
                    gnn_io.run_pages = run_pages
            torch.cuda.synchronize()
            call_ms = sum(e0.elapsed_time(e1) for e0, e1 in events) / (a.repeats * len(paths))
            recs = profiled_run(paths, flags, r)
            rest = [x for x in recs if any(k in x[0] for k in rest_names)]
            bb = [x for x in recs if x not in rest]
            med = statistics.median(walls)
            result["per_n"][str(n)] = {
                "wall_ms_per_page_median": 1e3 * med, "wall_ms_per_page_min": 1e3 * min(walls), "wall_ms_per_page_max": 1e3 * max(walls),
                "pages_per_s_median": 1.0 / med,
                "recorded_launches_per_page": {"backbone": sum(x[1] for x in bb) / len(paths), "rest_of_visual_stage": sum(x[1] for x in rest) / len(paths)},
                "device_ms_per_page_isolated": {"backbone": sum(x[2] for x in bb) / len(paths), "rest_of_visual_stage": sum(x[2] for x in rest) / len(paths)},
                "engine_call_event_ms_per_page": call_ms,
                "graph_part": "not in the launch records; inside engine_call_event_ms_per_page",
            }
            print(n, json.dumps(result["per_n"][str(n)]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
