"""Files in, files out for the relation net: graph jsons (+ scans for the visual net) + PAGE-XML -> run_gnn_clustering command
line -> PAGE-XML with article ids.  200 text blocks / ~20k directed edges / 40k pairs per page (BASELINE configs[3]).

    python scripts/e2e_gnn_bench.py [n_pages=64] [workers=8] [visual=1] [--load_mode L|RGB] [--device_resize True|False]
                                    [--workers_list 1,8,16] [--repeat 1] [--json out.json]

--load_mode RGB: colour scans into a 3-channel backbone.  --device_resize is handed to the command line when given (a tree without the
flag ignores it: parse_known_args).  --json appends one record per run to a json list."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("n_pages", nargs="?", type=int, default=64)
ap.add_argument("workers", nargs="?", type=int, default=8)
ap.add_argument("visual", nargs="?", type=int, default=1)
ap.add_argument("--load_mode", default="L", choices=["L", "RGB"])
ap.add_argument("--device_resize", default=None)
ap.add_argument("--workers_list", default=None)
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("--json", default=None)
args = ap.parse_args()
n_pages, workers, visual = args.n_pages, args.workers, bool(args.visual)


def main():
    import inspect
    from citlab_article_separation_new_amd import run_gnn_clustering, synth
    records = []
    with tempfile.TemporaryDirectory(prefix="asep_gnn_e2e_") as tmp:
        t0 = time.perf_counter()
        kw = {"load_mode": args.load_mode} if "load_mode" in inspect.signature(synth.write_gnn_cli_inputs).parameters else {}
        if args.load_mode != "L" and not kw:
            raise SystemExit("this tree's synth.write_gnn_cli_inputs writes gray scans only")
        argv = synth.write_gnn_cli_inputs(tmp, n_pages, visual=visual, **kw)
        if args.device_resize is not None:
            argv += ["--device_resize", args.device_resize]
        # what the command line resizes with: the flag's effective value, "host" on a tree that has no such flag
        effective = getattr(run_gnn_clustering.build_parser().parse_known_args(argv)[0], "device_resize", None)
        resize = "host" if not effective or not visual else "device"
        lst = argv[argv.index("--eval_list") + 1]
        jsons = [ln for ln in open(lst).read().split("\n") if ln]
        print(f"inputs written in {time.perf_counter() - t0:.1f} s; json {os.path.getsize(jsons[0]) / 1e6:.2f} MB per page")
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            counts = sorted({int(v) for v in args.workers_list.split(",")}) if args.workers_list else sorted({1, workers})
            for nw in counts:
                part = jsons if nw > 1 else jsons[: max(8, n_pages // 8)]
                with open(lst, "w") as f:
                    f.write("\n".join(part) + "\n")
                for rep in range(args.repeat):
                    t0 = time.perf_counter()
                    outs = run_gnn_clustering.main(argv + ["--out_dir", f"out{nw}_{rep}", "--gpu_devices", "0", "--num_workers", str(nw)])
                    dt = time.perf_counter() - t0
                    print(f"run_gnn_clustering, {'visual' if visual else 'geometric'} net, load_mode={args.load_mode}, {resize} resize, {nw:2d} worker(s): "
                          f"{len(outs)} pages in {dt:.2f} s = {len(outs) / dt:.1f} pages/s ({dt / len(outs) * 1e3:.1f} ms/page incl. start-up)",
                          flush=True)
                    records.append({"visual": visual, "load_mode": args.load_mode, "resize": resize, "workers": nw,
                                    "list": f"{len(part)} pages, start-up included", "run": rep, "pages": len(outs), "seconds": round(dt, 3), "pages_per_s": round(len(outs) / dt, 2)})
        finally:
            os.chdir(cwd)
            if args.json:
                old = json.load(open(args.json)) if os.path.exists(args.json) else []
                with open(args.json, "w") as f:
                    json.dump(old + records, f, indent=1)


if __name__ == "__main__":
    main()
