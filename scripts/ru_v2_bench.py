"""What the input pyramid of graph 'RU_v2' costs: one forward of a 3000 x 4500 gray page, graph RU_v2 (defaults) against graph RU, same
build, same device, arithmetic f32s; and the tap kernel's time per level against its algorithmic bytes.  A number to record, not a gate.

    python scripts/ru_v2_bench.py [--out profiles/ru_v2/gpu.json] [--rounds 7] [--steps 10] [--warmup 5]

Timing: both models stay loaded; after `warmup` forwards of each, `rounds` rounds alternate between the two graphs, each round `steps`
forwards on device buffers between two device synchronisations (host clock).  Reported: the median round per graph and the spread.  The
per-kernel times come from a pass of its own with the engine's launch recorder (asep_aru_profile mode 2: one stream, one lane)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ru_v2", "gpu.json"))
    ap.add_argument("--height", type=int, default=4500)
    ap.add_argument("--width", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from citlab_article_separation_new_amd import _lib, synth
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    from citlab_article_separation_new_amd.weights import init_aru_weights
    lib = _lib.init_device(0)
    H, W = args.height, args.width
    page = torch.from_numpy(synth.synth_page(0, W, H).astype(np.float32) / 255.0).cuda()
    out = torch.empty(H, W, 2, device="cuda")
    graphs, handles = {}, {}
    for name in ("RU_v2", "RU"):
        cfg = AruConfig(graph=name, compute_dtype="f32s")
        graphs[name] = AruGraph(init_aru_weights(cfg, 21, logit_scale=0.05), cfg)
        handles[name] = graphs[name].handle(0)

    def forward(name, n):
        for _ in range(n):
            _lib.check(lib.asep_aru_forward_dev(handles[name], page.data_ptr(), H, W, out.data_ptr(), None, None, 0.0, None), "asep_aru_forward_dev")
        torch.cuda.synchronize()

    for name in handles:
        forward(name, args.warmup)
    ms = {name: [] for name in handles}
    for _ in range(args.rounds):
        for name in handles:
            t0 = time.perf_counter()
            forward(name, args.steps)
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res = {"page": [H, W], "compute_dtype": "f32s", "rounds": args.rounds, "steps": args.steps, "warmup": args.warmup,
           "forward_ms": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}}
    res["ratio_ru_v2_over_ru"] = res["forward_ms"]["RU_v2"]["median"] / res["forward_ms"]["RU"]["median"]
    res["flops"] = {k: float(lib.asep_aru_flops(handles[k], H, W)) for k in handles}

    # per-launch records of ONE forward of each graph (recording serialises the net: these are kernel times, not the forward's)
    for name in handles:
        _lib.check(lib.asep_aru_profile(handles[name], 2), "asep_aru_profile")
        forward(name, 1)
        buf = C.create_string_buffer(1 << 20)
        _lib.check(lib.asep_aru_profile_report(handles[name], buf, len(buf)), "asep_aru_profile_report")
        lib.asep_aru_profile(handles[name], 0)
        recs = json.loads(buf.value.decode())
        res.setdefault("kernels", {})[name] = sorted(
            ({"kernel": r["kernel"], "calls": r["calls"], "us": r["total_ms"] * 1e3, "bytes": r["bytes"],
              "GBps": r["bytes"] / (r["total_ms"] * 1e-3) / 1e9 if r["total_ms"] > 0 else None} for r in recs), key=lambda r: -r["us"])
    taps = [r for r in res["kernels"]["RU_v2"] if r["kernel"].startswith("pyr_tap_kernel")]
    res["tap_us_total"] = sum(r["us"] for r in taps)
    res["level0_up_us"] = {name: sum(r["us"] for r in res["kernels"][name] if "unet_up_0" in r["kernel"] and "deconv" not in r["kernel"])
                           for name in handles}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("forward_ms", "ratio_ru_v2_over_ru", "tap_us_total", "level0_up_us")}))
    for r in taps:
        print(f"{r['us']:9.1f} us {r['GBps']:8.1f} GB/s  {r['kernel']}")
    for g in graphs.values():
        g.close()


if __name__ == "__main__":
    main()
