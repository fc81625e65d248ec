"""Device time of the relation net's feature-map generator (csrc/fmap_kernels.h) against the backbone that feeds it, in one run.

Layout [up_2, -1], [up_1, 32], ['', 32], ['', 32] at the relation net's page size (683 x 1024), 200 nodes, f32s and bf16 backbones.
Per repetition the backbone handle records every launch with a pair of events (asep_aru_profile mode 2: one launch at a time, the
generator's launches in the same report), so a kernel's figure is its own device time, not the call's wall time.  Reported per kernel:
median / min / max over the repetitions after a warm-up, its algorithmic bytes (input, filter and output once) and the bandwidth that
figure implies.  HBM bytes actually moved need hardware counters and are not collected here.

    python scripts/fmap_bench.py --out profiles/fmap/gpu.json [--reps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

UP2, UP1 = "scale_0_unet_up_2_conv", "scale_0_unet_up_1_conv"
LAYERS, DEPTHS, DIMS = [UP2, UP1, "", ""], [-1, 32, 32, 32], [16, 16, 16, 16]
H, W, N = 1024, 683, 200


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def run(dtype, reps, warmup):
    import torch
    from citlab_article_separation_new_amd import _lib, gnn_io, synth
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    cfg = GnnConfig(node_feature_dim=7, visual_dims=DIMS, visual_layers=LAYERS, visual_layer_depths=DEPTHS, mvn=True,
                    backbone={"compute_dtype": dtype})
    graph = gnn_io.GnnGraph(init_gnn_weights(cfg, 3, bias_jitter=0.05), cfg)
    lib = _lib.init_device(0)
    graph.handle(0)
    bb = graph._backbones[0].handle(0)
    g = synth.synth_graph(0, N=N, n_pairs=10000, node_dim=7)
    page = synth.synth_page(0, W=W, H=H)
    img, regions, npts = synth.visual_inputs(page, N, 0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    t = [dev(g["interacting_nodes"]), dev(g["node_features"]), dev(g["edge_features"]), dev(np.asarray(img, np.float32)),
         dev(np.asarray(regions, np.float32)), dev(np.asarray(npts, np.int32)), torch.zeros(N * N, 2, device="cuda")]
    h, w = int(t[3].shape[0]), int(t[3].shape[1])

    def forward():
        gnn_io.gnn_forward_visual_dev(graph, N, t[0].shape[0], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), h, w,
                                      t[4].data_ptr(), int(t[4].shape[2]), t[5].data_ptr(), N * N, None, t[6].data_ptr(), None)
    for _ in range(warmup):
        forward()
    torch.cuda.synchronize()
    per_kernel, backbone_ms, meta = {}, [], {}
    buf = C.create_string_buffer(1 << 20)
    for _ in range(reps):
        _lib.check(lib.asep_aru_profile(bb, 2), "asep_aru_profile")
        try:
            forward()
            torch.cuda.synchronize()
            _lib.check(lib.asep_aru_profile_report(bb, buf, len(buf)), "asep_aru_profile_report")
        finally:
            lib.asep_aru_profile(bb, 0)
        recs = json.loads(buf.value.decode())
        backbone_ms.append(sum(r["total_ms"] for r in recs if not r["kernel"].startswith("fmap_")))
        for r in recs:
            if r["kernel"].startswith("fmap_"):
                per_kernel.setdefault(r["kernel"], []).append(r["total_ms"])
                meta[r["kernel"]] = {"calls": r["calls"], "algorithmic_bytes": r["bytes"], "flops": r["flops"]}
    # the whole call, unprofiled, with torch events: the generated layout against the same net without the three generated maps
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record(); forward(); ev[2 * i + 1].record()
    torch.cuda.synchronize()
    call_ms = [ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(reps)]
    graph.close()
    kernels = {}
    for k, v in per_kernel.items():
        s = spread(v)
        kernels[k] = {"ms": s, **meta[k], "algorithmic_GB_per_s": meta[k]["algorithmic_bytes"] / (s["median"] * 1e-3) / 1e9,
                      "GFLOP_per_s": meta[k]["flops"] / (s["median"] * 1e-3) / 1e9}
    gen = [sum(per_kernel[k][i] for k in per_kernel) for i in range(reps)]
    return {"compute_dtype": dtype, "page": [h, w], "nodes": N, "layout": {"from_layer": LAYERS, "layer_depth": DEPTHS},
            "generator_kernels": kernels, "generator_ms_per_page": spread(gen), "backbone_ms_per_page": spread(backbone_ms),
            "generator_share_of_backbone": statistics.median(gen) / statistics.median(backbone_ms),
            "visual_forward_call_ms_unprofiled": spread(call_ms),
            "note": "per-launch event pairs, one launch at a time (asep_aru_profile mode 2); backbone = the sum of its launches in the same report"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fmap/gpu.json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {"runs": [run(d, a.reps, a.warmup) for d in ("f32s", "bf16")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for r in out["runs"]:
        print(json.dumps({"dtype": r["compute_dtype"], "generator_ms": r["generator_ms_per_page"], "backbone_ms": r["backbone_ms_per_page"],
                          "share": r["generator_share_of_backbone"]}))


if __name__ == "__main__":
    main()
