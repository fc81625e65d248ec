#!/usr/bin/env python
"""Per-page cost of the relation net's graph part: page by page (asep_gnn_forward[_dev]) against the pages of a call in one set of launches
(asep_gnn_forward_batch[_dev]) at 1, 4, 16 and 64 pages per call.

Inputs: planted-article graphs (oracle/gnn_cases.planted_graph) of N = 50 and N = 200 nodes, a Delaunay-sized edge list (3 N - 6 undirected
edges), all N * N relations, the default net (7 node / 2 edge features, factored MFMA step, 64-32-2 classifier), 64 distinct pages per size.

Two figures per form, both per page:
  wall_us    the host-pointer entry as a caller pays it: upload, launches, download, one synchronisation per call
  device_us  the device-pointer entry on inputs that already lie in HBM: the time between two events around the queued calls of all 64 pages
             (launch gaps included: it is what the stream is busy or waiting for launches)

``--parent_lib`` names a build of the PARENT commit's libasep_hip.so; its single-page and batched entries (``parent_single``, ``parent_batch_<k>``)
run on the same inputs, in the same process and in alternation with this build's (loaded with RTLD_LOCAL | RTLD_DEEPBIND, so that each library
calls its own functions); its batched results and launch record are compared with this build's.  Warm-up rounds, then ``--rounds`` rounds that
visit the forms in turn; the medians over the rounds are reported.  Nothing here asserts a speed-up.

    python scripts/gnn_graph_batch_bench.py --out profiles/gnn_graph_batch/gpu.json [--parent_lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAGES = 64
PER_CALL = (1, 4, 16, 64)


def _load_parent(path):
    """the parent build beside this one: its own symbols first (DEEPBIND), none exported to the process (LOCAL)"""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND | os.RTLD_NOW)
    P = C.c_void_p
    lib.asep_abi_version.restype = C.c_int
    lib.asep_last_error.restype = C.c_char_p
    lib.asep_init.argtypes, lib.asep_init.restype = [C.c_int], C.c_int
    lib.asep_gnn_load.argtypes, lib.asep_gnn_load.restype = [P, C.c_size_t, P], P
    lib.asep_gnn_free.argtypes, lib.asep_gnn_free.restype = [P], None
    lib.asep_gnn_forward.argtypes, lib.asep_gnn_forward.restype = [P, C.c_int, C.c_int, P, P, P, C.c_int, P, P], C.c_int
    lib.asep_gnn_forward_dev.argtypes, lib.asep_gnn_forward_dev.restype = [P, C.c_int, C.c_int, P, P, P, C.c_int, P, P, P], C.c_int
    lib.asep_gnn_forward_batch.argtypes, lib.asep_gnn_forward_batch.restype = [P, C.c_int] + [P] * 8 + [C.c_size_t], C.c_int
    lib.asep_gnn_forward_batch_dev.argtypes, lib.asep_gnn_forward_batch_dev.restype = [P, C.c_int] + [P] * 8 + [C.c_size_t, P], C.c_int
    lib.asep_gnn_batch_launches.argtypes, lib.asep_gnn_batch_launches.restype = [P], C.c_long
    return lib


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 200])
    a = ap.parse_args(argv)

    import torch
    from citlab_article_separation_new_amd import _lib, gnn_io
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    from oracle import gnn_cases

    lib = _lib.init_device(0)
    cfg = GnnConfig()
    graph = gnn_io.GnnGraph(init_gnn_weights(cfg, 1234, bias_jitter=0.05), cfg)
    h_new = graph.handle(0)
    parent = h_old = None
    if a.parent_lib:
        parent = _load_parent(a.parent_lib)
        assert parent.asep_init(0) >= 0, parent.asep_last_error()
        ih, ch = list(cfg.interaction_hidden) + [0] * 4, list(cfg.classifier_hidden) + [0] * 4
        pc = _lib.GnnCfg(cfg.u_dim, cfg.edge_in_dim, cfg.num_transition_steps, cfg.hidden_dim, cfg.interaction_dim, ih[0], ch[0], ch[1],
                         cfg.num_classes, int(cfg.undirected_graph), 0, cfg.output_type_code, 0, 0, 0, cfg.aggregation_code, ih[1], ih[2], ih[3],
                         0, 0, 0, ch[2], ch[3], int(cfg.incorporate_hidden_features_in_update),
                         int(cfg.incorporate_node_input_features_in_update), 0)
        blob = graph.blob()
        h_old = parent.asep_gnn_load(blob, len(blob), C.byref(pc))
        assert h_old, parent.asep_last_error()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream or None
    result = {"device": torch.cuda.get_device_name(0), "pages": PAGES, "rounds": a.rounds, "warmup": a.warmup, "step_mode": gnn_io.step_mode(graph),
              "parent_abi": parent.asep_abi_version() if parent else None, "abi": lib.asep_abi_version(), "sizes": {}}

    for N in a.sizes:
        pages = []
        for k in range(PAGES):
            g = gnn_cases.planted_graph(1000 + k, N=N, n_pairs=3 * N - 6, node_dim=cfg.node_feature_dim, edge_dim=cfg.edge_feature_dim)
            pages.append(dict(N=N, edges=np.ascontiguousarray(g["interacting_nodes"]), u=np.ascontiguousarray(g["node_features"]),
                              ef=np.ascontiguousarray(g["edge_features"]), rel=None))
        E = pages[0]["edges"].shape[0]
        R = N * N
        out1 = np.empty((R, cfg.num_classes), np.float32)
        # device copies: per page for the single entries, per group for the batched entry
        d_pages = [tuple(torch.from_numpy(p[k]).to(dev) for k in ("edges", "u", "ef")) for p in pages]
        d_out1 = torch.empty((R, cfg.num_classes), dtype=torch.float32, device=dev)
        groups = {}
        for P in PER_CALL:
            groups[P] = []
            for s in range(0, PAGES, P):
                Nn, Ee, Rr, u, edges, ef, _ = gnn_io.pack_graph_pages(pages[s:s + P], cfg.node_feature_dim, cfg.edge_feature_dim)
                groups[P].append(dict(N=Nn, E=Ee, R=Rr, u=u, edges=edges, ef=ef, out=np.empty(int(Rr.sum()), np.float32),
                                      d=tuple(torch.from_numpy(x).to(dev) for x in (u, edges, ef)),
                                      d_out=torch.empty(int(Rr.sum()), dtype=torch.float32, device=dev)))
        i32p = gnn_io._i32p

        def single_wall(L, h):
            for p in pages:
                rc = L.asep_gnn_forward(h, N, E, p["edges"].ctypes.data, p["u"].ctypes.data, p["ef"].ctypes.data, R, None, out1.ctypes.data)
                assert rc >= 0

        def single_dev(L, h):
            for e, u, ef in d_pages:
                rc = L.asep_gnn_forward_dev(h, N, E, e.data_ptr(), u.data_ptr(), ef.data_ptr(), R, None, d_out1.data_ptr(), sp)
                assert rc >= 0

        def batch_wall(P, L=lib, h=h_new):
            for g in groups[P]:
                rc = L.asep_gnn_forward_batch(h, len(g["N"]), i32p(g["N"]), i32p(g["E"]), i32p(g["R"]), g["u"].ctypes.data,
                                              g["edges"].ctypes.data, g["ef"].ctypes.data, None, g["out"].ctypes.data, g["out"].size)
                assert rc >= 0, L.asep_last_error()

        def batch_dev(P, L=lib, h=h_new):
            for g in groups[P]:
                rc = L.asep_gnn_forward_batch_dev(h, len(g["N"]), i32p(g["N"]), i32p(g["E"]), i32p(g["R"]), g["d"][0].data_ptr(),
                                                  g["d"][1].data_ptr(), g["d"][2].data_ptr(), None, g["d_out"].data_ptr(), g["d_out"].numel(), sp)
                assert rc >= 0, L.asep_last_error()

        forms = {}
        if parent:
            forms["parent_single"] = (lambda: single_wall(parent, h_old), lambda: single_dev(parent, h_old))
        forms["single"] = (lambda: single_wall(lib, h_new), lambda: single_dev(lib, h_new))
        for P in PER_CALL:
            if parent:
                forms[f"parent_batch_{P}"] = (lambda P=P: batch_wall(P, parent, h_old), lambda P=P: batch_dev(P, parent, h_old))
            forms[f"batch_{P}"] = (lambda P=P: batch_wall(P), lambda P=P: batch_dev(P))

        # the forms agree on the values before anything is timed: page 5 alone (both builds) and as a member of a call of 16
        lib.asep_gnn_forward(h_new, N, E, pages[5]["edges"].ctypes.data, pages[5]["u"].ctypes.data, pages[5]["ef"].ctypes.data, R, None,
                             out1.ctypes.data)
        ref = out1[:, 1].copy()
        batch_wall(16)
        same = bool(np.array_equal(groups[16][0]["out"][5 * R:6 * R].view(np.uint32), ref.view(np.uint32)))
        same_parent = same_parent_batch = None
        if parent:
            parent.asep_gnn_forward(h_old, N, E, pages[5]["edges"].ctypes.data, pages[5]["u"].ctypes.data, pages[5]["ef"].ctypes.data, R, None,
                                    out1.ctypes.data)
            same_parent = bool(np.array_equal(out1[:, 1].view(np.uint32), ref.view(np.uint32)))
            groups[16][0]["out"].fill(-1.0)
            batch_wall(16, parent, h_old)
            same_parent_batch = bool(np.array_equal(groups[16][0]["out"][5 * R:6 * R].view(np.uint32), ref.view(np.uint32)))

        wall = {k: [] for k in forms}
        devt = {k: [] for k in forms}
        for rnd in range(a.warmup + a.rounds):
            for name, (fw, fd) in forms.items():                       # the forms in turn inside every round
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fw()
                t1 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fd()
                e1.record(stream)
                e1.synchronize()
                if rnd >= a.warmup:
                    wall[name].append((t1 - t0) * 1e6 / PAGES)
                    devt[name].append(e0.elapsed_time(e1) * 1e3 / PAGES)
        res = {"N": N, "E_fed": int(E), "R": int(R), "batch_equals_single_bits": same, "parent_equals_single_bits": same_parent,
               "parent_equals_batch_bits": same_parent_batch, "forms": {}}
        for name in forms:
            res["forms"][name] = {"wall_us_per_page": round(statistics.median(wall[name]), 2),
                                  "wall_us_min_max": [round(min(wall[name]), 2), round(max(wall[name]), 2)],
                                  "device_us_per_page": round(statistics.median(devt[name]), 2),
                                  "device_us_min_max": [round(min(devt[name]), 2), round(max(devt[name]), 2)]}
        res["launches_per_call"], res["parent_launches_per_call"] = {}, {} if parent else None
        for P in PER_CALL:                                                 # the launch record of a call at every pages-per-call
            batch_dev(P)
            res["launches_per_call"][str(P)] = gnn_io.gnn_batch_launches(graph)
            if parent:
                batch_dev(P, parent, h_old)
                res["parent_launches_per_call"][str(P)] = parent.asep_gnn_batch_launches(h_old)
        result["sizes"][str(N)] = res
        print(json.dumps(res), flush=True)

    if parent:
        parent.asep_gnn_free(h_old)
    graph.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
