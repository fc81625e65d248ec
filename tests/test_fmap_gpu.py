"""GPU parity of the relation net's GENERATED feature maps (feature_map_generators.py:72-197; csrc/fmap_kernels.h): map by map against the
numpy restatement tests/fmap_reference.py (pinned to the reference by tests/golden/fmap_golden.npz), degenerate sizes, the whole visual
forward, the batch entry, the session mirror and the command line, and that the default layout launches none of the new kernels."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fmap_reference as fr  # noqa: E402

pytestmark = pytest.mark.gpu

UP2, UP1, UP0 = "scale_0_unet_up_2_conv", "scale_0_unet_up_1_conv", "scale_0_unet_up_0_conv"
LAYERS = [UP1, UP1, "", "", UP0]
DEPTHS = [-1, 6, 8, 2, 12]
DIMS = [8, 6, 4, 3, 5]


def _setup(layers=LAYERS, depths=DEPTHS, dims=DIMS, seed=11, backbone=None, mvn=True, **kw):
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.gnn_io import GnnGraph
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    cfg = GnnConfig(node_feature_dim=7, visual_dims=list(dims), visual_layers=list(layers), visual_layer_depths=list(depths), mvn=mvn,
                    backbone=dict(backbone or {}), **kw)
    w = init_gnn_weights(cfg, seed, bias_jitter=0.05)
    return cfg, w, GnnGraph(w, cfg)


def _page(rng, N, h, w, P=4):
    """the regions of tests/test_gnn_visual_gpu.py::_page: node 0 the full page, node 1 without points, node 2 a single point"""
    from citlab_article_separation_new_amd import synth
    img = synth.synth_page(5, W=w, H=h).astype(np.float32)
    regions = np.zeros((N, 2, P), np.float32)
    npts = np.full(N, P, np.int32)
    for n in range(N):
        x0, y0 = rng.random() * 0.8, rng.random() * 0.8
        x1, y1 = x0 + 0.02 + rng.random() * 0.18, y0 + 0.01 + rng.random() * 0.1
        regions[n, 0] = [x0, x1, x1, x0]
        regions[n, 1] = [y0, y0, y1, y1]
    regions[0, 0, :] = [0.0, 1.0, 1.0, 0.0]
    regions[0, 1, :] = [0.0, 0.0, 1.0, 1.0]
    npts[1] = 0
    if N > 2:
        regions[2, :, :] = 0.5
    if N > 3:
        npts[3] = 2
    return img, regions, npts


def _get_endpoint(graph, name):
    """asep_aru_get_endpoint of the handle's backbone -> float32 [h, w, C]"""
    from citlab_article_separation_new_amd import _lib
    lib = _lib.init_device(0)
    h = graph._backbones[0].handle(0)
    dims = (C.c_int32 * 3)()
    n = _lib.check(lib.asep_aru_get_endpoint(h, name.encode(), None, 0, dims), "asep_aru_get_endpoint")
    out = np.empty(n, np.float32)
    _lib.check(lib.asep_aru_get_endpoint(h, name.encode(), out.ctypes.data, n, dims), "asep_aru_get_endpoint")
    return out.reshape(dims[0], dims[1], dims[2])


def _graph_inputs(N, seed=1, n_pairs=80):
    from citlab_article_separation_new_amd import synth
    return synth.synth_graph(seed, N=N, n_pairs=n_pairs, node_dim=7)


@pytest.mark.parametrize("hw", [(37, 52), (64, 48)])
def test_every_generated_map_matches_the_restatement_on_the_engines_end_points(hw):
    """Stage by stage: each map read back with asep_gnn_get_feature_map against generated_maps (float64) evaluated on the engine's OWN end
    points (asep_aru_get_endpoint).  Stride 1, stride 2 on even and odd sides, widths 1, 3, 4 and 6, a chain of two strided maps.
    Gate: max|d| <= 1e-5 * max(1, max|ref|) (the longest sum has 9 * 128 fp32 terms; the fp32 engine's per-layer gates are of this order).
    The float32 evaluation of the restatement is itself 3.5e-7 (37 x 52) and 3.3e-7 (64 x 48) from its float64 evaluation (relative to
    max(1, max|ref|); the same weights on uniform random end points of these sizes, on the CPU): far inside 1e-5, so the gate stays 1e-5."""
    from citlab_article_separation_new_amd import gnn_io
    cfg, w, graph = _setup(backbone={"compute_dtype": "f32"})
    rng = np.random.default_rng(3)
    N = 6
    g = _graph_inputs(N, n_pairs=10)
    img, regions, npts = _page(rng, N, *hw)
    gnn_io.gnn_forward_visual(graph, N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts)
    eps = {n: _get_endpoint(graph, n) for n in (UP1, UP0)}
    ref = fr.generated_maps(eps, LAYERS, DEPTHS, w)
    h1, w1 = -(-hw[0] // 2), -(-hw[1] // 2)
    shapes = [(h1, w1, 16), (h1, w1, 6), (-(-h1 // 2), -(-w1 // 2), 8), (-(-(-(-h1 // 2)) // 2), -(-(-(-w1 // 2)) // 2), 2), (hw[0], hw[1], 12)]
    for i, r in enumerate(ref):
        got = gnn_io.gnn_feature_map(graph, i)
        assert got.shape == r.shape == shapes[i], (i, got.shape, r.shape, shapes[i])
        d, scale = float(np.abs(got - r).max()), max(1.0, float(np.abs(r).max()))
        print(f"page {hw}: map {i} {got.shape}: max|d| = {d:.3e}, max|ref| = {float(np.abs(r).max()):.3e}")
        assert d <= 1e-5 * scale, (i, d)
        if DEPTHS[i] == -1:
            assert np.array_equal(got, eps[LAYERS[i]])
        else:
            assert (r > 0).any()                                     # the ReLU is not dead everywhere
    graph.close()


def test_degenerate_sizes_down_to_a_one_cell_map():
    """Page 21 x 30, up_2 (6 x 8) and three strided maps: 3 x 4, 2 x 2, 1 x 1.  Shapes exact, the 1 x 1 map equals the restatement, and the
    ROI maximum of a one-cell map is that cell (every node's compressed feature of map 3 is the same row).  fp32 backbone."""
    from citlab_article_separation_new_amd import gnn_io
    layers, depths, dims = [UP2, "", "", ""], [-1, 4, 4, 4], [4, 3, 3, 5]
    cfg, w, graph = _setup(layers, depths, dims, backbone={"compute_dtype": "f32"})
    rng = np.random.default_rng(5)
    N = 5
    g = _graph_inputs(N, n_pairs=8)
    img, regions, npts = _page(rng, N, 21, 30)
    gnn_io.gnn_forward_visual(graph, N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts)
    u = gnn_io.gnn_node_features(graph, N)
    eps = {UP2: _get_endpoint(graph, UP2)}
    ref = fr.generated_maps(eps, layers, depths, w)
    got = [gnn_io.gnn_feature_map(graph, i) for i in range(4)]
    assert [m.shape for m in got] == [(6, 8, 32), (3, 4, 4), (2, 2, 4), (1, 1, 4)] == [m.shape for m in ref]
    for i in range(4):
        d = float(np.abs(got[i] - ref[i]).max())
        print(f"21 x 30: map {i} {got[i].shape}: max|d| = {d:.3e}")
        assert d <= 1e-5 * max(1.0, float(np.abs(ref[i]).max()))
    cell = got[3][0, 0]
    want = np.maximum(cell @ w["visual_node_feature_compression_fm_3/dense/weights"] + w["visual_node_feature_compression_fm_3/dense/bias"], 0)
    assert u.shape == (N, 7 + sum(dims))
    assert np.abs(u[:, -5:] - want[None]).max() <= 1e-6 * max(1.0, float(np.abs(want).max()))
    assert np.array_equal(u[:, -5:], np.repeat(u[:1, -5:], N, axis=0))
    graph.close()


@pytest.mark.parametrize("dtype,visual_edges", [("f32", False), ("f32s", False), ("bf16", False), ("f32", True)])
def test_visual_forward_over_generated_maps_matches_the_oracle(dtype, visual_edges):
    """N = 30 nodes on a 200 x 136 page, the layout of the map test: node features and probabilities against forward_visual_maps (the
    oracle's graph over the restated maps) with the gates of tests/test_gnn_visual_gpu.py: 1e-4 * max(1, max|u|) and 1e-5 for the fp32
    backbones, 2e-2 and 2e-2 (and du > 0) for a bf16 backbone."""
    from citlab_article_separation_new_amd import gnn_io
    cfg, w, graph = _setup(backbone={"compute_dtype": dtype}, visual_edges=visual_edges)
    rng = np.random.default_rng(3)
    N = 30
    g = _graph_inputs(N)
    img, regions, npts = _page(rng, N, 200, 136)
    kw = {}
    if visual_edges:
        from test_gnn_visual_gpu import _edge_regions
        er, enp = _edge_regions(rng, regions, g["interacting_nodes"])
        kw = dict(edge_regions=er, edge_num_points=enp)
    probs = gnn_io.gnn_forward_visual(graph, N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts, **kw)
    u = gnn_io.gnn_node_features(graph, N)
    ref_probs, ref_u = fr.forward_visual_maps(N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts, None, w, cfg, **kw)
    du, dp, mu = float(np.abs(u - ref_u).max()), float(np.abs(probs - ref_probs).max()), float(np.abs(ref_u).max())
    print(f"{dtype} edges={visual_edges}: max|du| = {du:.3e} (max|u| {mu:.3f}), max|dp| = {dp:.3e}")
    assert u.shape == (N, 7 + sum(DIMS)) and probs.shape == (N * N, 2)
    assert np.array_equal(u[:, :7], ref_u[:, :7])
    for lo, hi in zip(np.cumsum([7] + DIMS[:-1]), np.cumsum([7] + DIMS)[1:]):
        assert (ref_u[:, lo:hi] > 0).any()                           # every map contributes
    if dtype == "bf16":
        assert du <= 2e-2 * max(1.0, mu) and du > 0.0 and dp <= 2e-2
    else:
        assert du <= 1e-4 * max(1.0, mu) and dp <= 1e-5
    graph.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_entry_equals_the_single_page_calls_bit_for_bit(dtype):
    import torch
    from citlab_article_separation_new_amd import gnn_io
    cfg, w, graph = _setup(backbone={"compute_dtype": dtype})
    rng = np.random.default_rng(29)
    h, wd = 200, 136
    pages, keep, singles = [], [], []
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    for b, N in enumerate((24, 17, 31, 9)):
        g = _graph_inputs(N, seed=40 + b, n_pairs=3 * N)
        img, regions, npts = _page(rng, N, h, wd)
        img = np.ascontiguousarray(np.roll(img, 9 * b, axis=1))
        singles.append(gnn_io.gnn_forward_visual(graph, N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts))
        last_map = gnn_io.gnn_feature_map(graph, 3)
        t = [dev(g["interacting_nodes"]), dev(g["node_features"]), dev(g["edge_features"]), dev(img), dev(regions), dev(npts),
             torch.zeros(N * N, 2, device="cuda")]
        keep.append(t)
        pages.append(dict(N=N, E=int(t[0].shape[0]), R=N * N, d_edges=t[0].data_ptr(), d_node_feat=t[1].data_ptr(), d_edge_feat=t[2].data_ptr(),
                          d_image=t[3].data_ptr(), d_regions=t[4].data_ptr(), d_num_points=t[5].data_ptr(), d_relations=None,
                          d_probs_out=t[6].data_ptr()))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for _ in range(2):                                                    # the second call reuses every buffer
        gnn_io.gnn_forward_visual_batch_dev(graph, pages, h, wd, 4, stream.cuda_stream)
    stream.synchronize()
    for t, single in zip(keep, singles):
        assert np.array_equal(t[6].cpu().numpy(), single)
    assert np.array_equal(gnn_io.gnn_feature_map(graph, 3), last_map)    # the read-back serves the batch's last page
    graph.close()


def test_session_mirror_and_pb_roundtrip_match_the_direct_handle(tmp_path):
    from citlab_article_separation_new_amd import gnn_io, pb_import
    from citlab_article_separation_new_amd.gnn_input import build_full_relations
    cfg, w, direct = _setup(seed=5)
    pb = tmp_path / "gnn_fmap.pb"
    extra = [{"name": "graph/map/per_image_standardization/Mean", "op": "Mean"}]
    pb.write_bytes(pb_import.weights_to_graphdef(w, "graph/", extra, meta={"num_transition_steps": cfg.num_transition_steps}))
    graph = gnn_io.load_graph(str(pb), visual_layers=list(LAYERS))
    assert graph.cfg.visual_layer_depths == DEPTHS and graph.cfg.visual_layers == LAYERS and graph.cfg.visual_dims == DIMS and graph.cfg.mvn
    rng = np.random.default_rng(8)
    N = 12
    g = _graph_inputs(N, seed=2, n_pairs=30)
    img, regions, npts = _page(rng, N, 120, 96)
    rel = build_full_relations(N)[0]
    E = g["interacting_nodes"].shape[0]
    feed = {"num_nodes:0": np.array([N], np.int32), "num_interacting_nodes:0": np.array([E], np.int32),
            "interacting_nodes:0": g["interacting_nodes"][None], "node_features:0": g["node_features"][None],
            "edge_features:0": g["edge_features"][None], "image:0": img[None, :, :, None],
            "image_shape:0": np.array([[120, 96, 1]], np.int32), "visual_regions_nodes:0": regions[None],
            "num_points_visual_regions_nodes:0": npts[None], "relations_to_consider_belong_to_same_instance:0": rel[None]}
    with gnn_io.GnnSession(graph) as sess:
        out = sess.run("output_belong_to_same_instance:0", feed)
    want = gnn_io.gnn_forward_visual(direct, N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts, rel)
    assert out.shape == (1, N * N, 2) and np.array_equal(out[0], want)
    graph.close(); direct.close()


def test_old_attach_entry_still_refuses_nothing_it_served_and_new_entry_refuses_bad_layouts():
    from citlab_article_separation_new_amd import _lib
    cfg, w, graph = _setup()
    lib = _lib.init_device(0)
    h = graph.handle(0)
    bb = graph._backbones[0].handle(0)
    def attach(names, depths):
        return lib.asep_gnn_attach_backbone_maps(h, bb, len(names), (C.c_char_p * len(names))(*[n.encode() for n in names]),
                                                 (C.c_int32 * len(depths))(*depths))
    for names, depths, reason in (([""], [8], "empty from_layer"), ([UP1, ""], [-1, -1], "layer_depth -1"), ([UP1, UP1], [-1, 7], "even depth"),
                                  ([UP1, ""], [-1, 0], "even depth"), ([UP1, ""], [-1, 258], "to 256")):
        assert attach(names, depths) < 0
        assert reason in _lib.last_error(), _lib.last_error()
    assert attach(LAYERS, DEPTHS) == 0                                   # a second attach replaces (and frees) the first
    graph.close()


def _fmap_launches(graph, run):
    """kernel names the backbone handle's launch profile recorded during run() (the recorder of tests/launch_records.py: asep_aru_profile
    mode 2 and asep_aru_profile_report)"""
    import torch
    import launch_records  # noqa: F401  (the same profile calls, on the relation net's backbone)
    from citlab_article_separation_new_amd import _lib
    lib = _lib.init_device(0)
    graph.handle(0)
    h = graph._backbones[0].handle(0)
    _lib.check(lib.asep_aru_profile(h, 2), "asep_aru_profile")
    try:
        run()
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 20)
        _lib.check(lib.asep_aru_profile_report(h, buf, len(buf)), "asep_aru_profile_report")
    finally:
        lib.asep_aru_profile(h, 0)
    return [(r["kernel"], int(r["calls"])) for r in json.loads(buf.value.decode())]


def test_default_layout_launches_no_generator_kernel_and_a_generated_layout_does():
    from citlab_article_separation_new_amd import gnn_io
    rng = np.random.default_rng(4)
    N = 8
    g = _graph_inputs(N, n_pairs=12)
    img, regions, npts = _page(rng, N, 96, 80)
    for layers, depths, dims, want in (([UP1, UP0], [-1, -1], [4, 4], 0), ([UP1, UP0], [], [4, 4], 0), (LAYERS, DEPTHS, DIMS, 8)):
        cfg, w, graph = _setup(layers, depths, dims)
        recs = _fmap_launches(graph, lambda: gnn_io.gnn_forward_visual(graph, N, g["interacting_nodes"], g["node_features"],
                                                                          g["edge_features"], img, regions, npts))
        fmap = [(k, c) for k, c in recs if k.startswith("fmap_")]
        assert recs and sum(c for _, c in fmap) == want, fmap            # four generated maps: a 1x1 and a 3x3 launch each
        if want:
            assert any(k.startswith("fmap_conv1x1_kernel<false>") for k, _ in fmap) and any(k.startswith("fmap_conv3x3_kernel") for k, _ in fmap)
        graph.close()


def test_run_gnn_clustering_with_the_reference_spelling_writes_the_api_article_ids(tmp_path):
    """two synthetic pages through `run_gnn_clustering --feature_map_generation_params from_layer=[...] layer_depth=[...]`: the article ids
    it writes are those of the same feeds through the Python API (load_graph(visual_layers=, visual_layer_depths=) + GnnSession) and the
    same clustering"""
    from citlab_article_separation_new_amd import gnn_io, gnn_results, pb_import, run_gnn_clustering, synth
    from citlab_article_separation_new_amd.clustering import TextblockClustering
    from citlab_article_separation_new_amd.gnn_input import InputGNN
    from citlab_article_separation_new_amd.page_xml import Page
    layers, depths = [UP1, "", ""], [-1, 8, 6]
    cfg, w, _ = _setup(layers, depths, [16, 16, 16], seed=9, mvn=False)
    argv = synth.write_gnn_cli_inputs(str(tmp_path), 2, visual=True, W=300, H=450, N=30)
    argv = argv[:argv.index("--visual_layers")]                          # the helper's own (default) layout: replaced below
    pb = tmp_path / "model" / "export" / "gnn_best_1.pb"
    pb.write_bytes(pb_import.weights_to_graphdef(w, "graph/", meta={"num_transition_steps": cfg.num_transition_steps}))
    spelled = ["--feature_map_generation_params", f"from_layer=[{UP1},,]", "layer_depth=[-1,8,6]"]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        outs = run_gnn_clustering.main(argv + spelled + ["--out_dir", "out", "--gpu_devices", "0"])
        flags = run_gnn_clustering.build_parser().parse_known_args(argv + ["--visual_layers"] + layers + ["--visual_layer_depths"] + [str(d) for d in depths])[0]
        graph = gnn_io.load_graph(str(pb), visual_layers=layers, visual_layer_depths=depths)
        assert graph.cfg.layer_depths() == depths
        input_fn = InputGNN(flags)
        expected = {}
        with gnn_io.GnnSession(graph) as sess:
            for jp in [p for p in open(flags.eval_list).read().split("\n") if p]:
                feed, n = run_gnn_clustering._prepare_feed(input_fn, flags, jp)
                out = sess.run("output_belong_to_same_instance:0", feed)
                tb = TextblockClustering(flags)
                tb.set_confs(gnn_results.confidences_from_output(out, n))
                tb.calc(method=flags.clustering_method)
                expected[os.path.basename(jp)[:-5]] = [f"a{int(v)}" for v in tb.tb_labels]
        graph.close()
    finally:
        os.chdir(cwd)
    assert len(outs) == 2
    for out in outs:
        out = os.path.join(tmp_path, out) if not os.path.isabs(out) else out
        name = os.path.basename(out).replace("_clustering.xml", "")
        got = [r.text_lines[0].get_article_id() for r in Page(out).get_regions()["TextRegion"]]
        assert got == expected[name], name
