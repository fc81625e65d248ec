"""The relation net fed with the scan as decoded ('image_u8:0', uint8) and resized on the device, against the same session fed the
image the host resizes (``gnn_input.resize_bilinear_tf1`` -> 'image:0'; Pillow's ``convert('L')`` first for a colour scan into a
gray backbone).  The resize kernel reproduces the host function bit for bit, so the probabilities are compared bit for bit and
the command line's files byte for byte.

The only bytes of a written PAGE-XML that depend on the clock are the text of its ``LastChange`` element (page_xml.write_page_xml
stamps the second of the write): ``_files`` blanks that one element before comparing, everything else is compared as written."""
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYERS = ("scale_0_unet_up_1_conv", "scale_0_unet_up_0_conv")
OUTPUT = "output_belong_to_same_instance:0"


def _setup(channels, seed=11):
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.gnn_io import GnnGraph
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    cfg = GnnConfig(node_feature_dim=7, visual_dims=[16, 8], visual_layers=list(LAYERS), mvn=True,
                    backbone={"channels": channels, "scale_space_num": 3})
    w = init_gnn_weights(cfg, seed, bias_jitter=0.05)
    return cfg, w, GnnGraph(w, cfg)


def _scan(seed, h, w, channels):
    """a synthetic scan, uint8 [h,w] or [h,w,3] (R, G, B, tinted differently per channel)"""
    from citlab_article_separation_new_amd import synth
    gray = synth.synth_page(seed, W=w, H=h).astype(np.float32)
    if channels == 1:
        return np.ascontiguousarray(gray.astype(np.uint8))
    rng = np.random.default_rng(seed)
    tint = np.array([0.35, 0.7, 1.0], np.float32)
    return np.ascontiguousarray(np.clip(gray[:, :, None] * tint + rng.random((h, w, 3), dtype=np.float32) * np.array([60, 30, 5], np.float32),
                                        0, 255).astype(np.uint8))


def _regions(rng, N, P=4):
    regions = np.zeros((N, 2, P), np.float32)
    npts = np.full(N, P, np.int32)
    for n in range(N):
        x0, y0 = rng.random() * 0.8, rng.random() * 0.8
        x1, y1 = x0 + 0.02 + rng.random() * 0.18, y0 + 0.01 + rng.random() * 0.1
        regions[n, 0] = [x0, x1, x1, x0]
        regions[n, 1] = [y0, y0, y1, y1]
    regions[0, 0, :] = [0.0, 1.0, 1.0, 0.0]                          # full page
    regions[0, 1, :] = [0.0, 0.0, 1.0, 1.0]
    npts[1] = 0                                                      # no points -> cell (0, 0)
    return regions, npts


def _graph_json(path, k, N, feature_dim=7):
    """a planted graph json with visual regions; feature_dim 15: the 7 features the nets read spread by synth.GNN_FEATURE_MASK"""
    from citlab_article_separation_new_amd import synth
    g = synth.synth_graph(k, N=N, n_pairs=4 * N, node_dim=7)
    feats = g["node_features"]
    if feature_dim == 15:
        feats = np.zeros((N, 15), np.float32)
        feats[:, [i for i, m in enumerate(synth.GNN_FEATURE_MASK) if m]] = g["node_features"]
    regions, npts = _regions(np.random.default_rng(k), N)
    with open(path, "w") as f:
        json.dump({"num_nodes": N, "interacting_nodes": g["interacting_nodes"].tolist(), "num_interacting_nodes": int(g["interacting_nodes"].shape[0]),
                   "node_features": feats.tolist(), "edge_features": g["edge_features"].tolist(), "gt_relations": [], "gt_num_relations": 0,
                   "visual_regions_nodes": regions.tolist(), "num_points_visual_regions_nodes": npts.tolist()}, f)


class _Flags:
    image_input = True

    def __init__(self, **input_params):
        self.input_params = dict(node_feature_dim=7, edge_feature_dim=2, **input_params)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# (scan H x W, resize_min_dim, resize_max_dim): 97 x 131 is scaled down; 150 x 101 with resize_min_dim above its short side is scaled up
SCANS = {"down": ((97, 131), 64, 96), "up": ((150, 101), 128, 1024)}


@pytest.mark.parametrize("scan", sorted(SCANS))
@pytest.mark.parametrize("channels", [1, 3], ids=["gray", "rgb"])
def test_session_fed_the_uint8_scan_equals_the_session_fed_the_host_resize(channels, scan, tmp_path):
    from citlab_article_separation_new_amd import gnn_input, gnn_io
    (H, W), lo, hi = SCANS[scan]
    _, _, graph = _setup(channels)
    try:
        page = _scan(3, H, W, channels)
        _graph_json(tmp_path / "g.json", 1, 24)
        fn = gnn_input.InputGNN(_Flags(load_mode="L" if channels == 1 else "RGB", resize_min_dim=lo, resize_max_dim=hi))
        host = fn.feed_from_json(str(tmp_path / "g.json"), page)
        dev = fn.feed_from_json(str(tmp_path / "g.json"), page, device_resize=True)
        assert "image:0" in host and "image_u8:0" not in host and "image_u8:0" in dev and "image:0" not in dev
        nh, nw = gnn_input.compute_new_size(H, W, lo, hi)
        assert (nh > H) == (scan == "up") and host["image:0"].shape == (1, nh, nw, channels)
        assert dev["image_shape:0"].tolist() == [[nh, nw, channels]]
        sess = gnn_io.GnnSession(graph, "0")
        want = sess.run(OUTPUT, host)
        got = sess.run(OUTPUT, dev)
        assert got.shape == (1, 24 * 24, 2) and np.isfinite(got).all()
        assert _bits_equal(got, want)
        if channels == 1:                                    # [1,H,W,1] is the same scan
            dev["image_u8:0"] = dev["image_u8:0"][..., None]
            assert _bits_equal(sess.run(OUTPUT, dev), want)
    finally:
        graph.close()


def test_colour_scan_into_the_gray_backbone_equals_pillows_gray_resized_on_the_host(tmp_path):
    from PIL import Image
    from citlab_article_separation_new_amd import gnn_input, gnn_io
    _, _, graph = _setup(1)
    try:
        page = _scan(5, 97, 131, 3)
        gray = np.asarray(Image.fromarray(page, "RGB").convert("L"))
        _graph_json(tmp_path / "g.json", 2, 17)
        fn = gnn_input.InputGNN(_Flags(load_mode="L", resize_min_dim=64, resize_max_dim=96))
        host = fn.feed_from_json(str(tmp_path / "g.json"), gray)
        dev = fn.feed_from_json(str(tmp_path / "g.json"), page, device_resize=True)
        assert dev["image_u8:0"].shape == (1, 97, 131, 3) and dev["image_shape:0"][0, 2] == 1      # one channel is fed
        sess = gnn_io.GnnSession(graph, "0")
        want = sess.run(OUTPUT, host)
        assert _bits_equal(sess.run(OUTPUT, dev), want)
        # the function beside gnn_forward_visual, called without the session
        a = {k: v[0] for k, v in dev.items()}
        rel = a["relations_to_consider_belong_to_same_instance:0"]
        probs = gnn_io.gnn_forward_visual_u8(graph, 17, a["interacting_nodes:0"], a["node_features:0"], a["edge_features:0"], page,
                                             int(a["image_shape:0"][0]), int(a["image_shape:0"][1]), a["visual_regions_nodes:0"],
                                             a["num_points_visual_regions_nodes:0"], rel)
        assert _bits_equal(probs, want[0])
    finally:
        graph.close()


def test_gray_scan_into_the_colour_backbone_and_both_image_feeds_are_refused(tmp_path):
    from citlab_article_separation_new_amd import gnn_input, gnn_io
    _, _, colour = _setup(3)
    try:
        _graph_json(tmp_path / "g.json", 3, 9)
        fn = gnn_input.InputGNN(_Flags(load_mode="L", resize_min_dim=64, resize_max_dim=96))
        sess = gnn_io.GnnSession(colour, "0")
        for page in (_scan(1, 40, 52, 1), _scan(1, 40, 52, 1)[:, :, None]):
            dev = fn.feed_from_json(str(tmp_path / "g.json"), page, device_resize=True)
            with pytest.raises(ValueError, match=r"takes 3 image channel\(s\).*has 1"):
                sess.run(OUTPUT, dev)
        both = fn.feed_from_json(str(tmp_path / "g.json"), _scan(1, 40, 52, 1))
        both.update(fn.image_feeds(_scan(1, 40, 52, 1), device_resize=True))
        assert "image:0" in both and "image_u8:0" in both
        with pytest.raises(KeyError, match="both image:0 and image_u8:0"):
            sess.run(OUTPUT, both)
    finally:
        colour.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _write_page_xml(path, n_regions, W, H):
    regs = []
    for i in range(n_regions):
        x, y = 10 + (i % 5) * 50, 10 + (i // 5) * 30
        regs.append(f'<TextRegion id="tr{i}"><Coords points="{x},{y} {x+40},{y} {x+40},{y+20} {x},{y+20}"/>'
                    f'<TextLine id="tr{i}l0"><Coords points="{x},{y} {x+40},{y} {x+40},{y+10} {x},{y+10}"/></TextLine>'
                    f'<TextLine id="tr{i}l1"><Coords points="{x},{y+10} {x+40},{y+10} {x+40},{y+20} {x},{y+20}"/></TextLine></TextRegion>')
    path.write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/'
                    'pagecontent/2013-07-15"><Metadata><Creator>t</Creator><Created>2020-01-01T00:00:00</Created>'
                    '<LastChange>2020-01-01T00:00:00</LastChange></Metadata><Page imageFilename="x.png" '
                    f'imageWidth="{W}" imageHeight="{H}">' + "".join(regs) + '</Page></PcGts>')


def _cli_inputs(root, backbone_channels, scan_channels):
    """a frozen relation graph + three synthetic pages (scan png, graph json, PAGE-XML) -> argv without --out_dir / --device_resize"""
    from PIL import Image
    from citlab_article_separation_new_amd import pb_import, synth
    cfg, w, graph = _setup(backbone_channels, seed=23)
    graph.close()
    model = root / "model" / "export"
    model.mkdir(parents=True)
    extra = [{"name": "graph/map/per_image_standardization/Mean", "op": "Mean"}]
    (model / "gnn_best_1.pb").write_bytes(pb_import.weights_to_graphdef(w, "graph/", extra, meta={"num_transition_steps": cfg.num_transition_steps}))
    data = root / "data"
    (data / "page").mkdir(parents=True)
    (data / "json15d2bb").mkdir()
    H, W = 150, 110
    jsons = []
    for k, N in enumerate((20, 12, 16)):
        name = f"p{k}"
        page = _scan(30 + k, H, W, scan_channels)
        Image.fromarray(page, "L" if scan_channels == 1 else "RGB").save(str(data / f"{name}.png"))
        _graph_json(data / "json15d2bb" / f"{name}.json", 60 + k, N, feature_dim=15)
        _write_page_xml(data / "page" / f"{name}.xml", N, W, H)
        jsons.append(str(data / "json15d2bb" / f"{name}.json"))
    (root / "eval.lst").write_text("\n".join(jsons) + "\n")
    return ["--model_dir", str(root / "model"), "--eval_list", str(root / "eval.lst"), "--clustering_method", "dbscan", "--image_input", "True",
            "--visual_layers", *LAYERS, "--gpu_devices", "0", "--save_conf", "with_conf", "--input_params", "node_feature_dim=15",
            "edge_feature_dim=2", "node_input_feature_mask=" + str(synth.GNN_FEATURE_MASK).replace(" ", ""),
            "load_mode=" + ("L" if backbone_channels == 1 else "RGB")]


def _files(root, out_dir):
    """{relative path: bytes} of the clustering PAGE-XMLs under ``out_dir`` and the confidence jsons beside the data (LastChange's
    text blanked: see the module docstring)"""
    found = {}
    for top in (root / out_dir, root / "data" / "confidences"):
        for dirpath, _, names in os.walk(top):
            for n in names:
                p = os.path.join(dirpath, n)
                with open(p, "rb") as f:
                    raw = f.read()
                if n.endswith(".xml"):
                    raw = re.sub(rb"(<(?:\w+:)?LastChange>)[^<]*(</)", rb"\1\2", raw)
                found[os.path.relpath(p, top)] = raw
    return found


def _run_both_ways(root, argv, extra=()):
    from citlab_article_separation_new_amd import run_gnn_clustering
    cwd = os.getcwd()
    os.chdir(root)
    got = {}
    try:
        for flag in ("True", "False"):
            for f in (root / "data" / "confidences").glob("*.json") if (root / "data" / "confidences").is_dir() else ():
                f.unlink()
            outs = run_gnn_clustering.main(argv + ["--out_dir", "out_" + flag, "--device_resize", flag, *extra])
            assert len(outs) == 3
            got[flag] = _files(root, "out_" + flag)
    finally:
        os.chdir(cwd)
    assert sorted(got["True"]) == sorted(got["False"])
    assert sum(k.endswith("_clustering.xml") for k in got["True"]) == 3 and sum(k.endswith("_confidences.json") for k in got["True"]) == 3
    for k in got["True"]:
        assert got["True"][k] == got["False"][k], k


CLI_CASES = {"gray_png": (1, 1), "colour_png_RGB": (3, 3), "colour_png_L": (1, 3)}     # (backbone channels, scan channels)


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_command_line_writes_the_same_bytes_with_and_without_device_resize(case, tmp_path):
    _run_both_ways(tmp_path, _cli_inputs(tmp_path, *CLI_CASES[case]))


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_pipelined_command_line_writes_the_same_bytes_with_and_without_device_resize(case, tmp_path):
    """--num_workers 3: with --device_resize the scans reach the owner through DecodePool's shared-memory slots"""
    _run_both_ways(tmp_path, _cli_inputs(tmp_path, *CLI_CASES[case]), ("--num_workers", "3"))
