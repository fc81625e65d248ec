"""Colour (RGB) page input, the host side: frozen RU / U graphs whose first convolution reads three channels import with ``channels == 3`` and
an ARU graph with three channels is refused with the reason (ARU_v1.py:115); ``InputGNN`` honours ``load_mode`` (input_dataset.py:42-49, :279:
Pillow's ``convert('RGB')``, R, G, B order, every channel resized like a gray page) and leaves ``load_mode=L`` as it was; ``load_mode`` against
the channels of a relation graph's backbone; and ``pack_first_rgb`` of csrc/aru_pack.h (shape check, TensorFlow's order kept, bfloat16 rounding
for the bf16 engine) against numpy, through
tests/aru_pack_rgb_check.cpp compiled with the host compiler under the address and undefined-behaviour sanitizers and run as a child process
(as tests/test_aru_pack_host.py does for the other packers)."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from citlab_article_separation_new_amd import gnn_input  # noqa: E402
from citlab_article_separation_new_amd.config import AruConfig, GnnConfig  # noqa: E402
from citlab_article_separation_new_amd.weights import init_aru_weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")


# ---- frozen graphs -----------------------------------------------------------------------------------------------------------------
def _frozen(cfg, seed=3):
    pytest.importorskip("google.protobuf")
    import tf_aru_graph
    from citlab_article_separation_new_amd import pb_import
    w = init_aru_weights(cfg, seed, bias_jitter=0.05, logit_scale=0.05)
    return w, pb_import.parse_graphdef(tf_aru_graph.build_aru_pb(w, cfg))


@pytest.mark.parametrize("graph", ["RU", "U"])
@pytest.mark.parametrize("mapper", ["aru_from_nodes", "aru_from_constants"])
def test_three_channel_ru_and_u_graphs_import_with_channels_3(graph, mapper):
    from citlab_article_separation_new_amd import pb_import
    cfg = AruConfig(graph=graph, channels=3, scale_space_num=3)
    w, nodes = _frozen(cfg)
    tensors, got = getattr(pb_import, mapper)(nodes)
    assert got.channels == 3 and got.graph == graph and got.scale_space_num == 3
    first = "aru_net/featMapG/unet_down_0/conv1/weights"
    assert tensors[first].shape == (3, 3, 3, 8) and np.array_equal(tensors[first], w[first])
    got.check_channels()


@pytest.mark.parametrize("mapper", ["aru_from_nodes", "aru_from_constants"])
def test_three_channel_aru_graph_is_refused_with_the_reason(mapper):
    from citlab_article_separation_new_amd import pb_import
    cfg = AruConfig(graph="ARU", channels=3, scale_space_num=2, num_scales_att=2)
    _, nodes = _frozen(cfg)
    with pytest.raises(IOError, match=r"3 image channel.*without attention \(RU or U\).*one-channel filter \(ARU_v1\.py:115\)"):
        getattr(pb_import, mapper)(nodes)
    with pytest.raises(ValueError, match="without attention"):
        cfg.check_channels()
    with pytest.raises(ValueError, match="2 input channels"):
        AruConfig(graph="RU", channels=2).check_channels()
    AruConfig().check_channels()


# ---- InputGNN ------------------------------------------------------------------------------------------------------------------------
def _page_files(tmp_path, H=37, W=61):
    """a small colour png with three clearly different channels + a graph json beside it"""
    import json
    from PIL import Image
    rng = np.random.default_rng(5)
    rgb = np.stack([rng.integers(0, 80, (H, W)), rng.integers(90, 170, (H, W)), rng.integers(180, 256, (H, W))], axis=2).astype(np.uint8)
    img_path = str(tmp_path / "page.png")
    Image.fromarray(rgb, "RGB").save(img_path)
    n = 3
    data = {"num_nodes": n, "interacting_nodes": [[0, 1], [1, 2]], "num_interacting_nodes": 2,
            "node_features": rng.random((n, 4)).tolist(), "edge_features": [[0.5], [0.25]],
            "visual_regions_nodes": [[[0.1, 0.4], [0.1, 0.3]], [[0.5, 0.9], [0.2, 0.6]], [[0.3, 0.6], [0.6, 0.9]]],
            "num_points_visual_regions_nodes": [2, 2, 2]}
    json_path = str(tmp_path / "page.json")
    with open(json_path, "w") as f:
        json.dump(data, f)
    return rgb, img_path, json_path


def _flags(**input_params):
    return types.SimpleNamespace(input_params=input_params, image_input=True)


def test_input_gnn_load_mode_rgb_feeds_r_g_b_each_resized_like_a_gray_page(tmp_path):
    rgb, img_path, json_path = _page_files(tmp_path)
    params = dict(resize_min_dim=48, resize_max_dim=64)
    fn = gnn_input.InputGNN(_flags(load_mode="RGB", **params))
    assert fn.img_channels == 3
    nh, nw = gnn_input.compute_new_size(rgb.shape[0], rgb.shape[1], 48, 64)
    assert (nh, nw) != rgb.shape[:2]
    loaded = gnn_input.load_page_rgb(img_path)
    assert loaded.dtype == np.uint8 and np.array_equal(loaded, rgb)                   # R, G, B: not the B, G, R of image_io's decode
    for image in (loaded, rgb.astype(np.float32)):                                   # the decoded page, uint8 or float32
        feed = fn.feed_from_json(json_path, image)
        assert feed["image:0"].shape == (1, nh, nw, 3) and feed["image:0"].dtype == np.float32
        assert feed["image_shape:0"].tolist() == [[nh, nw, 3]]
        for c in range(3):
            alone = gnn_input.resize_bilinear_tf1(rgb[:, :, c], nh, nw)
            assert np.array_equal(feed["image:0"][0, :, :, c], alone[:, :, 0]), c
        means = feed["image:0"][0].mean(axis=(0, 1))
        assert means[0] < 80 < means[1] < 180 < means[2]                              # channel 0 is the dark red plane
    with pytest.raises(ValueError, match="RGB"):
        fn.feed_from_json(json_path, rgb[:, :, 0])
    with pytest.raises(ValueError, match="load_mode"):
        gnn_input.InputGNN(_flags(load_mode="CMYK"))


def test_input_gnn_load_mode_l_is_unchanged_on_the_same_file(tmp_path):
    from PIL import Image
    rgb, img_path, json_path = _page_files(tmp_path)
    params = dict(resize_min_dim=48, resize_max_dim=64)
    with Image.open(img_path) as im:
        gray = np.asarray(im.convert("L"))
    nh, nw = gnn_input.compute_new_size(gray.shape[0], gray.shape[1], 48, 64)
    want = gnn_input.resize_bilinear_tf1(gray, nh, nw)[None]
    for flags in (_flags(**params), _flags(load_mode="L", **params)):
        fn = gnn_input.InputGNN(flags)
        assert fn.img_channels == 1
        feed = fn.feed_from_json(json_path, gray)
        assert feed["image:0"].shape == (1, nh, nw, 1) and np.array_equal(feed["image:0"], want)
        assert feed["image_shape:0"].tolist() == [[nh, nw, 1]]
    # the command line's own loader (run_gnn_clustering._prepare_feed) gives the same gray feed as before, and the colour one under RGB
    from citlab_article_separation_new_amd import run_gnn_clustering
    feeds = {}
    for mode in ("L", "RGB"):
        fl = _flags(load_mode=mode, **params)
        feeds[mode], n = run_gnn_clustering._prepare_feed(gnn_input.InputGNN(fl), fl, _json_beside_scan(tmp_path, json_path, img_path))
        assert n == 3
    assert np.array_equal(feeds["L"]["image:0"], want)
    assert feeds["RGB"]["image:0"].shape == (1, nh, nw, 3)
    assert np.array_equal(feeds["RGB"]["image:0"][0, :, :, 2], gnn_input.resize_bilinear_tf1(rgb[:, :, 2], nh, nw)[:, :, 0])


def _json_beside_scan(tmp_path, json_path, img_path):
    """the layout get_img_from_json_path expects: <dir>/page.png, <dir>/json<suffix>/page.json"""
    from citlab_article_separation_new_amd.path_util import get_img_from_json_path
    d = tmp_path / "json"
    d.mkdir(exist_ok=True)
    target = str(d / "page.json")
    if not os.path.exists(target):
        shutil.copy(json_path, target)
    assert os.path.samefile(get_img_from_json_path(target), img_path)
    return target


def test_load_mode_against_the_backbone_channels():
    rgb_graph = GnnConfig(visual_dims=[4], visual_layers=["scale_0_unet_up_0_conv"], backbone={"channels": 3, "scale_space_num": 2})
    gray_graph = GnnConfig(visual_dims=[4], visual_layers=["scale_0_unet_up_0_conv"], backbone={"scale_space_num": 2})
    gnn_input.check_load_mode({"load_mode": "RGB"}, rgb_graph)
    gnn_input.check_load_mode({}, gray_graph)
    gnn_input.check_load_mode({"load_mode": "RGB"}, GnnConfig())                       # no visual branch: no image is fed
    with pytest.raises(ValueError, match=r"load_mode=L feeds 1 image channel\(s\), the graph's backbone reads 3"):
        gnn_input.check_load_mode({}, rgb_graph)
    with pytest.raises(ValueError, match=r"load_mode=RGB feeds 3 image channel\(s\), the graph's backbone reads 1"):
        gnn_input.check_load_mode({"load_mode": "RGB"}, gray_graph)


# ---- pack_first_rgb -----------------------------------------------------------------------------------------------------------------
def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def _bf16_round(a):
    """round to nearest even to bfloat16, as float32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def test_pack_first_rgb_keeps_the_order_rounds_for_bf16_and_refuses_other_shapes(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path / "aru_pack_rgb_check")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), "-I", CSRC, os.path.join(ROOT, "tests", "aru_pack_rgb_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-4000:]
    lines = ran.stdout.splitlines()
    assert lines[-1] == "aru pack rgb ok"
    packed, refused = {}, {}
    for line in lines[:-1]:
        t = line.split(" ", 3)
        if t[0] == "P":
            vals = np.array([int(x, 16) for x in t[3].split()], np.uint32).view(np.float32)
            assert len(vals) == int(t[2])
            packed[t[1]] = vals
        else:
            assert t[0] == "R"
            refused[t[1]] = (int(t[2]), t[3])
    assert sorted(packed) == ["c16", "c16_bf16", "c8", "c8_bf16"]
    for cout in (8, 16):
        w = (np.arange(1, 27 * cout + 1, dtype=np.float32) * np.float32(1.001)).reshape(3, 3, 3, cout)     # TensorFlow's [ky][kx][ci][co]
        # conv_c3_kernel reads [ky][kx][ci][co] as it is: the nine values [kx][ci] of a filter row beside the nine interleaved values of a window row
        want = np.stack([np.stack([w[ky, j // 3, j % 3] for j in range(9)]) for ky in range(3)]).reshape(-1)
        assert np.array_equal(want, w.reshape(-1))
        assert np.array_equal(packed[f"c{cout}"], want)
        assert np.array_equal(packed[f"c{cout}_bf16"], _bf16_round(want))
        assert not np.array_equal(packed[f"c{cout}_bf16"], want)
    ERR_WEIGHTS, ERR_UNSUPPORTED = -3, -4                                            # include/asep_hip.h
    codes = {k: v[0] for k, v in refused.items()}
    assert codes == {"gray": ERR_UNSUPPORTED, "four_channels": ERR_UNSUPPORTED, "cout12": ERR_UNSUPPORTED, "k4": ERR_UNSUPPORTED,
                     "rank3": ERR_UNSUPPORTED, "bias": ERR_WEIGHTS}
    assert all("[3,3,3,8] or [3,3,3,16]" in refused[k][1] for k in ("gray", "four_channels", "cout12", "k4", "rank3"))
    assert "bias has 7 elements, expected 8" in refused["bias"][1]
