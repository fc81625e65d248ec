"""Host side of --device_resize (no GPU): what ``feed_from_json`` puts into the feed, the flag, and the DecodePool page loaders against the
decode ``run_gnn_clustering._prepare_feed`` does."""
import json

import numpy as np
import pytest


class _Flags:
    image_input = True

    def __init__(self, **input_params):
        self.input_params = dict(node_feature_dim=4, **input_params)


def _json(path, N=3):
    regions = np.tile(np.array([[0.1, 0.4, 0.4, 0.1], [0.2, 0.2, 0.3, 0.3]], np.float32), (N, 1, 1))
    path.write_text(json.dumps({"num_nodes": N, "interacting_nodes": [[0, 1], [1, 2]], "num_interacting_nodes": 2,
                                "node_features": np.arange(N * 4, dtype=np.float32).reshape(N, 4).tolist(), "edge_features": [],
                                "gt_relations": [], "gt_num_relations": 0, "visual_regions_nodes": regions.tolist(),
                                "num_points_visual_regions_nodes": [4] * N}))
    return str(path)


@pytest.mark.parametrize("load_mode,shape,fed", [("L", (97, 131), 1), ("L", (97, 131, 1), 1), ("L", (97, 131, 3), 1), ("RGB", (97, 131, 3), 3)])
def test_device_resize_feeds_the_untouched_page_and_the_target_shape(load_mode, shape, fed, tmp_path):
    from citlab_article_separation_new_amd import gnn_input
    page = np.random.default_rng(1).integers(0, 256, size=shape, dtype=np.uint8)
    fn = gnn_input.InputGNN(_Flags(load_mode=load_mode, resize_min_dim=64, resize_max_dim=96))
    feed = fn.feed_from_json(_json(tmp_path / "g.json"), page, device_resize=True)
    assert "image:0" not in feed
    got = feed["image_u8:0"]
    assert got.dtype == np.uint8 and got.shape == (1,) + shape and np.shares_memory(got, page) and np.array_equal(got[0], page)
    nh, nw = gnn_input.compute_new_size(97, 131, 64, 96)
    assert feed["image_shape:0"].dtype == np.int32 and feed["image_shape:0"].tolist() == [[nh, nw, fed]]
    assert feed["visual_regions_nodes:0"].shape == (1, 3, 2, 4) and feed["num_points_visual_regions_nodes:0"].tolist() == [[4, 4, 4]]
    # the json half alone (the scan follows through a decode slot), completed by image_feeds, is the same feed
    later = fn.feed_from_json(_json(tmp_path / "g.json"), None, device_resize=True, image_later=True)
    assert "image_u8:0" not in later and "image_shape:0" not in later and "visual_regions_nodes:0" in later
    later.update(fn.image_feeds(page, device_resize=True))
    assert sorted(later) == sorted(feed) and all(np.array_equal(later[k], feed[k]) for k in feed)


def test_device_resize_refuses_what_is_not_a_decoded_scan(tmp_path):
    from citlab_article_separation_new_amd import gnn_input
    with pytest.raises(ValueError, match="uint8"):
        gnn_input.InputGNN(_Flags()).feed_from_json(_json(tmp_path / "g.json"), np.zeros((8, 9), np.float32), device_resize=True)
    with pytest.raises(ValueError, match="load_mode=RGB feeds"):
        gnn_input.InputGNN(_Flags(load_mode="RGB")).feed_from_json(_json(tmp_path / "g.json"), np.zeros((8, 9), np.uint8), device_resize=True)


def test_default_call_is_the_host_resize_as_before(tmp_path):
    from citlab_article_separation_new_amd import gnn_input
    page = np.random.default_rng(2).integers(0, 256, size=(97, 131), dtype=np.uint8)
    fn = gnn_input.InputGNN(_Flags(resize_min_dim=64, resize_max_dim=96))
    feed = fn.feed_from_json(_json(tmp_path / "g.json"), page)
    nh, nw = gnn_input.compute_new_size(97, 131, 64, 96)
    assert "image_u8:0" not in feed and feed["image:0"].dtype == np.float32 and feed["image:0"].shape == (1, nh, nw, 1)
    assert np.array_equal(feed["image:0"][0], gnn_input.resize_bilinear_tf1(page, nh, nw))
    assert feed["image_shape:0"].tolist() == [[nh, nw, 1]]
    assert sorted(feed) == sorted(["num_nodes:0", "num_interacting_nodes:0", "interacting_nodes:0", "node_features:0", "image:0", "image_shape:0",
                                   "visual_regions_nodes:0", "num_points_visual_regions_nodes:0", "relations_to_consider_belong_to_same_instance:0"])
    no_image = fn.feed_from_json(_json(tmp_path / "g.json"))
    assert "image:0" not in no_image and "visual_regions_nodes:0" not in no_image


def test_the_flag_parses_and_defaults_to_the_host_resize():
    """the default is the host resize until the device path is no slower on every measured leg"""
    from citlab_article_separation_new_amd import lav_rel, run_gnn_clustering
    for parse in (lambda a: run_gnn_clustering.build_parser().parse_known_args(a)[0], lav_rel.parse_flags):
        assert parse([]).device_resize is False
        assert parse(["--device_resize", "False"]).device_resize is False
        assert parse(["--device_resize", "True"]).device_resize is True


def _files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    gray = rng.integers(0, 256, size=(37, 53), dtype=np.uint8)
    colour = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    Image.fromarray(gray, "L").save(str(tmp_path / "gray.png"))
    Image.fromarray(colour, "RGB").save(str(tmp_path / "colour.png"))
    Image.fromarray(colour, "RGB").save(str(tmp_path / "colour.jpg"), quality=90)
    Image.fromarray(colour, "RGB").convert("P").save(str(tmp_path / "palette.png"))
    return {n: str(tmp_path / n) for n in ("gray.png", "colour.png", "colour.jpg", "palette.png")}, gray, colour


def _prepare_feed_decode(monkeypatch, path, load_mode, device_resize):
    """the page ``run_gnn_clustering._prepare_feed`` hands to ``feed_from_json`` for the scan at ``path``"""
    from citlab_article_separation_new_amd import gnn_input, path_util, run_gnn_clustering
    seen = {}

    class Fn:
        input_params = {"load_mode": load_mode}
        img_channels = gnn_input.LOAD_MODE_CHANNELS[load_mode]

        def feed_from_json(self, json_path, image, targets, **kw):
            seen["image"], seen["kw"] = image, kw
            return {"num_nodes:0": np.array([1], np.int32)}

    class Flags:
        image_input = True
    Flags.device_resize = device_resize
    monkeypatch.setattr(path_util, "get_img_from_json_path", lambda p: path)
    run_gnn_clustering._prepare_feed(Fn(), Flags(), "unused.json")
    assert seen["kw"]["device_resize"] is device_resize
    return seen["image"]


@pytest.mark.parametrize("name", ["gray.png", "colour.png", "colour.jpg", "palette.png"])
def test_decode_pool_loaders_return_what_prepare_feed_decodes(name, tmp_path, monkeypatch):
    from PIL import Image
    from citlab_article_separation_new_amd import host_pipeline
    files, _, _ = _files(tmp_path)
    path = files[name]
    with Image.open(path) as im:
        pil_l, pil_rgb, plain = np.asarray(im.convert("L")), np.asarray(im.convert("RGB")), im.mode in ("L", "RGB")
        pil_mode = im.mode
    for load_mode, device_resize in (("L", False), ("L", True), ("RGB", False), ("RGB", True)):
        loader = host_pipeline._resolve_loader(host_pipeline.page_loader_name(load_mode, device_resize))
        got = loader(path)
        want = _prepare_feed_decode(monkeypatch, path, load_mode, device_resize)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (name, load_mode, device_resize)
        if load_mode == "RGB":
            assert np.array_equal(got, pil_rgb)                              # Pillow semantics
        elif not device_resize or not (plain and pil_mode == "RGB"):
            assert np.array_equal(got, pil_l)
        else:                                                                # a plain colour scan stays R, G, B: the kernel takes the luma
            assert np.array_equal(got, pil_rgb)
            luma = (got[:, :, 0].astype(np.uint32) * 19595 + got[:, :, 1].astype(np.uint32) * 38470 + got[:, :, 2].astype(np.uint32) * 7471 + 0x8000) >> 16
            assert np.array_equal(luma.astype(np.uint8), pil_l)


def test_decode_pool_hands_out_pages_of_the_page_loaders_in_order(tmp_path):
    """inline pool (no worker processes): the loader names resolve and the list order is kept"""
    from citlab_article_separation_new_amd import gnn_input, host_pipeline
    files, gray, colour = _files(tmp_path)
    paths = [files["colour.png"], files["gray.png"], files["colour.png"]]
    pages = list(host_pipeline.DecodePool(paths, 0, loader=host_pipeline.page_loader_name("L", True)))
    assert [p for p, _ in pages] == paths
    assert np.array_equal(pages[0][1], colour) and np.array_equal(pages[1][1], gray) and np.array_equal(pages[2][1], colour)
    assert np.array_equal(gnn_input.load_page(paths[0], "L", False), gnn_input.load_page_gray(paths[0]))
