"""asep_gnn_forward_visual_batch_dev2: the visual relation net over pages of DIFFERENT image sizes in one call, against the single-page
entry asep_gnn_forward_visual_dev on the same handle.  The batched stages run the single-page kernels' bodies over a page table, so
everything is compared bit for bit (np.array_equal on the float bits): probabilities, concatenated node features and every feature map,
page by page (asep_gnn_get_page_node_features / asep_gnn_get_page_feature_map).

Shapes: four pages of 64 x 96, 96 x 64, 71 x 53 (odd both ways: the stride-2 maps and the pools get remainders) and 128 x 80 with N = 2, 3,
30 and 17 nodes; one page without interactions, every page with a region that clamps to the last cell, two pages with all N * N pairs asked
for by a NULL list and two with an explicit list.  The bf16 backbone gets sizes of at least 64 both ways (the open
fault of the bf16 engine on pages whose level-3 maps are one row high).

uint8 scans (asep_gnn_forward_visual_batch_u8_dev): sources of 300 x 200, 211 x 333 and 256 x 256 resized in one launch; the resized bytes and
the probabilities against the single-page u8 path (asep_prep_resize_tf1_dev + asep_gnn_forward_visual_dev)."""
import ctypes as C
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(64, 96), (96, 64), (71, 53), (128, 80)]
SIZES_BF16 = [(64, 96), (96, 64), (72, 64), (128, 80)]
NODES = [2, 3, 30, 17]
UP1 = "scale_0_unet_up_1_conv"
THREE = ("scale_0_unet_up_2_conv", UP1, "scale_0_unet_up_0_conv")
# name -> (GnnConfig keywords, page sizes)
VARIANTS = {
    "aru_gray": (dict(visual_layers=list(THREE), visual_dims=[8, 4, 4], backbone={"graph": "ARU"}), SIZES),
    "ru_rgb": (dict(visual_layers=list(THREE), visual_dims=[8, 4, 4], backbone={"channels": 3}), SIZES),
    "fmaps": (dict(visual_layers=[UP1, "", ""], visual_layer_depths=[-1, 6, 2], visual_dims=[8, 4, 4]), SIZES),
    "visual_edges": (dict(visual_layers=list(THREE), visual_dims=[8, 4, 4], visual_edges=True), SIZES),
    "fmaps_visual_edges": (dict(visual_layers=[UP1, "", ""], visual_layer_depths=[-1, 6, 2], visual_dims=[8, 4, 4], visual_edges=True), SIZES),
    "bf16": (dict(visual_layers=list(THREE), visual_dims=[8, 4, 4], backbone={"compute_dtype": "bf16"}), SIZES_BF16),
}
P = 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _host_pages(cfg, sizes, seed=17, nodes=NODES):
    """numpy inputs of the pages: a different image, graph and region set each"""
    from citlab_article_separation_new_amd import synth
    rng = np.random.default_rng(seed)
    chans = cfg.backbone_cfg().channels
    pages = []
    for b, ((h, w), N) in enumerate(zip(sizes, nodes)):
        E = 0 if b == 1 else 3 * N                                   # page 1: no interactions
        edges = rng.integers(0, N, size=(E, 2)).astype(np.int32)
        img = synth.synth_page(20 + b, W=w, H=h).astype(np.float32)
        if chans == 3:
            img = np.ascontiguousarray(img[:, :, None] * np.array([0.35, 0.7, 1.0], np.float32) + rng.random((h, w, 3), dtype=np.float32) * 20)
        regions = np.zeros((N, 2, P), np.float32)
        for n in range(N):
            x0, y0 = rng.random() * 0.8, rng.random() * 0.8
            x1, y1 = x0 + 0.02 + rng.random() * 0.18, y0 + 0.01 + rng.random() * 0.1
            regions[n, 0] = [x0, x1, x1, x0]
            regions[n, 1] = [y0, y0, y1, y1]
        regions[0, 0, :] = [0.0, 1.0, 1.0, 0.0]                      # x = y = 1.0: floor(1.0 * fw) = fw clamps to the last cell
        regions[0, 1, :] = [0.0, 0.0, 1.0, 1.0]
        npts = np.full(N, P, np.int32)
        npts[1:2] = 0                                                # no points -> cell (0, 0)
        eregions = np.zeros((E, 2, P), np.float32)
        for e, (i, j) in enumerate(edges):
            x0, x1 = min(regions[i, 0].min(), regions[j, 0].min()), max(regions[i, 0].max(), regions[j, 0].max())
            y0, y1 = min(regions[i, 1].min(), regions[j, 1].min()), max(regions[i, 1].max(), regions[j, 1].max())
            eregions[e, 0] = [x0, x1, x1, x0]
            eregions[e, 1] = [y0, y0, y1, y1]
        enpts = np.full(E, P, np.int32)
        enpts[::5] = 0
        rel = None if b % 2 == 0 else np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing="ij"), -1).reshape(-1, 2).astype(np.int32)
        pages.append(dict(N=N, E=E, h=h, w=w, edges=edges, u=rng.standard_normal((N, cfg.node_feature_dim)).astype(np.float32),
                          ef=rng.standard_normal((E, 2)).astype(np.float32), img=img, regions=regions, npts=npts,
                          eregions=eregions if cfg.visual_edges else None, enpts=enpts if cfg.visual_edges else None, rel=rel))
    return pages


def _upload(page, num_classes=2):
    """-> (tensors kept alive, the fields of asep_gnn_page)"""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None and a.size else None      # noqa: E731
    ptr = lambda t: t.data_ptr() if t is not None else None                                                    # noqa: E731
    t = {k: up(page[k]) for k in ("edges", "u", "ef", "img", "regions", "npts", "eregions", "enpts", "rel")}
    t["out"] = torch.zeros(page["N"] * page["N"], num_classes, device="cuda")
    q = dict(N=page["N"], E=page["E"], R=page["N"] ** 2, d_edges=ptr(t["edges"]), d_node_feat=ptr(t["u"]), d_edge_feat=ptr(t["ef"]),
             d_image=ptr(t["img"]), d_regions=ptr(t["regions"]), d_num_points=ptr(t["npts"]), d_edge_regions=ptr(t["eregions"]),
             d_edge_num_points=ptr(t["enpts"]), d_relations=ptr(t["rel"]), d_probs_out=t["out"].data_ptr())
    return t, q


def _single(graph, t, q, h, w, n_maps):
    """one page through asep_gnn_forward_visual_dev -> (probabilities, node features, feature maps)"""
    import torch
    from citlab_article_separation_new_amd import gnn_io
    t["out"].zero_()
    gnn_io.gnn_forward_visual_dev(graph, q["N"], q["E"], q["d_edges"], q["d_node_feat"], q["d_edge_feat"], q["d_image"], h, w, q["d_regions"], P,
                                  q["d_num_points"], q["R"], q["d_relations"], q["d_probs_out"], None, 0, d_edge_regions=q["d_edge_regions"],
                                  d_edge_num_points=q["d_edge_num_points"])
    torch.cuda.synchronize()
    return t["out"].cpu().numpy(), gnn_io.gnn_node_features(graph, q["N"]), [gnn_io.gnn_feature_map(graph, i) for i in range(n_maps)]


class _Case:
    """a model, its four pages in HBM and the single-page results, computed once per variant and left unchanged"""

    def __init__(self, name):
        from citlab_article_separation_new_amd.config import GnnConfig
        from citlab_article_separation_new_amd.gnn_io import GnnGraph
        from citlab_article_separation_new_amd.weights import init_gnn_weights
        kw, sizes = VARIANTS[name]
        self.cfg = GnnConfig(node_feature_dim=7, mvn=True, **kw)
        self.graph = GnnGraph(init_gnn_weights(self.cfg, 11, bias_jitter=0.05), self.cfg)
        self.sizes = sizes
        self.host = _host_pages(self.cfg, sizes)
        self.dev = [_upload(p, self.cfg.num_classes) for p in self.host]
        self.n_maps = len(self.cfg.visual_layers)
        self.singles = [_single(self.graph, t, q, h, w, self.n_maps) for (t, q), (h, w) in zip(self.dev, sizes)]

    def batch(self, order=None):
        """one dev2 call over the pages in `order` -> per page (probabilities, node features, feature maps), in that order"""
        import torch
        from citlab_article_separation_new_amd import gnn_io
        order = list(range(len(self.dev))) if order is None else list(order)
        for b in order:
            self.dev[b][0]["out"].zero_()
        gnn_io.gnn_forward_visual_batch_dev2(self.graph, [self.dev[b][1] for b in order], [self.sizes[b][0] for b in order],
                                             [self.sizes[b][1] for b in order], P)
        torch.cuda.synchronize()
        got = []
        for k, b in enumerate(order):
            got.append((self.dev[b][0]["out"].cpu().numpy(), gnn_io.gnn_page_node_features(self.graph, k, self.host[b]["N"]),
                        [gnn_io.gnn_page_feature_map(self.graph, k, i) for i in range(self.n_maps)]))
        return got


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Case(name)
        return made[name]
    yield get
    for c in made.values():
        c.graph.close()


def _assert_pages_equal(got, want, label):
    for b, ((p, u, maps), (p0, u0, maps0)) in enumerate(zip(got, want)):
        assert np.isfinite(p0).all() and p0.shape[0] > 0, (label, b)
        assert _same(p, p0), (label, "probabilities of page", b, float(np.abs(p - p0).max()))
        assert _same(u, u0), (label, "node features of page", b)
        assert len(maps) == len(maps0)
        for i, (m, m0) in enumerate(zip(maps, maps0)):
            assert _same(m, m0), (label, "feature map", i, "of page", b, m.shape, m0.shape)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_mixed_sizes_in_one_call_equal_the_single_page_calls_bit_for_bit(variant, cases):
    c = cases(variant)
    if variant.startswith("fmaps"):                                   # d / 2 = 3 and 1; 71 x 53 -> odd maps under stride 2
        assert [m.shape[2] for m in c.singles[2][2]] == [c.cfg.visual_channels()[0], 6, 2]
    assert any((u[:, 7:] > 0).any() for _, u, _ in c.singles)        # the compression ReLU is not dead everywhere
    for _ in range(2):                                                # the second call reuses every arena
        _assert_pages_equal(c.batch(), c.singles, variant)


@pytest.mark.parametrize("variant", ["fmaps_visual_edges", "aru_gray"])
def test_reversed_page_order_gives_the_same_pages(variant, cases):
    c = cases(variant)
    order = [3, 2, 1, 0]
    _assert_pages_equal(c.batch(order), [c.singles[b] for b in order], variant + " reversed")


def test_eight_pages_in_one_call_on_two_backbone_lanes_equal_the_single_page_calls(cases):
    """eight pages: the grouped backbone forward deals them over two lanes (a lane takes at least four pages); the pages' statistics, end
    points and tables must follow the split"""
    import torch
    from citlab_article_separation_new_amd import gnn_io
    c = cases("fmaps_visual_edges")
    twice = [_upload(p, c.cfg.num_classes) for p in c.host]           # the same four pages again, with their own output buffers
    dev = c.dev + twice
    sizes = c.sizes + c.sizes
    for t, _ in dev:
        t["out"].zero_()
    gnn_io.gnn_forward_visual_batch_dev2(c.graph, [q for _, q in dev], [s[0] for s in sizes], [s[1] for s in sizes], P)
    torch.cuda.synchronize()
    got = [(t["out"].cpu().numpy(), gnn_io.gnn_page_node_features(c.graph, k, q["N"]), [gnn_io.gnn_page_feature_map(c.graph, k, i) for i in range(c.n_maps)])
           for k, (t, q) in enumerate(dev)]
    _assert_pages_equal(got, c.singles + c.singles, "eight pages")


def test_four_pages_of_one_size_equal_the_uniform_batch_entry(cases):
    import torch
    from citlab_article_separation_new_amd import gnn_io
    c = cases("fmaps_visual_edges")
    h, w = 71, 53
    host = _host_pages(c.cfg, [(h, w)] * 4, seed=5)
    dev = [_upload(p, c.cfg.num_classes) for p in host]
    gnn_io.gnn_forward_visual_batch_dev(c.graph, [q for _, q in dev], h, w, P)
    torch.cuda.synchronize()
    old = [t["out"].cpu().numpy() for t, _ in dev]
    for t, _ in dev:
        t["out"].zero_()
    gnn_io.gnn_forward_visual_batch_dev2(c.graph, [q for _, q in dev], [h] * 4, [w] * 4, P)
    torch.cuda.synchronize()
    for b, (t, _) in enumerate(dev):
        assert np.isfinite(old[b]).all() and _same(t["out"].cpu().numpy(), old[b]), b


@pytest.mark.parametrize("dtype,hw", [("f32", (71, 53)), ("bf16", (64, 96))])
def test_uniform_entry_with_visual_edges_over_stride_1_and_stride_2_maps_equals_the_single_page_calls(dtype, hw):
    """asep_gnn_forward_visual_batch_dev (pages of ONE size, page by page behind a grouped backbone) on a model with interaction visual
    features and a layout of an end point, a generated stride-1 map and a generated stride-2 map: three pages of N = 1, 3 and 4 nodes, the
    second without interactions, P = 4, against asep_gnn_forward_visual_dev bit for bit.  fp32: 71 x 53, the smallest page of this file with
    a generated stride-2 map; bf16: 64 x 96, the smallest of them that the bf16 backbone is given here (at least 64 both ways, see above).

    The uniform entry has no per-page read-back: asep_gnn_get_feature_map serves the LAST page of a call, asep_gnn_get_node_features the
    first N(last page) rows of the call's node features.  So the three pages go through the entry in their three rotations: every page is last
    once (its maps), the probabilities of every page are compared in every call, and the node-feature rows the read-back reaches are compared
    with the same rows of the single-page results one behind the other.  Row 3 of the four-node page is reached by no three-page call: that
    page also goes through the entry alone."""
    import torch
    from citlab_article_separation_new_amd import gnn_io
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    cfg = GnnConfig(node_feature_dim=7, mvn=True, visual_layers=[UP1, UP1, ""], visual_layer_depths=[-1, 6, 2], visual_dims=[8, 4, 4], visual_edges=True,
                    backbone={"compute_dtype": dtype})
    graph = gnn_io.GnnGraph(init_gnn_weights(cfg, 11, bias_jitter=0.05), cfg)
    h, w = hw
    host = _host_pages(cfg, [hw] * 3, seed=23, nodes=[1, 3, 4])
    assert [p["E"] for p in host] == [3, 0, 12]
    dev = [_upload(p, cfg.num_classes) for p in host]
    singles = [_single(graph, t, q, h, w, 3) for t, q in dev]
    assert [m.shape[2] for m in singles[2][2]] == [cfg.visual_channels()[0], 6, 2]
    assert singles[2][2][1].shape[:2] == singles[2][2][0].shape[:2] and singles[2][2][2].shape[0] == (singles[2][2][1].shape[0] + 1) // 2   # strides 1 and 2
    rows_seen = [0, 0, 0]
    for order in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [2]):
        for b in order:
            dev[b][0]["out"].zero_()
        gnn_io.gnn_forward_visual_batch_dev(graph, [dev[b][1] for b in order], h, w, P)
        torch.cuda.synchronize()
        for b in order:
            p0 = singles[b][0]
            assert np.isfinite(p0).all() and _same(dev[b][0]["out"].cpu().numpy(), p0), (dtype, order, "probabilities of page", b)
        last = order[-1]
        for i in range(3):
            assert _same(gnn_io.gnn_feature_map(graph, i), singles[last][2][i]), (dtype, order, "feature map", i, "of page", last)
        n_read = host[last]["N"]
        want = np.concatenate([singles[b][1] for b in order])[:n_read]
        assert _same(gnn_io.gnn_node_features(graph, n_read), want), (dtype, order, "node features")
        left = n_read
        for b in order:
            rows_seen[b] = max(rows_seen[b], min(left, host[b]["N"]))
            left = max(left - host[b]["N"], 0)
    assert rows_seen == [1, 3, 4]                                     # every row of every page was compared
    graph.close()


def _records(graph, run):
    """[(kernel with layer text, calls)] the backbone handle's launch records made during run().  tests/launch_records.py's `records` builds
    an ARU model of its own and records one asep_aru_forward_batch_dev2 call of it, so it cannot be pointed at a relation net's backbone; this
    makes the same three library calls it makes (asep_aru_profile mode 2, asep_aru_profile_report, asep_aru_profile 0) on that backbone."""
    import torch
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


# The launch records [(kernel with layer text, calls)] of the three visual entries on the one page of the test below, in the report's order
# (a kernel stands where it was first launched).  Recorded on an MI355X with the build in front of the refactor that gave the single and the
# uniform entry one body and the table entry its stages; literal on purpose: nothing here is computed from the code under test.
_BACKBONE_LAUNCHES = [
    ('res8v_down_kernel<0> unet_down_0 (conv1+3xconvR+add+pool) 71x53', 1),
    ('conv_mfma_kernel<3,3,1,true,16,false,false,false,4> aru_net/featMapG/unet_down_1/conv1 36x27 8->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,4> aru_net/featMapG/unet_down_1/convR_0 36x27 16->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,4> aru_net/featMapG/unet_down_1/convR_1 36x27 16->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,2> aru_net/featMapG/unet_down_1/convR_2 36x27 16->16', 1),
    ('conv_winor_kernel<false,2,false> aru_net/featMapG/unet_down_2/conv1 18x14 16->32', 1),
    ('conv_winor_kernel<false,2,false> aru_net/featMapG/unet_down_2/convR_0 18x14 32->32', 1),
    ('conv_winor_kernel<false,2,false> aru_net/featMapG/unet_down_2/convR_1 18x14 32->32', 1),
    ('conv_winor_kernel<false,2,true> aru_net/featMapG/unet_down_2/convR_2 18x14 32->32', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_3/conv1 9x7 32->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_3/convR_0 9x7 64->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_3/convR_1 9x7 64->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_3/convR_2 9x7 64->64', 1),
    ('maxpool2_kernel', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_4/conv1 5x4 64->128', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_4/convR_0 5x4 128->128', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_4/convR_1 5x4 128->128', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_down_4/convR_2 5x4 128->128', 1),
    ('deconv_mfma_kernel<2,false> aru_net/featMapG/unet_up_3/deconv 5x4 128->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_up_3/conv1 9x7 128->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_up_3/convR_0 9x7 64->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_up_3/convR_1 9x7 64->64', 1),
    ('conv_wino_kernel<4,false> aru_net/featMapG/unet_up_3/convR_2 9x7 64->64', 1),
    ('deconv_mfma_kernel<2,false> aru_net/featMapG/unet_up_2/deconv 9x7 64->32', 1),
    ('conv_winor_kernel<false,2,false> aru_net/featMapG/unet_up_2/conv1 18x14 64->32', 1),
    ('conv_winor_kernel<false,2,false> aru_net/featMapG/unet_up_2/convR_0 18x14 32->32', 1),
    ('conv_winor_kernel<false,2,false> aru_net/featMapG/unet_up_2/convR_1 18x14 32->32', 1),
    ('conv_winor_kernel<false,2,true> aru_net/featMapG/unet_up_2/convR_2 18x14 32->32', 1),
    ('deconv_mfma_kernel<1,false> aru_net/featMapG/unet_up_1/deconv 18x14 32->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,4> aru_net/featMapG/unet_up_1/conv1 36x27 32->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,4> aru_net/featMapG/unet_up_1/convR_0 36x27 16->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,4> aru_net/featMapG/unet_up_1/convR_1 36x27 16->16', 1),
    ('conv_mfma_kernel<3,3,1,false,16,false,false,false,2> aru_net/featMapG/unet_up_1/convR_2 36x27 16->16', 1),
    ('deconv8v_kernel aru_net/featMapG/unet_up_0/deconv 36x27 16->8', 1),
    ('res8v_up_kernel<0> unet_up_0 (conv1[16->8]+3xconvR+add) 71x53', 1),
    ('combine_kernel<8,2,false,1>', 1),
]
SINGLE_LAUNCHES = _BACKBONE_LAUNCHES + [
    ('fmap_conv1x1_kernel<false> fm_1 36x27 16->3', 1),
    ('fmap_conv3x3_kernel fm_1 36x27 3->6 s1', 1),
    ('fmap_conv1x1_kernel<false> fm_2 36x27 6->1', 1),
    ('fmap_conv3x3_kernel fm_2 36x27 1->2 s2', 1),
]
UNIFORM_LAUNCHES = _BACKBONE_LAUNCHES + [
    ('fmap_conv1x1_kernel<false> fm_1 36x27 16->3', 1),
    ('fmap_conv3x3_kernel fm_1 36x27 3->6 s1', 1),
    ('fmap_conv1x1_kernel<false> fm_2 36x27 6->1', 1),
    ('fmap_conv3x3_kernel fm_2 36x27 1->2 s2', 1),
]
TABLE_LAUNCHES = [
    ('moments_pages_kernel 1 pages', 1),
    ('moments_finish_pages_kernel 1 pages', 1),
] + _BACKBONE_LAUNCHES + [
    ('fmap_conv1x1_pages_kernel<false> fm_1 1 pages 16->3', 1),
    ('fmap_conv3x3_pages_kernel fm_1 1 pages 3->6 s1', 1),
    ('fmap_conv1x1_pages_kernel<false> fm_2 1 pages 6->1', 1),
    ('fmap_conv3x3_pages_kernel fm_2 1 pages 1->2 s2', 1),
    ('gnn_roi_compress_pages_kernel<false> 1 pages 6 entries 48 regions', 1),
]


def test_one_page_through_the_three_entries_keeps_each_launch_sequence_and_nothing_left_in_the_handle_changes_a_later_call():
    """one handle (an end point, a generated stride-1 and a generated stride-2 map, interaction visual features; fp32), one page of 71 x 53 with
    N = 4 nodes and 12 interactions, four calls with the launch records on: the single entry, the uniform entry with one page, the table entry
    with one page, the single entry again.  The first and the last call must give the same output bits and the same records, and every entry's
    records must be the literal list above."""
    import torch
    from citlab_article_separation_new_amd import gnn_io
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    cfg = GnnConfig(node_feature_dim=7, mvn=True, visual_layers=[UP1, UP1, ""], visual_layer_depths=[-1, 6, 2], visual_dims=[8, 4, 4], visual_edges=True,
                    backbone={"compute_dtype": "f32"})
    graph = gnn_io.GnnGraph(init_gnn_weights(cfg, 11, bias_jitter=0.05), cfg)
    h, w = 71, 53
    host = _host_pages(cfg, [(h, w)], seed=23, nodes=[4])
    assert host[0]["E"] == 12
    t, q = _upload(host[0], cfg.num_classes)
    entries = {
        "single": lambda: gnn_io.gnn_forward_visual_dev(graph, q["N"], q["E"], q["d_edges"], q["d_node_feat"], q["d_edge_feat"], q["d_image"], h, w,
                                                        q["d_regions"], P, q["d_num_points"], q["R"], q["d_relations"], q["d_probs_out"], None, 0,
                                                        d_edge_regions=q["d_edge_regions"], d_edge_num_points=q["d_edge_num_points"]),
        "uniform": lambda: gnn_io.gnn_forward_visual_batch_dev(graph, [q], h, w, P),
        "table": lambda: gnn_io.gnn_forward_visual_batch_dev2(graph, [q], [h], [w], P),
    }
    got = []
    for name in ("single", "uniform", "table", "single"):
        t["out"].zero_()
        recs = _records(graph, entries[name])
        torch.cuda.synchronize()
        got.append((name, recs, t["out"].cpu().numpy()))
        print(name, recs)
    graph.close()
    (_, recs1, out1), (_, recs4, out4) = got[0], got[3]
    assert np.isfinite(out1).all() and out1.shape == (16, 2)
    assert _same(out4, out1) and recs4 == recs1
    want = {"single": SINGLE_LAUNCHES, "uniform": UNIFORM_LAUNCHES, "table": TABLE_LAUNCHES}
    for name, recs, _ in got:
        assert recs == want[name], (name, recs)


def test_every_batched_stage_is_one_launch_per_call(cases):
    """what fails when the entry is a loop over the single-page one: per call ONE launch of the normalisation's moments (and one of their
    finish), ONE per convolution of each generated map and ONE ROI / compression launch, none of the single-page kernels"""
    from citlab_article_separation_new_amd import gnn_io
    c = cases("fmaps_visual_edges")
    pages = [q for _, q in c.dev]
    recs = _records(c.graph, lambda: gnn_io.gnn_forward_visual_batch_dev2(c.graph, pages, [s[0] for s in c.sizes], [s[1] for s in c.sizes], P))
    by = lambda part: [(k, n) for k, n in recs if part in k]                                                     # noqa: E731
    assert len(recs) > 10                                            # the backbone's layers are there
    assert by("moments_pages_kernel") == [("moments_pages_kernel 4 pages", 1)] and by("moments_finish_pages_kernel") == [("moments_finish_pages_kernel 4 pages", 1)]
    assert not by("moments_kernel") and not by("moments_finish_kernel")
    assert [n for _, n in by("fmap_conv1x1_pages_kernel<false>")] == [1, 1], by("fmap_conv1x1")     # two generated maps
    assert [n for _, n in by("fmap_conv3x3_pages_kernel")] == [1, 1], by("fmap_conv3x3")
    assert [n for _, n in by("gnn_roi_compress_pages_kernel<false>")] == [1], by("gnn_roi")
    assert not by("fmap_conv1x1_kernel") and not by("fmap_conv3x3_kernel") and not by("gnn_roi_compress_pages_kernel<true>")


def test_bad_arguments_are_refused_with_the_page_named_and_nothing_is_launched(cases):
    from citlab_article_separation_new_amd import _lib
    c = cases("fmaps_visual_edges")
    lib = _lib.init_device(0)
    g = c.graph.handle(0)
    arr = (_lib.GnnPage * 4)()
    for q, (_, d) in zip(arr, c.dev):
        for k, v in d.items():
            setattr(q, k, v)
    Ints = C.c_int32 * 4
    hs, ws = Ints(*[s[0] for s in c.sizes]), Ints(*[s[1] for s in c.sizes])
    zero_w = Ints(53, 53, 0, 53)
    neg_h = Ints(64, -3, 64, 64)
    calls = {
        "n_pages = 0": lambda: lib.asep_gnn_forward_visual_batch_dev2(g, 0, arr, hs, ws, P, None),
        "size array h is NULL": lambda: lib.asep_gnn_forward_visual_batch_dev2(g, 4, arr, None, ws, P, None),
        "size array w is NULL": lambda: lib.asep_gnn_forward_visual_batch_dev2(g, 4, arr, hs, None, P, None),
        "page 2 has the size 71 x 0": lambda: lib.asep_gnn_forward_visual_batch_dev2(g, 4, arr, hs, zero_w, P, None),
        "page 1 has the size -3 x 64": lambda: lib.asep_gnn_forward_visual_batch_dev2(g, 4, arr, neg_h, ws, P, None),
    }
    for text, call in calls.items():
        rc = []
        recs = _records(c.graph, lambda: rc.append(call()))
        assert rc == [-1], text                                      # ASEP_ERR_ARG
        assert text in _lib.last_error(), (text, _lib.last_error())
        assert recs == [], (text, recs)
    _assert_pages_equal(c.batch(), c.singles, "after the refusals")  # the handle is as good as before


# ---- uint8 scans ------------------------------------------------------------------------------------------------------------------
U8_SOURCES = [(300, 200), (211, 333), (256, 256)]
U8_TARGETS = [(96, 64), (71, 112), (80, 80)]


def _u8_case(cases, name, scan_channels):
    """-> (case, scans uint8, their tensors, page dicts): three pages of the case's model fed as scans"""
    import torch
    from citlab_article_separation_new_amd import synth
    c = cases(name)
    rng = np.random.default_rng(3)
    host = _host_pages(c.cfg, U8_TARGETS + [(64, 64)], seed=23)[:3]
    scans = []
    for k, (H, W) in enumerate(U8_SOURCES):
        gray = synth.synth_page(70 + k, W=W, H=H).astype(np.float32)
        if scan_channels == 3:
            gray = np.clip(gray[:, :, None] * np.array([0.35, 0.7, 1.0], np.float32) + rng.random((H, W, 3), dtype=np.float32) * 30, 0, 255)
        scans.append(np.ascontiguousarray(gray.astype(np.uint8)))
    dev = [_upload(p, c.cfg.num_classes) for p in host]
    return c, host, scans, [torch.from_numpy(x).cuda() for x in scans], dev


@pytest.mark.parametrize("name,scan_channels", [("fmaps_visual_edges", 1), ("fmaps_visual_edges", 3), ("ru_rgb", 3)],
                         ids=["gray_scan", "colour_scan_luma", "colour_scan_rgb_backbone"])
def test_uint8_scans_of_three_sizes_in_one_call_equal_the_single_page_u8_path(name, scan_channels, cases):
    import torch
    from citlab_article_separation_new_amd import gnn_io, image_ops
    c, host, scans, d_scans, dev = _u8_case(cases, name, scan_channels)
    chans = c.cfg.backbone_cfg().channels
    mode = "keep" if scan_channels == chans else "luma"
    want = []
    for (t, q), d_scan, (h, w) in zip(dev, d_scans, U8_TARGETS):      # the single-page path: one resize launch, one forward
        d_img = image_ops.resize_tf1_dev(d_scan, h, w, mode, 0)
        t["out"].zero_()
        gnn_io.gnn_forward_visual_dev(c.graph, q["N"], q["E"], q["d_edges"], q["d_node_feat"], q["d_edge_feat"], d_img.data_ptr(), h, w,
                                      q["d_regions"], P, q["d_num_points"], q["R"], q["d_relations"], q["d_probs_out"], None, 0,
                                      d_edge_regions=q["d_edge_regions"], d_edge_num_points=q["d_edge_num_points"])
        torch.cuda.synchronize()
        want.append((d_img.cpu().numpy().reshape(h, w, chans), t["out"].cpu().numpy()))
        t["out"].zero_()
    pages = [dict(q, d_image=None) for _, q in dev]
    src = [(d.data_ptr(), s.shape[0], s.shape[1], scan_channels) for d, s in zip(d_scans, scans)]
    recs = _records(c.graph, lambda: gnn_io.gnn_forward_visual_batch_u8_dev(c.graph, pages, src, [s[0] for s in U8_TARGETS], [s[1] for s in U8_TARGETS], P))
    assert [(k, n) for k, n in recs if "prep_resize" in k] == [("prep_resize_tf1_pages_kernel 3 pages", 1)]       # one launch for the three scans
    assert [(k, n) for k, n in recs if "moments_pages" in k] == [("moments_pages_kernel 3 pages", 1)]
    for b, ((img0, p0), (t, _)) in enumerate(zip(want, dev)):
        img = gnn_io.gnn_page_image(c.graph, b)
        assert img.shape == img0.shape and np.array_equal(img.view(np.uint32), img0.view(np.uint32)), ("resized bytes of page", b)
        assert np.isfinite(p0).all() and _same(t["out"].cpu().numpy(), p0), ("probabilities of page", b)


def test_a_page_whose_image_channels_do_not_match_the_backbone_is_refused_and_nothing_is_launched(cases):
    """the entry that knows a page's channels: a gray scan into the colour backbone is ASEP_ERR_ARG naming the page"""
    from citlab_article_separation_new_amd import _lib, gnn_io
    c, host, scans, d_scans, dev = _u8_case(cases, "ru_rgb", 3)
    pages = [dict(q, d_image=None) for _, q in dev]
    src = [(d.data_ptr(), s.shape[0], s.shape[1], 3) for d, s in zip(d_scans, scans)]
    src[1] = (src[1][0], 211, 333, 1)                                 # page 1 says one channel
    err = []

    def call():
        try:
            gnn_io.gnn_forward_visual_batch_u8_dev(c.graph, pages, src, [s[0] for s in U8_TARGETS], [s[1] for s in U8_TARGETS], P)
        except _lib.AsepError as e:
            err.append(str(e))
    recs = _records(c.graph, call)
    assert len(err) == 1 and "page 1: the scan has 1 image channel(s), the backbone takes 3" in err[0], err
    assert recs == []
