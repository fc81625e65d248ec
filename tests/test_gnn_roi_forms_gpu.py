"""gnn_roi_compress_kernel / gnn_roi_compress_pages_kernel (csrc/gnn_kernels.h): every reduce form, negative maps, region edges, the page
table and the dense layer, with the region maxima observed BIT FOR BIT through the existing ABI.

Method.  For a map of C channels the model's compression layer is 2C wide, its weights are [ I | -I ] and its bias is zero, so the kernel
writes relu(v) and relu(-v): every product is v * (+-1) or v * 0 and every sum is exact, and features[:, :C] - features[:, C:2C] is the
region maximum v without rounding.  The reference is numpy on the ENGINE'S OWN map (asep_gnn_get_feature_map; a bf16 map widens exactly):
the rectangle of oracle/gnn_oracle.py:visual_node_features (float32 product, floor, clamp, at least one cell) and a plain max.  No tolerance.

Which reduction runs (VEC = 4 values per 16-byte load for an fp32 map, 8 for a bf16 map):
  vector   C % VEC == 0 and C / VEC in {1, 2, 4, 8} groups: xor-shuffle over the groups, four waves through LDS
  thread   256 % C == 0 otherwise: one channel per thread, red[256] reduced at stride C (256 / C partials per channel)
  generic  every other C: one thread per channel, nested loops

  map type  C     form (groups / partials)   reached by
  fp32      4     vector (1)                 generated depth 4 from up_1
  fp32      8     vector (2)                 feat_root 8 up_0
  fp32      16    vector (4)                 feat_root 8 up_1, feat_root 16 up_0
  fp32      32    vector (8)                 feat_root 8 up_2 (geometry, negative maps)
  fp32      64    thread (4)                 feat_root 8 down_3 (f32s and f32), generated depth 64, feat_root 16 down_2 (dense layer)
  fp32      128   thread (2)                 feat_root 8 down_4
  fp32      256   thread (1)                 feat_root 16 down_4, generated depth 256
  fp32      6     generic                    generated depth 6 (geometry)
  fp32      24    generic                    generated depth 24, stride 2 below the depth-4 map
  fp32      48    generic                    generated depth 48
  fp32      96    generic                    generated depth 96
  bf16      8     vector (1)                 feat_root 8 up_0
  bf16      16    vector (2)                 feat_root 8 up_1
  bf16      32    vector (4)                 feat_root 8 up_2
  bf16      64    vector (8)                 feat_root 8 down_3
  bf16      128   thread (2)                 feat_root 8 down_4
  bf16      24/48 generic                    NOT reachable: generated maps are fp32, and the bf16 engine is a feat_root 8 engine -- a
                                             feat_root 12 bf16 backbone is refused (at its first forward, not at load); the refusal and its
                                             message are asserted instead
A feat_root 4 backbone (fp32 end points of 4 and 8 channels) is refused by the fp32 engines the same way (no first-layer kernel of 4
output channels); that refusal is asserted too, C = 4 and 8 come from the rows above.

Pages: 64 x 48 (level-4 maps of 4 x 3 cells), 200 x 160 and 96 x 176 for the fp32 engines; 64 x 96 and 200 x 160 for the bf16 engine (level-3
maps of 8 and 25 rows: clear of DESIGN.md's open fault on maps one row high)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

UP0, UP1, UP2 = "scale_0_unet_up_0_conv", "scale_0_unet_up_1_conv", "scale_0_unet_up_2_conv"
D2, D3, D4 = "scale_0_unet_down_2_conv", "scale_0_unet_down_3_conv", "scale_0_unet_down_4_conv"
GEO = 7
POISON = 9.0                                                         # in the slots behind num_points: must never be read

# name -> layout, the channels every map is meant to have and the backbone; the reduce form follows from (map type, C): _form
MODELS = {
    "fr8_f32s": dict(layers=[D3, D4, UP0, UP1, UP1, "", UP1, UP1, UP1, UP1], depths=[-1, -1, -1, -1, 4, 24, 48, 64, 96, 256],
                     C=[64, 128, 8, 16, 4, 24, 48, 64, 96, 256],
                     forms=["thread", "thread", "vector", "vector", "vector", "generic", "generic", "thread", "generic", "thread"], backbone={}),
    "fr8_f32": dict(layers=[D3, D4], C=[64, 128], forms=["thread", "thread"], backbone={"compute_dtype": "f32"}),
    "fr16_f32s": dict(layers=[D4, UP0], C=[256, 16], forms=["thread", "vector"], backbone={"feat_root": 16}),
    "fr8_bf16": dict(layers=[UP0, UP1, UP2, D3, D4], C=[8, 16, 32, 64, 128], forms=["vector"] * 4 + ["thread"],
                     backbone={"compute_dtype": "bf16"}),
    "geometry": dict(layers=[UP2, D3, UP1], depths=[-1, -1, 6], C=[32, 64, 6], forms=["vector", "thread", "generic"], backbone={}),
}
for _act in ("leaky", "elu"):
    for _dt in ("f32s", "bf16"):
        MODELS[f"{_act}_{_dt}"] = dict(layers=[UP2, D4], C=[32, 128], forms=["vector", "thread"],
                                       backbone={"activation_name": _act, "compute_dtype": _dt})


def _form(bf16, C):
    """the branch of gnn_roi_compress_kernel_body a map of C channels takes (its end points and arena maps are 16-byte aligned)"""
    vec = 8 if bf16 else 4
    if C % vec == 0 and C // vec in (1, 2, 4, 8):
        return "vector"
    return "thread" if 256 % C == 0 else "generic"


class _Model:
    """a relation net whose node compression layers are the identity pairs (identity=True) or seeded random layers `dims` wide"""

    def __init__(self, layers, depths=None, backbone=None, identity=True, dims=None, seed=11, **kw):
        from citlab_article_separation_new_amd.config import GnnConfig
        from citlab_article_separation_new_amd.gnn_io import GnnGraph
        from citlab_article_separation_new_amd.weights import init_gnn_weights
        base = dict(node_feature_dim=GEO, mvn=True, visual_layers=list(layers), visual_layer_depths=list(depths or []), backbone=dict(backbone or {}), **kw)
        self.C = GnnConfig(visual_dims=[1] * len(layers), **base).visual_channels()
        self.dims = [2 * c for c in self.C] if identity else list(dims)
        self.cfg = GnnConfig(visual_dims=self.dims, **base)
        self.bf16 = self.cfg.backbone_cfg().compute_dtype == "bf16"
        self.w = init_gnn_weights(self.cfg, seed, bias_jitter=0.05)
        if identity:
            for i, c in enumerate(self.C):
                eye = np.eye(c, dtype=np.float32)
                self.w[f"visual_node_feature_compression_fm_{i}/dense/weights"] = np.ascontiguousarray(np.concatenate([eye, -eye], axis=1))
                self.w[f"visual_node_feature_compression_fm_{i}/dense/bias"] = np.zeros(2 * c, np.float32)
        self.graph = GnnGraph(self.w, self.cfg)

    def forward(self, img, regions, npts, **kw):
        """one page through asep_gnn_forward_visual -> (probabilities, node features, the engine's feature maps)"""
        from citlab_article_separation_new_amd import gnn_io, synth
        N = len(npts)
        g = synth.synth_graph(1, N=N, n_pairs=2 * N, node_dim=GEO)
        self.inputs = g
        probs = gnn_io.gnn_forward_visual(self.graph, N, g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts, **kw)
        u = gnn_io.gnn_node_features(self.graph, N)
        return probs, u, [gnn_io.gnn_feature_map(self.graph, i) for i in range(len(self.C))]


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(name):
        if name not in made:
            spec = MODELS[name]
            made[name] = _Model(spec["layers"], spec.get("depths"), spec["backbone"])
            assert made[name].C == spec["C"], (name, made[name].C)
        return made[name]
    yield get
    for m in made.values():
        m.graph.close()


def _image(hw, seed=5):
    """a synthetic scan under strong noise, 0..255 as fed: every map gets cells that differ"""
    from citlab_article_separation_new_amd import synth
    h, w = hw
    rng = np.random.default_rng(seed)
    img = synth.synth_page(seed, W=w, H=h).astype(np.float32) + rng.normal(0, 40, size=(h, w)).astype(np.float32)
    return np.ascontiguousarray(np.clip(img, 0, 255), np.float32)


def _regions(seed, N=14, P=4):
    """node 0 the full page, node 1 without points, node 2 a single point, node 3 two points of four, nodes 4-7 random rectangles, the rest
    one point each (one cell on every map: where a negative maximum shows)"""
    rng = np.random.default_rng(seed)
    regions = np.full((N, 2, P), POISON, np.float32)
    npts = np.full(N, P, np.int32)
    for n in range(N):
        x0, y0 = rng.random() * 0.8, rng.random() * 0.8
        if n < 8:
            x1, y1 = x0 + 0.02 + rng.random() * 0.18, y0 + 0.01 + rng.random() * 0.1
            regions[n, 0, :4] = [x0, x1, x1, x0]
            regions[n, 1, :4] = [y0, y0, y1, y1]
        else:
            regions[n, :, :] = np.array([[x0], [y0]], np.float32)
    regions[0, 0, :4] = [0.0, 1.0, 1.0, 0.0]
    regions[0, 1, :4] = [0.0, 0.0, 1.0, 1.0]
    npts[1] = 0
    regions[1, :, :] = POISON
    regions[2, :, :] = 0.5
    npts[3] = 2
    regions[3, :, 2:] = POISON
    return regions, npts


def _rects(regions, npts, fh, fw):
    """oracle/gnn_oracle.py:visual_node_features' rectangle per region -> int [N, 8]: x0, x1, y0, y1 clamped into the map, then the same four
    before the clamp.  num_points above P counts as P (the kernel's documented min(npts, P))"""
    regions = np.asarray(regions, np.float32)
    N, _, P = regions.shape
    out = np.zeros((N, 8), np.int64)
    for n in range(N):
        k = min(int(npts[n]), P)
        if k > 0:
            lim = [regions[n, 0, :k].min(), regions[n, 0, :k].max(), regions[n, 1, :k].min(), regions[n, 1, :k].max()]
        else:
            lim = [np.float32(0)] * 4
        raw = [int(np.floor(np.float32(v) * np.float32(s))) for v, s in zip(lim, (fw, fw, fh, fh))]
        out[n] = [max(min(r, s - 1), 0) for r, s in zip(raw, (fw, fw, fh, fh))] + raw
    return out


def _roi_max(fm, rects):
    out = np.empty((len(rects), fm.shape[2]), np.float32)
    for n, (x0, x1, y0, y1) in enumerate(rects[:, :4]):
        nx, ny = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
        out[n] = fm[y0:y0 + ny, x0:x0 + nx].max(axis=(0, 1))
    return out


def _maxima(u, chans):
    """the identity pairs' columns of the node features -> the region maxima per map, exact"""
    col, out = GEO, []
    for c in chans:
        pos, neg = u[:, col:col + c], u[:, col + c:col + 2 * c]
        assert (pos >= 0).all() and (neg >= 0).all() and (np.minimum(pos, neg) == 0).all()        # relu(v) and relu(-v)
        out.append(pos - neg)
        col += 2 * c
    assert col == u.shape[1]
    return out


def _expected_shapes(layers, hw):
    """[fh, fw] per map: ceil(page / 2^level) for an end point and a stride-1 generated map, ceil(previous / 2) under an empty from_layer"""
    out = []
    for name in layers:
        if name:
            lv = int(re.fullmatch(r"scale_0_unet_(?:down|up)_(\d)_conv", name).group(1))
            out.append((-(-hw[0] // (1 << lv)), -(-hw[1] // (1 << lv))))
        else:
            out.append((-(-out[-1][0] // 2), -(-out[-1][1] // 2)))
    return out


def _assert_maxima(label, m, spec, u, maps, regions, npts, hw):
    """channels, shapes and forms as the case means them, then the maxima bit for bit; -> [(reference maxima, rectangles)] per map"""
    assert [fm.shape[2] for fm in maps] == spec["C"], (label, [fm.shape for fm in maps])
    assert [fm.shape[:2] for fm in maps] == _expected_shapes(spec["layers"], hw), (label, [fm.shape for fm in maps])
    assert [_form(m.bf16, c) for c in spec["C"]] == spec["forms"], label
    got = _maxima(u, spec["C"])
    refs, wrong = [], []
    for i, fm in enumerate(maps):
        assert np.isfinite(fm).all() and float(fm.max()) > float(fm.min()), (label, i)
        if m.bf16:
            assert not (fm.view(np.uint32) & 0xffff).any(), (label, i, "a bf16 map widens to floats with 16 zero bits")
        rects = _rects(regions, npts, fm.shape[0], fm.shape[1])
        ref = _roi_max(fm, rects)
        bad = np.argwhere(got[i] != ref)
        if len(bad):                                                 # every map is looked at before the case fails: one wrong form does not hide another
            wrong.append(("map", i, "C", spec["C"][i], spec["forms"][i], len(bad), "wrong maxima, first (region, channel)", bad[0].tolist(),
                          "rectangle", rects[bad[0][0]].tolist()))
        refs.append((ref, rects))
    assert not wrong, (label, wrong)
    return refs


def _run_exact(name, m, hw, seed=3):
    spec = MODELS[name]
    regions, npts = _regions(seed)
    _, u, maps = m.forward(_image(hw), regions, npts)
    assert np.array_equal(u[:, :GEO], m.inputs["node_features"])     # the fed columns stay in front
    refs = _assert_maxima(f"{name} {hw}", m, spec, u, maps, regions, npts, hw)
    for (ref, rects), fm in zip(refs, maps):                          # the regions are what their docstring says on every map
        nx, ny = rects[:, 1] - rects[:, 0] + 1, rects[:, 3] - rects[:, 2] + 1
        assert nx[0] == fm.shape[1] and ny[0] == fm.shape[0] and (rects[1, :4] == 0).all() and (nx[8:] * ny[8:] == 1).all()
    return refs


# ---- 1. every reduce form, fp32 maps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(64, 48), (200, 160)], ids=["64x48", "200x160"])
@pytest.mark.parametrize("name", ["fr8_f32s", "fr8_f32", "fr16_f32s"])
def test_fp32_maps_of_every_reduce_form_give_the_exact_region_maxima(name, hw, models):
    m = models(name)
    assert not m.bf16
    _run_exact(name, m, hw)


def test_a_feat_root_4_backbone_is_refused_by_name_at_its_first_forward():
    """the fp32 end points of 4 and 8 channels the issue asks for (feat_root 4: up_0, up_1): the engine has no first-layer kernel of 4 output
    channels and says so; fp32 maps of 4 and 8 channels are tested on a generated map and on feat_root 8's up_0 instead"""
    from citlab_article_separation_new_amd import _lib
    m = _Model([UP0, UP1], backbone={"feat_root": 4})
    assert m.C == [4, 8]
    regions, npts = _regions(3)
    with pytest.raises(_lib.AsepError, match="first-layer conv k=3 cout=4 not instantiated"):
        m.forward(_image((64, 48)), regions, npts)
    m.graph.close()


# ---- 2. every reduce form, bf16 maps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(64, 96), (200, 160)], ids=["64x96", "200x160"])
def test_bf16_maps_of_every_reduce_form_give_the_exact_region_maxima(hw, models):
    m = models("fr8_bf16")
    assert m.bf16
    _run_exact("fr8_bf16", m, hw)


def test_a_feat_root_12_bf16_backbone_is_refused_so_no_bf16_map_reaches_the_generic_form():
    """bf16 maps of 24 and 48 channels (the generic form over bf16 values) would need a feat_root 12 bf16 backbone; the bf16 engine is a
    feat_root 8 engine.  It loads such a model and refuses its first forward, naming the first layer; generated maps are fp32 whatever
    the backbone.  So gnn_roi_compress_kernel<true> cannot reach its generic branch through the ABI today."""
    from citlab_article_separation_new_amd import _lib
    m = _Model([UP1, UP2], backbone={"feat_root": 12, "compute_dtype": "bf16"})
    assert m.C == [24, 48] and [_form(True, c) for c in m.C] == ["generic", "generic"]
    regions, npts = _regions(3)
    with pytest.raises(_lib.AsepError, match=re.escape("bf16 path: first-layer conv k=3 cin=1 cout=12 not instantiated")):
        m.forward(_image((64, 96)), regions, npts)
    m.graph.close()


# ---- 3. negative maps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
@pytest.mark.parametrize("act", ["leaky", "elu"])
def test_maps_with_negative_values_give_negative_maxima(act, dtype, models):
    """leaky / elu backbones: a vector-form map (up_2, 32 channels) and a one-channel-per-thread map (down_4, 128 channels).  The reference
    alone must hold negative maxima on every map (several regions, one of more than one cell where the page gives one), else the case
    says nothing about where the kernel starts its maxima."""
    name = f"{act}_{dtype}"
    refs = _run_exact(name, models(name), (64, 96))
    for i, (ref, rects) in enumerate(refs):
        neg = (ref < 0).any(axis=1)
        cells = (rects[:, 1] - rects[:, 0] + 1) * (rects[:, 3] - rects[:, 2] + 1)
        print(f"{name}: map {i}: {int(neg.sum())} of {len(neg)} regions with a negative maximum ({int((ref < 0).sum())} values), "
              f"largest such region {int(cells[neg].max()) if neg.any() else 0} cells")
        assert neg.sum() >= 3, (name, i)


@pytest.mark.parametrize("act", ["leaky", "elu"])
def test_visual_forward_over_a_leaky_or_elu_backbone_matches_the_oracle(act):
    """seeded compression layers (8 and 4 wide) over up_2 and down_4 of an f32s backbone: node features and probabilities against
    gnn_oracle.forward_visual at the fp32 gates of tests/test_gnn_visual_gpu.py, 1e-4 * max(1, max|u|) and 1e-5"""
    from oracle import gnn_oracle
    m = _Model([UP2, D4], backbone={"activation_name": act}, identity=False, dims=[8, 4])
    regions, npts = _regions(3)
    img = _image((64, 96))
    probs, u, _ = m.forward(img, regions, npts)
    g = m.inputs
    ref_probs, ref_u = gnn_oracle.forward_visual(len(npts), g["interacting_nodes"], g["node_features"], g["edge_features"], img, regions, npts, None, m.w, m.cfg)
    du, dp, mu = float(np.abs(u - ref_u).max()), float(np.abs(probs - ref_probs).max()), float(np.abs(ref_u).max())
    print(f"{act}: max|du| = {du:.3e} (max|u| {mu:.3f}), max|dp| = {dp:.3e}")
    assert (ref_u[:, GEO:GEO + 8] > 0).any() and (ref_u[:, GEO + 8:] > 0).any()
    assert np.array_equal(u[:, :GEO], ref_u[:, :GEO])
    assert du <= 1e-4 * max(1.0, mu) and dp <= 1e-5
    m.graph.close()


# ---- 4. region geometry -----------------------------------------------------------------------------------------------------------------
GEO_HW, GEO_P = (96, 176), 5                                         # up_2: 24 x 44, down_3: 12 x 22, the depth-6 map over up_1: 48 x 88


def _axis_values(sizes):
    f = np.float32
    vals = [f(0.0), f(1.0), f(1.5), f(-0.25), np.nextafter(f(1), f(0))]
    for s in sorted(set(sizes)):
        for k in sorted({1, 2, s // 2, s - 1}):
            b = f(k / s)                                             # a cell boundary of a map s cells wide, and its float32 neighbours
            vals += [np.nextafter(b, f(-1)), b, np.nextafter(b, f(2))]
    return vals


def _geometry_regions():
    """two-point regions in GEO_P slots (the other slots poisoned), then the point-count regions -> (regions, npts, rows of the special ones)"""
    fh, fw = zip(*_expected_shapes(MODELS["geometry"]["layers"], GEO_HW))
    boxes = [(0.0, 1.0, 0.0, 1.0), (-0.25, 1.5, -0.25, 1.5), (0.5, 0.5, 0.5, 0.5), (1.0, 1.5, 1.0, 1.5), (-0.25, 0.0, -0.25, 0.0),
             (1.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 1.0)]
    for v in _axis_values(fw):
        boxes += [(v, v, 0.3, 0.6), (0.26, v, 0.4, 0.4)]
    for v in _axis_values(fh):
        boxes += [(0.3, 0.6, v, v), (0.4, 0.4, 0.26, v)]
    n2 = len(boxes)
    N = n2 + 5
    regions = np.full((N, 2, GEO_P), POISON, np.float32)
    regions[:, 1, 2:] = -POISON
    npts = np.full(N, 2, np.int32)
    for n, (xa, xb, ya, yb) in enumerate(boxes):
        regions[n, 0, :2] = [xa, xb]
        regions[n, 1, :2] = [ya, yb]
    rows = dict(no_points=n2, one_point=n2 + 1, all_points=n2 + 2, last_is_extreme=n2 + 3, above_P=n2 + 4)
    npts[n2] = 0                                                     # every slot poisoned: the rectangle is cell (0, 0)
    npts[n2 + 1] = 1
    regions[n2 + 1, :, 0] = [0.7, 0.2]
    npts[n2 + 2] = npts[n2 + 3] = GEO_P
    regions[n2 + 2, 0] = [0.40, 0.45, 0.90, 0.42, 0.50]
    regions[n2 + 2, 1] = [0.50, 0.52, 0.10, 0.50, 0.48]
    regions[n2 + 3, 0] = [0.40, 0.45, 0.50, 0.42, 0.93]              # the last point alone has the largest x and the smallest y
    regions[n2 + 3, 1] = [0.50, 0.52, 0.48, 0.50, 0.07]
    npts[n2 + 4] = GEO_P + 3                                         # the kernel's min(npts, P): all P points and nothing behind them
    regions[n2 + 4, 0] = [0.30, 0.20, 0.25, 0.22, 0.04]
    regions[n2 + 4, 1] = [0.60, 0.62, 0.58, 0.60, 0.97]
    return regions, npts, rows


def test_region_edges_clamps_cell_boundaries_and_point_counts(models):
    """one model with maps of 32 (vector), 64 (one channel per thread) and 6 channels (generic) on a 96 x 176 page; per axis rel = 0, 1, 1.5,
    -0.25, nextafter(1, 0) and float32(k / size) with its two neighbours for k in {1, 2, size / 2, size - 1} of every map's size;
    num_points 0, 1, P and P + 3 (the host entry passes it on, the kernel clamps to P)"""
    m = models("geometry")
    spec = MODELS["geometry"]
    regions, npts, rows = _geometry_regions()
    _, u, maps = m.forward(_image(GEO_HW), regions, npts)
    refs = _assert_maxima("geometry", m, spec, u, maps, regions, npts, GEO_HW)
    assert maps[0].shape[1] >= 40
    for i, ((ref, rects), fm) in enumerate(zip(refs, maps)):
        fh, fw, C = fm.shape
        x0, x1, y0, y1, rx0, rx1, ry0, ry1 = rects.T
        nx, ny = x1 - x0 + 1, y1 - y0 + 1
        assert (rx0 < 0).any() and (rx1 > fw - 1).any() and (ry0 < 0).any() and (ry1 > fh - 1).any(), (i, "a clamp on each of the four sides")
        assert ((nx == 1) & (ny == 1)).any() and ((nx == fw) & (ny == fh)).any(), (i, "a one-cell and a full-map rectangle")
        assert nx.max() * C > 256 * (4 if spec["forms"][i] == "vector" else 1), (i, "a row loop that runs more than once")
        assert min(len(np.unique(c)) for c in (x0, x1, y0, y1)) >= 5  # first, second, middle and last cells, both sides of their boundaries
        assert (rects[rows["no_points"], :4] == 0).all() and nx[rows["one_point"]] == 1 and ny[rows["one_point"]] == 1
        for r in ("all_points", "last_is_extreme", "above_P"):
            k = rows[r]
            want = [int(np.floor(np.float32(v) * np.float32(s))) for v, s in ((regions[k, 0].min(), fw), (regions[k, 0].max(), fw),
                                                                              (regions[k, 1].min(), fh), (regions[k, 1].max(), fh))]
            assert rects[k, :4].tolist() == want, (i, r)             # all P points, the last one included, none of another region's
        kx = rects[rows["last_is_extreme"]]
        assert kx[1] == int(np.floor(np.float32(0.93) * np.float32(fw))) and kx[2] == int(np.floor(np.float32(0.07) * np.float32(fh)))


# ---- 5. the page table ------------------------------------------------------------------------------------------------------------------
TABLE_SIZES = [(64, 48), (200, 160), (96, 176)]
TABLE_NODES = [5, 12, 9]


def _table_call(m, dev):
    """the pages of `dev` in one asep_gnn_forward_visual_batch_dev2 call -> per page (probabilities, node features, feature maps)"""
    import torch
    from citlab_article_separation_new_amd import gnn_io
    for t, _ in dev:
        t["out"].zero_()
    gnn_io.gnn_forward_visual_batch_dev2(m.graph, [q for _, q in dev], [s[0] for s in TABLE_SIZES], [s[1] for s in TABLE_SIZES], 4)
    torch.cuda.synchronize()
    return [(t["out"].cpu().numpy(), gnn_io.gnn_page_node_features(m.graph, k, q["N"]), [gnn_io.gnn_page_feature_map(m.graph, k, i) for i in range(len(m.C))])
            for k, (t, q) in enumerate(dev)]


def test_page_table_form_gives_the_exact_maxima_of_every_page(models):
    """gnn_roi_compress_pages_kernel over three pages of 64 x 48, 200 x 160 and 96 x 176 in one call, maps of 32, 64 and 6 channels: every
    page's maxima bit for bit against numpy on that page's own maps, and its features those of the single-page call"""
    from test_gnn_visual_batch2_gpu import _host_pages, _same, _single, _upload
    m = models("geometry")
    spec = MODELS["geometry"]
    host = _host_pages(m.cfg, TABLE_SIZES, seed=31, nodes=TABLE_NODES)
    dev = [_upload(p, m.cfg.num_classes) for p in host]
    singles = [_single(m.graph, t, q, h, w, len(m.C)) for (t, q), (h, w) in zip(dev, TABLE_SIZES)]
    for b, ((p, u, maps), (p0, u0, maps0), page) in enumerate(zip(_table_call(m, dev), singles, host)):
        assert np.isfinite(p0).all() and _same(p, p0) and _same(u, u0), ("page", b)
        assert all(_same(a, a0) for a, a0 in zip(maps, maps0)), ("maps of page", b)
        refs = _assert_maxima(f"page {b}", m, spec, u, maps, page["regions"], page["npts"], TABLE_SIZES[b])
        assert all((rects[1, :4] == 0).all() and rects[0, 1] == fm.shape[1] - 1 and rects[0, 3] == fm.shape[0] - 1 for (_, rects), fm in zip(refs, maps))


def _oracle_over_float64_maps(page, m):
    """tests/fmap_reference.py:forward_visual_maps with the backbone's end points evaluated in float64 (oracle/aru_oracle.py:forward_torch,
    dtype=float64) -> (probabilities, node features); generator, ROI maxima, compression and graph as that function has them"""
    import torch
    import fmap_reference as fr
    from oracle import aru_oracle, gnn_oracle
    ends = aru_oracle.forward_torch(page["img"], {k: v for k, v in m.w.items() if k.startswith("aru_net/")}, m.cfg.backbone_cfg(),
                                    return_intermediates=True, dtype=torch.float64)[1]
    maps = [np.asarray(fm, np.float32) for fm in fr.generated_maps(ends, m.cfg.visual_layers, m.cfg.layer_depths(), m.w)]
    u = np.concatenate([page["u"], fr.roi_features(maps, page["regions"], page["npts"], m.w)], axis=1)
    ef = np.concatenate([page["ef"], fr.roi_features(maps, page["eregions"], page["enpts"], m.w, scope_kind="edge")], axis=1)
    return gnn_oracle.forward(page["N"], page["edges"], u, ef, page["rel"], m.w, m.cfg), u


def test_page_table_form_with_visual_edges_equals_the_single_page_calls_and_the_oracle():
    """the interactions' side with the new channel counts: visual_edges over down_3 (64), down_4 (128) and a generated 24-channel map, seeded
    compression layers of 8, 4 and 4 for nodes and edges.  Per page: probabilities, node features and maps of the single-page call bit for bit,
    and node features and probabilities within the fp32 gates of tests/test_fmap_gpu.py, 1e-4 * max(1, max|u|) and 1e-5, of the oracle.

    The oracle's backbone is evaluated in float64 here.  Its float32 evaluation (forward_visual_maps as it stands) is itself further from the
    float64 one than the gate on these noisy pages: measured on the MI355X, page 64 x 48 / 200 x 160 / 96 x 176, max|dp| of the float32 oracle
    against the float64 one 1.03e-5 / 4.8e-7 / 2.01e-5 (its maps 6e-5 / 5e-6 / 1.9e-4 of max|map| off), of the engine against the float64
    one 4.8e-7 / 2.7e-7 / 3.9e-7 with the f32s backbone and 2.1e-7 / 1.2e-7 / 3.0e-7 with the f32 one (maps 1.7e-6 and 8.4e-7 at most).
    Against the float32 evaluation the engine therefore reads 1.06e-5 / 5.4e-7 / 2.01e-5: the reference's own error, not the engine's."""
    from test_gnn_visual_batch2_gpu import _host_pages, _same, _single, _upload
    m = _Model([D3, D4, UP1], depths=[-1, -1, 24], identity=False, dims=[8, 4, 4], visual_edges=True)
    assert m.C == [64, 128, 24] and [_form(False, c) for c in m.C] == ["thread", "thread", "generic"]
    host = _host_pages(m.cfg, TABLE_SIZES, seed=31, nodes=TABLE_NODES)
    assert [p["E"] for p in host] == [15, 0, 27]
    dev = [_upload(p, m.cfg.num_classes) for p in host]
    singles = [_single(m.graph, t, q, h, w, len(m.C)) for (t, q), (h, w) in zip(dev, TABLE_SIZES)]
    for b, ((p, u, maps), (p0, u0, maps0), page) in enumerate(zip(_table_call(m, dev), singles, host)):
        assert np.isfinite(p0).all() and _same(p, p0) and _same(u, u0), ("page", b)
        assert [fm.shape[2] for fm in maps] == m.C and all(_same(a, a0) for a, a0 in zip(maps, maps0)), ("maps of page", b)
        ref_p, ref_u = _oracle_over_float64_maps(page, m)
        du, dp, mu = float(np.abs(u - ref_u).max()), float(np.abs(p - ref_p).max()), float(np.abs(ref_u).max())
        print(f"page {b} {TABLE_SIZES[b]}: max|du| = {du:.3e} (max|u| {mu:.3f}), max|dp| = {dp:.3e}")
        assert all((ref_u[:, lo:hi] > 0).any() for lo, hi in ((GEO, GEO + 8), (GEO + 8, GEO + 12), (GEO + 12, GEO + 16)))
        assert du <= 1e-4 * max(1.0, mu) and dp <= 1e-5, ("page", b)
    m.graph.close()


# ---- 6. the dense layer -----------------------------------------------------------------------------------------------------------------
def test_dense_layer_of_300_columns_over_64_and_256_channels_stays_inside_the_fma_chain_bound():
    """seeded compression layers 300 wide (the column loop passes 256) over down_2 (64) and down_4 (256) of a feat_root 16 backbone: the
    features against float64 relu(b + v @ W) on the exact maxima v.  The kernel's sum is a chain of C fused multiply-adds behind the bias
    and the ReLU is 1-Lipschitz, so |err| <= (C + 2) * 2^-24 * (|b| + |v| @ |W|) per element; the worst ratio to that bound is printed."""
    m = _Model([D2, D4], backbone={"feat_root": 16}, identity=False, dims=[300, 300])
    assert m.C == [64, 256]
    regions, npts = _regions(3)
    _, u, maps = m.forward(_image((96, 80)), regions, npts)
    assert u.shape == (len(npts), GEO + 600) and [fm.shape for fm in maps] == [(24, 20, 64), (6, 5, 256)]
    col = GEO
    for i, (fm, C) in enumerate(zip(maps, m.C)):
        v = _roi_max(fm, _rects(regions, npts, fm.shape[0], fm.shape[1])).astype(np.float64)
        W = m.w[f"visual_node_feature_compression_fm_{i}/dense/weights"].astype(np.float64)
        b = m.w[f"visual_node_feature_compression_fm_{i}/dense/bias"].astype(np.float64)
        ref = np.maximum(b + v @ W, 0)
        bound = (C + 2) * 2.0 ** -24 * (np.abs(b) + np.abs(v) @ np.abs(W))
        got = u[:, col:col + 300].astype(np.float64)
        ratio = float((np.abs(got - ref) / bound).max())
        print(f"dense layer, C = {C}: worst |err| / bound = {ratio:.4f} (max|err| {float(np.abs(got - ref).max()):.3e}, max|ref| {float(ref.max()):.3f})")
        assert (ref > 0).any() and (ref == 0).any() and (bound > 0).all()
        assert (np.abs(got - ref) <= bound).all(), (i, ratio)
        col += 300
    m.graph.close()
