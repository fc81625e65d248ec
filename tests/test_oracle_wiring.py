"""The CPU oracles' WIRING against the reference's own model code (CPU, no GPU).

tests/golden/model_wiring_aru.npz and model_wiring_gnn.npz hold what the reference's graph-definition Python -- ARU_v1_CNN.infer and
GraphGNN.infer -- computed when it was executed on an eager float64 stand-in for TensorFlow (tests/golden/make_model_wiring_golden.py,
tf_eager_standin.py; this test reads only the fixtures).  Here the hand-written oracles, which every GPU parity test of this project is
measured against, have to reproduce those tensors from the same inputs and variables, and this project's variable inventories
(weights.py, tests/tf_aru_graph.py, tests/tf_gnn_graph.py) have to name exactly the variables the reference created.

Gate: max |d| <= 1e-6 * max(1, max |golden|) per tensor -- derived, not measured: the fixtures are float32 (6e-8 relative), float64
evaluation of sums of <= 2304 terms over some forty layers adds many orders less.

Not pinned by this (see tf_eager_standin.py): the semantics of the TensorFlow ops, restated there a third time; the pair classifier
('Classification/...', created by graph_relation.py, which the maker does not run -- its names are left out of the name equality);
the frozen nets.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import model_wiring_cases as mc  # noqa: E402
from citlab_article_separation_new_amd.config import AruConfig, GnnConfig  # noqa: E402
from citlab_article_separation_new_amd.weights import init_aru_weights, init_gnn_weights  # noqa: E402
from oracle import aru_oracle, gnn_oracle  # noqa: E402


def _load(family):
    z = np.load(os.path.join(HERE, "golden", f"model_wiring_{family}.npz"))
    meta = json.loads(bytes(z["meta"]).decode("utf-8"))
    return z, meta, {c["name"]: c for c in meta["cases"]}


ARU_Z, ARU_META, ARU = _load("aru")
GNN_Z, GNN_META, GNN = _load("gnn")


def test_the_fixtures_hold_the_case_list():
    assert [c["name"] for c in ARU_META["cases"]] == [c["name"] for c in mc.ARU_CASES]
    assert [c["name"] for c in GNN_META["cases"]] == [c["name"] for c in mc.GNN_CASES]
    for case in mc.ARU_CASES:
        assert ARU[case["name"]]["cfg"] == case["cfg"]
        assert np.array_equal(ARU_Z[case["name"] + "::image"], mc.aru_image(case))
    for case in mc.GNN_CASES:
        assert GNN[case["name"]]["cfg"] == case["cfg"]
    # a variant the reference does not build is one the config refuses too
    assert [s["name"] for s in ARU_META["skipped"]] == [c["name"] for c in mc.ARU_REFUSED]
    for s in ARU_META["skipped"]:
        with pytest.raises(ValueError):
            AruConfig(**s["cfg"]).check_channels()
    for case in mc.ARU_CASES:
        AruConfig(**case["cfg"]).check_channels()


# ---- ARU-Net -----------------------------------------------------------------------------------------------------------------------
def _aru_inputs(name):
    rec = ARU[name]
    cfg = AruConfig(apply_softmax=False, **rec["cfg"])
    w = {n: mc.variable_value(n, shp) for n, shp in rec["variables"]}      # the values the maker gave the reference, by name and shape
    golden = {ep: ARU_Z[f"{name}::ep::{ep}"] for ep in rec["end_points"]}
    return cfg, ARU_Z[name + "::image"], w, golden


def _aru_run(which, image, w, cfg):
    import torch
    if which == "numpy":
        out, inter = aru_oracle.forward_numpy(image, w, cfg, dtype=np.float64, return_intermediates=True, pool_end_points=True)
    else:
        out, inter = aru_oracle.forward_torch(image, w, cfg, dtype=torch.float64, return_intermediates=True, pool_end_points=True)
    assert np.array_equal(out, inter["logits"])
    return inter


def _worst(golden, got):
    """the largest max |d| / gate over the stored tensors, every one present and of equal shape"""
    worst = 0.0
    for name, want in golden.items():
        assert name in got, f"the oracle has no end point {name}"
        have = np.asarray(got[name], np.float64)
        assert have.shape == want.shape, (name, have.shape, want.shape)
        worst = max(worst, float(np.max(np.abs(have - want))) / mc.gate(want))
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in mc.ARU_CASES])
def test_aru_oracle_reproduces_the_reference_graph(name):
    cfg, image, w, golden = _aru_inputs(name)
    assert len(golden) > 3 and "logits" in golden
    # names and shapes: this project's inventory == the variables the reference created
    ours = init_aru_weights(cfg, 1)
    assert {k: tuple(v.shape) for k, v in ours.items()} == {n: tuple(shp) for n, shp in ARU[name]["variables"]}
    for which in ("numpy", "torch"):
        worst = _worst(golden, _aru_run(which, image, w, cfg))
        print(f"{name} {which}: worst max|d| / gate = {worst:.3g} over {len(golden)} end points")
        assert worst <= 1.0, (which, worst)


# ---- GNN ---------------------------------------------------------------------------------------------------------------------------
def _gnn_inputs(name):
    rec = GNN[name]
    cfg = GnnConfig(**rec["cfg"])
    w = {n: GNN_Z[f"{name}::var::{n}"] for n, _ in rec["variables"]}
    for n, shp in rec["variables"]:
        assert w[n].shape == tuple(shp) and np.array_equal(w[n], mc.variable_value(n, shp))
    graph = {k: GNN_Z[f"{name}::{k}"] for k in ("interacting_nodes", "node_features")}
    graph["edge_features"] = GNN_Z[f"{name}::edge_features"] if f"{name}::edge_features" in GNN_Z.files else None
    return cfg, rec["num_nodes"], graph, w, GNN_Z[f"{name}::gnn_node_features"]


def _gnn_run(cfg, N, graph, w):
    full = dict(w)
    for k, v in init_gnn_weights(cfg, 1).items():          # the pair classifier is not part of GraphGNN: any weights do
        if k.startswith("Classification/"):
            full[k] = v
    _, h, node_out = gnn_oracle.forward(N, graph["interacting_nodes"], graph["node_features"], graph["edge_features"],
                                        np.array([[0, 1]]), full, cfg, dtype=np.float64, return_hidden=True, return_node_output=True)
    if cfg.output_type == "hidden":
        assert node_out is h
    return node_out


@pytest.mark.parametrize("name", [c["name"] for c in mc.GNN_CASES])
def test_gnn_oracle_reproduces_the_reference_graph(name):
    cfg, N, graph, w, golden = _gnn_inputs(name)
    ours = {k: tuple(v.shape) for k, v in init_gnn_weights(cfg, 1).items() if not k.startswith("Classification/")}
    assert ours == {n: tuple(shp) for n, shp in GNN[name]["variables"]}
    assert all(n.startswith("GraphLSTM1/") for n in ours)
    worst = _worst({"gnn_node_features": golden}, {"gnn_node_features": _gnn_run(cfg, N, graph, w)})
    print(f"{name}: max|d| / gate = {worst:.3g}")
    assert worst <= 1.0


def test_the_big_gnn_case_spans_two_chunks():
    rec = GNN["attention_two_chunks"]
    per_chunk = 100000 // rec["num_nodes"]
    to = GNN_Z["attention_two_chunks::interacting_nodes"][:, 1]
    assert per_chunk < rec["num_nodes"] and (to < per_chunk).any() and (to >= per_chunk).any()


# ---- the variable names the frozen-graph builders encode (what pb_import.py is tested on) ---------------------------------------
def _variables_of(nodes):
    """Const nodes that are read through a '<name>/read' Identity: the frozen variables"""
    names = {n.name for n in nodes}
    return {n.name for n in nodes if n.op == "Const" and n.name + "/read" in names}


@pytest.mark.parametrize("name", [c["name"] for c in mc.ARU_CASES])
def test_tf_aru_graph_encodes_the_reference_variable_names(name):
    pytest.importorskip("google.protobuf")
    import tf_aru_graph
    import tf_graphdef_proto as tp
    cfg, _, w, _ = _aru_inputs(name)
    b = tf_aru_graph.AruGraphBuilder(tp.build_messages(), w, cfg, output_softmax=False)
    b.build()
    consts = {n.name: n for n in b.nodes if n.op == "Const"}
    got = _variables_of(b.nodes)
    assert got == {n for n, _ in ARU[name]["variables"]}
    for n, shp in ARU[name]["variables"]:
        assert [d.size for d in consts[n].attr["value"].tensor.tensor_shape.dim] == list(shp), n


@pytest.mark.parametrize("name", [c["name"] for c in mc.GNN_CASES])
def test_tf_gnn_graph_encodes_the_reference_variable_names(name):
    pytest.importorskip("google.protobuf")
    import tf_gnn_graph
    import tf_graphdef_proto as tp
    cfg, _, _, w, _ = _gnn_inputs(name)
    full = dict(init_gnn_weights(cfg, 1))
    full.update(w)
    g = tf_gnn_graph.build(tp.build_messages(), full, cfg.num_transition_steps, prefix="", aggregation=cfg.aggregation_type,
                           merge_concat=cfg.multihead_attention_merge_type == "concat",
                           lstm_inputs=(cfg.incorporate_hidden_features_in_update, cfg.incorporate_node_input_features_in_update))
    got = {n for n in _variables_of(g.node) if not n.startswith("Classification/")}
    assert got == {n for n, _ in GNN[name]["variables"]}


# ---- the gate can fail ---------------------------------------------------------------------------------------------------------------
def _swap_rows(a, first, second):
    """exchange two equally long row blocks (slices of axis -2) of a filter / weight matrix"""
    out = a.copy()
    out[..., first, :], out[..., second, :] = a[..., second, :], a[..., first, :]
    return out


def _mutations():
    def concat_order():
        cfg, image, w, golden = _aru_inputs("aru_default_relu")
        k = "aru_net/featMapG/unet_up_0/conv1/weights"
        half = w[k].shape[2] // 2
        w[k] = _swap_rows(w[k], slice(0, half), slice(half, 2 * half))
        return _worst(golden, _aru_run("numpy", image, w, cfg)), _worst(golden, _aru_run("torch", image, w, cfg))

    def activation():
        cfg, image, w, golden = _aru_inputs("ru_elu")
        assert cfg.activation_name == "elu"
        cfg.activation_name = "relu"
        return _worst(golden, _aru_run("numpy", image, w, cfg)), _worst(golden, _aru_run("torch", image, w, cfg))

    def lstm_gates():
        cfg, N, graph, w, golden = _gnn_inputs("gnn_defaults")
        a, b = (f"{gnn_oracle.UPD}/{g}_activation/dense/" for g in ("ingate", "forgetgate"))
        for leaf in ("weights", "bias"):
            w[a + leaf], w[b + leaf] = w[b + leaf], w[a + leaf]
        return (_worst({"h": golden}, {"h": _gnn_run(cfg, N, graph, w)}),)

    def edge_mlp_blocks():
        cfg, N, graph, w, golden = _gnn_inputs("gnn_defaults")
        k = f"{gnn_oracle.MSG}/fully_connected_layer_h1/weights"
        u = cfg.u_dim
        w[k] = _swap_rows(w[k], slice(0, u), slice(u, 2 * u))                # u_from <-> u_to
        return (_worst({"h": golden}, {"h": _gnn_run(cfg, N, graph, w)}),)

    return {"concat_order_of_unet_up_0": concat_order, "relu_for_elu": activation, "ingate_for_forgetgate": lstm_gates,
            "u_from_for_u_to": edge_mlp_blocks}


@pytest.mark.parametrize("mutation", sorted(_mutations()))
def test_a_wiring_mistake_misses_the_gate_by_three_orders(mutation):
    for worst in _mutations()[mutation]():
        print(f"{mutation}: worst max|d| / gate = {worst:.3g}")
        assert worst >= 1000.0, (mutation, worst)
