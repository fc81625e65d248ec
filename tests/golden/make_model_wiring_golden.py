"""Goldens of the models' WIRING (tests/golden/model_wiring_aru.npz, model_wiring_gnn.npz): the reference's own graph-definition code,
executed.

The reference's backbones/ARU_v1.py, gnn/model/graph_util/layers.py, gnn/model/graph/graph_gnn.py, message_fn_chunk.py, update_fn_lstm.py and
the edge correction of graph_util/misc.py are imported through ref_import.install_stubs() with tf_eager_standin.py in the place of
``tensorflow`` and run on the cases of model_wiring_cases.py: ``ARU_v1_CNN.infer`` on a page, ``GraphGNN.infer`` (under the variable scope
'GraphLSTM1' that graph_relation.py:181 opens around it) on a graph.  Every variable the reference's code asks for gets its value from
model_wiring_cases.variable_value(name, shape).

Stored per ARU case: the page, the (name, shape) list in creation order, every tensor-valued end point and the logits.
Stored per GNN case: the fed graph, the (name, shape) list, every variable's value, ``gnn_node_features``.
Stored once per file: ``skipped`` -- variants the reference does not build (with its error) -- and the case list.
All arrays are float32 / int32; the files are zip archives of .npy members written with fixed time stamps, so that

    python tests/golden/make_model_wiring_golden.py --check

can regenerate them in memory and compare with the committed files byte for byte.  What this does NOT pin is said in
tf_eager_standin.py: the ops' semantics are restated there; the frozen nets and TensorFlow's kernels are not reachable from here.

Run:  python tests/golden/make_model_wiring_golden.py [--check]
"""
import io
import json
import logging
import os
import sys
import types
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402
import tf_eager_standin as standin  # noqa: E402

ref_import.install_stubs()
tf = standin.install()

import numpy as np  # noqa: E402

import model_wiring_cases as mc  # noqa: E402

FILES = {"aru": "model_wiring_aru.npz", "gnn": "model_wiring_gnn.npz"}
SIZE_LIMIT = os.path.getsize(os.path.join(HERE, "host_goldens.json"))       # the largest fixture committed so far


def import_reference():
    """the reference's modules; ARU_v1.py imports its siblings as ``gnn.model...`` / ``utils.flags``: aliases of the same modules"""
    import importlib
    saved = sys.argv
    sys.argv = ["make_model_wiring_golden.py"]
    try:
        import article_separation.gnn as gnn_pkg
        import article_separation.gnn.model as model_pkg
        import article_separation.gnn.model.graph_util as util_pkg
        import python_util.basic.flags as rflags
        from article_separation.gnn.model import model_base
        from article_separation.gnn.model.graph_util import layers
        from article_separation.gnn.model.graph import graph_gnn
    finally:
        sys.argv = saved
    utils = types.ModuleType("utils")
    utils.flags = rflags
    for name, mod in (("gnn", gnn_pkg), ("gnn.model", model_pkg), ("gnn.model.model_base", model_base), ("gnn.model.graph_util", util_pkg),
                      ("gnn.model.graph_util.layers", layers), ("utils", utils), ("utils.flags", rflags)):
        sys.modules[name] = mod
    aru = importlib.import_module("article_separation.backbones.ARU_v1")
    return aru.ARU_v1_CNN, graph_gnn.GraphGNN


class Source:
    """what get_variable draws from: name -> value, filled on first request"""
    def __init__(self):
        self.values = {}

    def __call__(self, name, shape):
        if name not in self.values:
            self.values[name] = mc.variable_value(name, shape)
        return self.values[name].astype(np.float64)


def run_aru(ARU, case):
    cfg = case["cfg"]
    backbone = {"graph": cfg.get("graph", "ARU")}
    for ours, theirs in (("mvn", "mvn"), ("feat_root", "featRoot"), ("num_scales_att", "num_scales_att"), ("scale_space_num", "scale_space_num"),
                         ("res_depth", "res_depth"), ("filter_size", "filter_size"), ("pool_size", "pool_size"),
                         ("activation_name", "activation_name")):
        if ours in cfg:
            backbone[theirs] = cfg[ours]
    flags = types.SimpleNamespace(graph_backbone_params=backbone, channels=cfg.get("channels", 1), n_classes=cfg.get("n_classes", 2))
    image = mc.aru_image(case)
    src = Source()
    standin.VARIABLES.reset(src)
    net = ARU({"flags": flags})
    logits, end_points = net.infer(tf.Tensor(image[None].astype(np.float64)), is_training=False)
    out = {"image": image}
    tensors = {k: v for k, v in end_points.items() if isinstance(v, standin.Tensor)}
    tensors["logits"] = logits
    for k, v in tensors.items():
        assert v.numpy().shape[0] == 1
        out["ep::" + k] = v.numpy()[0].astype(np.float32)
    names = [[k, list(v.shape)] for k, v in standin.VARIABLES.created.items()]
    return out, names


def run_gnn(GNN, case):
    cfg = case["cfg"]
    g = mc.gnn_graph(case)
    gnn_params = {k: cfg[k] for k in ("num_transition_steps", "compress_node_feature_dim", "undirected_graph", "output_type") if k in cfg}
    msg = {}
    for ours, theirs in (("aggregation_type", "aggregation_type"), ("interaction_dim", "interaction_feature_dim"),
                         ("interaction_hidden", "num_hidden_units_interaction_fct"), ("use_attention", "use_attention"),
                         ("num_attention_heads", "num_attention_heads"), ("multihead_attention_merge_type", "multihead_attention_merge_type"),
                         ("attention_hidden", "num_hidden_units_attention_fct")):
        if ours in cfg:
            msg[theirs] = cfg[ours]
    upd = {}
    for ours, theirs in (("hidden_dim", "hidden_node_feature_dim"), ("incorporate_hidden_features_in_update",) * 2,
                         ("incorporate_node_input_features_in_update",) * 2):
        if ours in cfg:
            upd[theirs] = cfg[ours]
    E = g["interacting_nodes"].shape[0]
    inputs = {"num_nodes": tf.Tensor(np.array([g["num_nodes"]])), "interacting_nodes": tf.Tensor(g["interacting_nodes"][None]),
              "num_interacting_nodes": tf.Tensor(np.array([E])), "node_features": tf.Tensor(g["node_features"][None].astype(np.float64))}
    if g["edge_features"] is not None:
        inputs["edge_features"] = tf.Tensor(g["edge_features"][None].astype(np.float64))
    src = Source()
    standin.VARIABLES.reset(src)
    net = GNN({"flags": types.SimpleNamespace()}, gnn_params, msg, upd)
    with tf.compat.v1.variable_scope("GraphLSTM1"):                      # graph_relation.py:181
        res = net.infer(inputs, is_training=False)
    feats = res["gnn_node_features"].numpy()
    assert feats.shape[0] == 1
    out = {"interacting_nodes": g["interacting_nodes"], "node_features": g["node_features"], "gnn_node_features": feats[0].astype(np.float32)}
    if g["edge_features"] is not None:
        out["edge_features"] = g["edge_features"]
    for k, v in standin.VARIABLES.created.items():
        out["var::" + k] = src.values[k]
    names = [[k, list(v.shape)] for k, v in standin.VARIABLES.created.items()]
    return out, names


def pack(arrays, meta):
    """a .npz (zip of .npy members) with fixed time stamps; `meta` travels as the bytes of a JSON text"""
    arrays = dict(arrays)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True, separators=(",", ":")).encode("utf-8"), dtype=np.uint8)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue(), compresslevel=9)
    return buf.getvalue()


def generate():
    standin.self_check()
    ARU, GNN = import_reference()
    files = {}
    arrays, meta = {}, {"cases": [], "skipped": []}
    for case in mc.ARU_CASES:
        out, names = run_aru(ARU, case)
        arrays.update({f"{case['name']}::{k}": v for k, v in out.items()})
        meta["cases"].append({"name": case["name"], "cfg": case["cfg"], "variables": names,
                              "end_points": sorted(k[4:] for k in out if k.startswith("ep::"))})
    for case in mc.ARU_REFUSED:
        try:
            run_aru(ARU, case)
        except ValueError as e:
            meta["skipped"].append({"name": case["name"], "cfg": case["cfg"], "reason": f"the reference's graph does not build: {e}"})
        else:
            raise SystemExit(f"{case['name']}: the reference builds this variant -- make it a case")
    files["aru"] = pack(arrays, meta)
    arrays, meta = {}, {"cases": [], "skipped": []}
    for case in mc.GNN_CASES:
        out, names = run_gnn(GNN, case)
        arrays.update({f"{case['name']}::{k}": v for k, v in out.items()})
        meta["cases"].append({"name": case["name"], "cfg": case["cfg"], "num_nodes": case.get("N", 12), "variables": names})
    files["gnn"] = pack(arrays, meta)
    standin.VARIABLES.reset(None)
    return files


def main():
    logging.getLogger().setLevel("ERROR")
    check = "--check" in sys.argv[1:]
    files = generate()
    bad = 0
    for family, data in files.items():
        path = os.path.join(HERE, FILES[family])
        if len(data) >= SIZE_LIMIT:
            raise SystemExit(f"{FILES[family]}: {len(data)} bytes, the limit is {SIZE_LIMIT}")
        if check:
            with open(path, "rb") as f:
                same = f.read() == data
            print(f"{FILES[family]}: {'reproduced byte for byte' if same else 'DIFFERS'} ({len(data)} bytes)")
            bad += not same
        else:
            with open(path, "wb") as f:
                f.write(data)
            print(path, len(data), "bytes")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
