"""Cases of the model wiring fixtures (model_wiring_aru.npz, model_wiring_gnn.npz), shared by their maker
(make_model_wiring_golden.py, which runs the reference's graph-definition code) and tests/test_oracle_wiring.py.

Everything here is a deterministic function of a name: the counter-based generator below is integer arithmetic on uint64 (splitmix64
over a CRC of the name), so the maker and the test get bit-identical numbers on any numpy version.

Variable values.  The maker hands ``variable_value(name, shape)`` to the reference's ``get_variable`` calls: N(0, 0.3 / sqrt(fan_in))-like
weights (the sum of four uniforms, scaled to that standard deviation) and biases of magnitude 0.02 .. 0.1 with either sign -- a function of
the name and shape the REFERENCE asked for and of nothing in this project.  The GNN fixture stores the values; the ARU fixture stores
the names and shapes only and the test regenerates the values from them: the default ARU-Net alone has 1.1 million weights (4.4 MB as
float32), nine times the size a fixture may have.

Widths.  ``aru_default_relu`` and ``gnn_defaults`` run at the reference's default widths.  The other cases keep every structural default
(five levels, residual depth three, three attention scales, three transition steps) but use small widths, chosen pairwise different where
the graph allows it so that a mixed-up dimension cannot go unnoticed -- the end points of eleven ARU cases at featRoot 8 would not fit the
size limit either.
"""
import zlib

import numpy as np

MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & MASK
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & MASK
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & MASK
    return z ^ (z >> np.uint64(31))


def uniform(tag, n, stream=0):
    """n float64 in [0, 1), a function of (tag, stream, index) alone"""
    key = np.uint64(zlib.crc32(tag.encode("utf-8"))) << np.uint64(32)
    idx = np.arange(n, dtype=np.uint64) * np.uint64(8) + np.uint64(stream)
    with np.errstate(over="ignore"):
        bits = _splitmix64(_splitmix64(idx ^ key))
    return (bits >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def variable_value(name, shape):
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    if len(shape) == 1:                                                  # biases: never zero, either sign
        sign = np.where(uniform(name, n, 1) < 0.5, -1.0, 1.0)
        return (sign * (0.02 + 0.08 * uniform(name, n, 0))).reshape(shape).astype(np.float32)
    fan_in = int(np.prod(shape[:-1]))
    z = (sum(uniform(name, n, s) for s in range(4)) - 2.0) * np.sqrt(3.0)   # variance 4 / 12 -> 1
    return (z * 0.3 / np.sqrt(fan_in)).reshape(shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# ARU-Net: tiny odd pages.  13 x 22 -> 7 x 11 -> 4 x 6 -> 2 x 3 -> 1 x 2 and 16 x 9 -> 8 x 5 -> 4 x 3 -> 2 x 2 -> 1 x 1: every ceil pool,
# every crop of a transposed convolution (odd and even sizes, both axes) and the upsample crops of the attention scales are taken.
# cfg: keyword arguments of AruConfig (apply_softmax stays False: the reference graph ends in the logits)
# ---------------------------------------------------------------------------------------------------------------------------
ARU_CASES = [
    {"name": "aru_default_relu", "hw": (13, 22), "cfg": {}},
    {"name": "ru_elu", "hw": (16, 9), "cfg": {"graph": "RU", "activation_name": "elu", "feat_root": 4}},
    {"name": "u_leaky", "hw": (13, 22), "cfg": {"graph": "U", "activation_name": "leaky", "feat_root": 4}},
    {"name": "aru_mvn", "hw": (16, 9), "cfg": {"mvn": True, "feat_root": 2}},
    {"name": "aru_res_depth2", "hw": (13, 22), "cfg": {"res_depth": 2, "feat_root": 2, "activation_name": "elu"}},
    {"name": "aru_scale_space3", "hw": (16, 9), "cfg": {"scale_space_num": 3, "feat_root": 4}},
    {"name": "aru_num_scales_att2", "hw": (13, 22), "cfg": {"num_scales_att": 2, "feat_root": 2, "activation_name": "leaky"}},
    {"name": "ru_feat_root16", "hw": (16, 9), "cfg": {"graph": "RU", "feat_root": 16, "scale_space_num": 3}},
    {"name": "aru_n_classes3", "hw": (13, 22), "cfg": {"n_classes": 3, "feat_root": 2}},
    {"name": "ru_rgb", "hw": (13, 22), "cfg": {"graph": "RU", "channels": 3, "feat_root": 4, "activation_name": "leaky"}},
    {"name": "u_rgb_mvn", "hw": (16, 9), "cfg": {"graph": "U", "channels": 3, "mvn": True, "feat_root": 4, "activation_name": "elu"}},
]
# a variant the maker TRIES and both sides refuse (a three-channel page in the attention graph): recorded in the fixture's `skipped`
ARU_REFUSED = [
    {"name": "aru_rgb", "hw": (13, 22), "cfg": {"graph": "ARU", "channels": 3, "feat_root": 2}},
]


def aru_image(case):
    h, w = case["hw"]
    c = case["cfg"].get("channels", 1)
    scale = 255.0 if case["cfg"].get("mvn") else 1.0                      # standardised pages are fed as 0..255
    return (uniform("image:" + case["name"], h * w * c) * scale).reshape(h, w, c).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# GNN.  cfg: keyword arguments of GnnConfig.  SMALL: every width different (node 7, edge 2, hidden 12, interaction 8, MLP 10, attention 6)
# ---------------------------------------------------------------------------------------------------------------------------
SMALL = {"hidden_dim": 12, "interaction_dim": 8, "interaction_hidden": [10], "attention_hidden": [6]}


def _small(**kw):
    out = dict(SMALL)
    out.update(kw)
    return out


GNN_CASES = [
    {"name": "gnn_defaults", "cfg": {}},
    {"name": "directed", "cfg": _small(undirected_graph=False)},
    {"name": "no_edge_features", "cfg": _small(edge_feature_dim=0)},
    {"name": "attention_1_head", "cfg": _small(use_attention=True)},
    {"name": "attention_4_heads_concat", "cfg": _small(use_attention=True, num_attention_heads=4)},
    {"name": "attention_2_heads_average", "cfg": _small(use_attention=True, num_attention_heads=2, multihead_attention_merge_type="average",
                                                        attention_hidden=[6, 5])},
    {"name": "max_aggregation", "cfg": _small(aggregation_type="max")},
    {"name": "max_aggregation_attention", "cfg": _small(aggregation_type="max", use_attention=True, num_attention_heads=2)},
    {"name": "interaction_hidden_3_layers", "cfg": _small(interaction_hidden=[40, 24, 16])},
    {"name": "lstm_reads_x_only", "cfg": _small(incorporate_hidden_features_in_update=False,
                                                 incorporate_node_input_features_in_update=False)},
    {"name": "compress_node_features", "cfg": _small(compress_node_feature_dim=6)},
    {"name": "output_add", "cfg": _small(output_type="add_final_hidden_and_input")},
    {"name": "output_concat", "cfg": _small(output_type="concat_final_hidden_and_input", compress_node_feature_dim=5)},
    {"name": "one_step", "cfg": _small(num_transition_steps=1)},
    {"name": "five_steps", "cfg": _small(num_transition_steps=5)},
    # 100000 // 330 = 303 target nodes per chunk (message_fn_chunk.py:77): the targets 303 .. 329 form a second chunk
    {"name": "attention_two_chunks", "N": 330, "E": 400,
     "cfg": {"hidden_dim": 6, "interaction_dim": 4, "interaction_hidden": [5], "attention_hidden": [3], "use_attention": True,
             "num_attention_heads": 2}},
]


def gnn_graph(case):
    """N nodes, E fed edges: edge 1 repeats edge 0, edge 3 is edge 2 reversed, edge 4 is a self loop, node N - 1 has no edge"""
    N, E = case.get("N", 12), case.get("E", 30)
    cfg = case["cfg"]
    tag = "graph:" + case["name"]
    a = np.minimum((uniform(tag, E, 0) * (N - 1)).astype(np.int64), N - 2)
    b = np.minimum((uniform(tag, E, 1) * (N - 2)).astype(np.int64), N - 3)
    b = np.where(b >= a, b + 1, b)                                        # b != a, both below N - 1
    edges = np.stack([a, b], axis=1)
    edges[1] = edges[0]
    edges[3] = edges[2][::-1]
    edges[4] = (edges[4, 0], edges[4, 0])
    if N > 300:                                                           # both chunks of the big case get targets with several in-edges
        edges[5:25, 1] = N - 2 - (np.arange(20) % 7)
        edges[5:25, 0] = np.arange(20) * 3
    nd, ed = cfg.get("node_feature_dim", 7), cfg.get("edge_feature_dim", 2)
    out = {"num_nodes": N, "interacting_nodes": edges.astype(np.int32),
           "node_features": (uniform(tag, N * nd, 2) * 2 - 1).reshape(N, nd).astype(np.float32)}
    out["edge_features"] = (uniform(tag, E * ed, 3) * 2 - 1).reshape(E, ed).astype(np.float32) if ed else None
    assert N - 1 not in edges and len(np.unique(edges, axis=0)) < E
    return out


def gate(golden):
    """max |d| allowed against a stored tensor: 1e-6 * max(1, max |golden|).  Derived, not measured: the fixtures are float32
    (6e-8 relative); float64 evaluation of sums of <= 2304 terms over some forty layers adds many orders less."""
    g = np.asarray(golden)
    return 1e-6 * max(1.0, float(np.max(np.abs(g))) if g.size else 1.0)
