"""GPU parity: HIP GNN (through the C ABI) vs the numpy oracle on the same seeded inputs.

Integer work (edge correction) is bit-exact; probabilities/hidden states within 1e-5."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-5


def _setup(seed=99, **cfg_kw):
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    from citlab_article_separation_new_amd.gnn_io import GnnGraph
    cfg = GnnConfig(**cfg_kw)
    w = init_gnn_weights(cfg, seed, bias_jitter=0.05)
    return cfg, w, GnnGraph(w, cfg)


def _random_graph(rng, N, E, node_dim=7, edge_dim=2, dup=True):
    edges = rng.integers(0, N, size=(E, 2)).astype(np.int32)       # duplicates, reversed duplicates, self loops
    if dup and E > 4:
        edges[1] = edges[0]
        edges[2] = edges[0][::-1]
        edges[3] = [min(3, N - 1), min(3, N - 1)]
    u = rng.random((N, node_dim), dtype=np.float32)
    ef = rng.random((E, edge_dim), dtype=np.float32)
    return edges, u, ef


FILL_GRID_CAP, PRE_GRID_CAP = 2048, 1024       # blocks of 256 threads: edge_table_kernel / gnn_pair_pre_kernel stride over what lies beyond


@pytest.mark.parametrize("N,E", [(4, 5), (12, 30), (50, 400), (200, 10000), (333, 2000), (3, 0), (800, 300000)])
def test_edge_correction_bit_exact(N, E):
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup()
    assert (2 * E > FILL_GRID_CAP * 256) == (E == 300000)          # the last case alone has fed entries beyond the fill launch's grid
    rng = np.random.default_rng(N * 7 + E)
    edges, u, ef = _random_graph(rng, N, E)
    want_e, want_f = gnn_oracle.correct_edges(edges, ef, N, True)
    got_e, got_f = gnn_io.correct_edges(graph, N, edges, ef)
    assert np.array_equal(got_e, want_e)
    if E:
        assert np.array_equal(got_f, want_f)
    graph.close()


def test_edge_correction_directed():
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup(undirected_graph=False)
    rng = np.random.default_rng(5)
    edges, u, ef = _random_graph(rng, 20, 90)
    want_e, want_f = gnn_oracle.correct_edges(edges, ef, 20, False)
    got_e, got_f = gnn_io.correct_edges(graph, 20, edges, ef)
    assert np.array_equal(got_e, want_e) and np.array_equal(got_f, want_f)
    graph.close()


@pytest.mark.parametrize("N,E", [(4, 5), (12, 30), (50, 400), (200, 10000), (77, 150)])
def test_probabilities_match_oracle(N, E):
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup()
    rng = np.random.default_rng(N + E)
    edges, u, ef = _random_graph(rng, N, E)
    want, want_h = gnn_oracle.forward(N, edges, u, ef, None, w, cfg, dtype=np.float64, return_hidden=True)
    got = gnn_io.gnn_forward(graph, N, edges, u, ef, None)
    got_h = gnn_io.gnn_hidden(graph, N)
    assert got.shape == (N * N, 2)
    assert float(np.abs(got_h - want_h).max()) <= PROB_TOL
    assert float(np.abs(got - want).max()) <= PROB_TOL
    graph.close()


@pytest.mark.parametrize("kw", [dict(), dict(use_attention=True, num_attention_heads=2)], ids=["default", "attention2"])
def test_probabilities_match_oracle_beyond_the_per_node_grid(kw):
    """N = 4200: the classifier's per-node first layer (gnn_pair_pre_kernel) has N x 64 > 1024 x 256 terms and strides over its capped grid; with
    attention the page has 183 interaction chunks of 23 target nodes.  500 listed relations keep the pair part small."""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup(**kw)
    N, E = 4200, 8000
    assert N * cfg.classifier_hidden[0] > PRE_GRID_CAP * 256
    assert 100000 // N == 23 and -(-N // 23) == 183
    rng = np.random.default_rng(N + E)
    edges, u, ef = _random_graph(rng, N, E)
    rel = rng.integers(0, N, size=(500, 2)).astype(np.int32)
    want, want_h = gnn_oracle.forward(N, edges, u, ef, rel, w, cfg, dtype=np.float64, return_hidden=True)
    got = gnn_io.gnn_forward(graph, N, edges, u, ef, rel)
    got_h = gnn_io.gnn_hidden(graph, N)
    err, err_h = float(np.abs(got - want).max()), float(np.abs(got_h - want_h).max())
    print(f"{kw}: max|p - oracle| = {err:.3e}, max|h - oracle| = {err_h:.3e}")
    assert got.shape == (500, 2) and err_h <= PROB_TOL and err <= PROB_TOL
    graph.close()


def test_c4_synthetic_graph_and_session_interface():
    """BASELINE config 4 shape through the reference's sess.run-by-tensor-name interface."""
    from citlab_article_separation_new_amd import gnn_io, synth
    from oracle import gnn_oracle
    cfg, w, graph = _setup(seed=1234)
    g = synth.synth_graph(0)
    N = g["num_nodes"]
    rel = gnn_oracle.build_full_relations(N)
    feed = {
        "num_nodes:0": np.array([N], np.int32),
        "num_interacting_nodes:0": np.array([g["interacting_nodes"].shape[0]], np.int32),
        "interacting_nodes:0": g["interacting_nodes"][None],
        "node_features:0": g["node_features"][None],
        "edge_features:0": g["edge_features"][None],
        "relations_to_consider_belong_to_same_instance:0": rel[None],
    }
    sess = gnn_io.GnnSession(graph, "0")
    out = sess.run("output_belong_to_same_instance:0", feed_dict=feed)
    assert out.shape == (1, N * N, 2)
    want = gnn_oracle.forward(N, g["interacting_nodes"], g["node_features"], g["edge_features"], rel, w, cfg)
    ce, _ = gnn_oracle.correct_edges(g["interacting_nodes"], g["edge_features"], N, True)
    assert ce.shape[0] == 20000
    assert float(np.abs(out[0] - want).max()) <= PROB_TOL
    with pytest.raises(KeyError):
        sess.run("no_such_node:0", feed_dict=feed)
    with pytest.raises(KeyError):
        sess.run("output_belong_to_same_instance:0", feed_dict={**feed, "bogus:0": 1})
    graph.close()


def test_relation_subset_and_isolated_nodes():
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup()
    rng = np.random.default_rng(3)
    N = 30
    edges = rng.integers(0, 10, size=(40, 2)).astype(np.int32)      # nodes 10..29 are isolated (x = 0)
    u = rng.random((N, 7), dtype=np.float32)
    ef = rng.random((40, 2), dtype=np.float32)
    rel = rng.integers(0, N, size=(123, 2)).astype(np.int32)
    want = gnn_oracle.forward(N, edges, u, ef, rel, w, cfg, dtype=np.float64)
    got = gnn_io.gnn_forward(graph, N, edges, u, ef, rel)
    assert float(np.abs(got - want).max()) <= PROB_TOL
    graph.close()


def test_permutation_equivariance():
    """Relabelling the nodes permutes the confidence matrix accordingly (property test at full C4 size)."""
    from citlab_article_separation_new_amd import gnn_io, synth
    cfg, w, graph = _setup(seed=1234)
    g = synth.synth_graph(1)
    N = g["num_nodes"]
    p0 = gnn_io.gnn_forward(graph, N, g["interacting_nodes"], g["node_features"], g["edge_features"])[:, 1].reshape(N, N)
    perm = np.random.default_rng(0).permutation(N)
    inv = np.argsort(perm)
    edges2 = inv[g["interacting_nodes"]].astype(np.int32)          # node i becomes inv[i]
    u2 = g["node_features"][perm]
    p1 = gnn_io.gnn_forward(graph, N, edges2, u2, g["edge_features"])[:, 1].reshape(N, N)
    assert float(np.abs(p1 - p0[np.ix_(perm, perm)]).max()) <= 2e-5
    graph.close()


@pytest.mark.parametrize("kw,mode", [
    (dict(), "factored"),
    (dict(node_feature_dim=20), "factored"),                                   # wide node features without an image
    (dict(node_feature_dim=55, edge_feature_dim=4), "factored"),
    (dict(node_feature_dim=9, edge_feature_dim=0), "factored"),
    (dict(hidden_dim=16, interaction_dim=24, interaction_hidden=[40]), "generic"),
    (dict(hidden_dim=48, interaction_dim=32, interaction_hidden=[32], edge_feature_dim=5), "generic"),
    (dict(classifier_hidden=[48, 20], num_classes=3), "factored"),      # generic pair classifier
    # graph_gnn.py:23,158-166 output_type: h += x W / the classifier pairs up [h | x]
    (dict(output_type="add_final_hidden_and_input"), "factored"),
    (dict(output_type="concat_final_hidden_and_input"), "factored"),
    (dict(output_type="concat_final_hidden_and_input", node_feature_dim=15, compress_node_feature_dim=6, hidden_dim=24,
          interaction_dim=20, interaction_hidden=[28]), "generic"),            # x = the features as FED, before compress_input
    (dict(output_type="add_final_hidden_and_input", node_feature_dim=20, classifier_hidden=[40, 12]), "factored"),
    # message_fn_chunk.py:35-41,199-245: learned attention over the in-edges, one / several heads, both merge types; directed graph:
    # the (to, from) <-> (from, to) pairing of the reference is then not the reverse edge
    (dict(use_attention=True), "generic"),
    (dict(use_attention=True, num_attention_heads=4), "generic"),
    (dict(use_attention=True, num_attention_heads=2, multihead_attention_merge_type="average", attention_hidden=[12]), "generic"),
    (dict(use_attention=True, num_attention_heads=2, undirected_graph=False, hidden_dim=24, interaction_dim=20,
          interaction_hidden=[28], num_transition_steps=2), "generic"),
    # round 4 -- message_fn_chunk.py:16,57-62 aggregation_type='max' (tf.sparse.reduce_max), with and without attention
    (dict(aggregation_type="max"), "generic"),
    (dict(aggregation_type="max", undirected_graph=False, node_feature_dim=20), "generic"),
    (dict(aggregation_type="max", use_attention=True, num_attention_heads=2), "generic"),
    (dict(aggregation_type="max", use_attention=True, num_attention_heads=2, multihead_attention_merge_type="average"), "generic"),
    # num_hidden_units_* are lists (message_fn_chunk.py:24,40; graph_relation.py:196): several hidden layers per MLP
    (dict(interaction_hidden=[32, 32]), "generic"),
    (dict(interaction_hidden=[40, 24, 16], classifier_hidden=[48, 20, 12]), "generic"),
    (dict(classifier_hidden=[48]), "factored"),                          # one hidden layer
    (dict(classifier_hidden=[64, 32, 16, 8], num_classes=3, node_feature_dim=20), "factored"),
    (dict(use_attention=True, num_attention_heads=2, attention_hidden=[16, 8], interaction_hidden=[24, 20]), "generic"),
    # update_fn_lstm.py:13-16,43-50: the gates read x alone / x + h / x + u
    (dict(incorporate_node_input_features_in_update=False), "generic"),
    (dict(incorporate_hidden_features_in_update=False), "generic"),
    (dict(incorporate_hidden_features_in_update=False, incorporate_node_input_features_in_update=False, aggregation_type="max"), "generic"),
])
def test_hyper_parameters_other_than_the_defaults(kw, mode):
    """message_fn_chunk.py:13-40, trainer_rel.py:15-17: every width is a free parameter of the reference; the engine picks
    the fused MFMA step (round 6: its factored form) where the widths allow it and plain FMA kernels elsewhere -- all against the oracle."""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup(seed=17, **kw)
    assert gnn_io.step_mode(graph) == mode
    rng = np.random.default_rng(len(str(kw)))
    N, E = 60, 500
    edges, u, ef = _random_graph(rng, N, E, node_dim=cfg.node_feature_dim, edge_dim=max(cfg.edge_feature_dim, 1))
    ef = ef if cfg.edge_feature_dim else None
    probs = gnn_io.gnn_forward(graph, N, edges, u, ef)
    ref, href = gnn_oracle.forward(N, edges, u, ef, None, w, cfg, return_hidden=True)
    h = gnn_io.gnn_hidden(graph, N)
    assert h.shape == href.shape and float(np.abs(h - href).max()) <= PROB_TOL
    assert probs.shape == (N * N, cfg.num_classes) and float(np.abs(probs - ref).max()) <= PROB_TOL
    graph.close()


@pytest.mark.parametrize("N,E,undirected", [(317, 900, True), (400, 2500, True), (523, 1500, False)])
def test_attention_nets_on_graphs_of_several_interaction_chunks(N, E, undirected):
    """message_fn_chunk.py:76-110: the reference runs the message function per chunk of 100000 // N target nodes and pairs the attention
    values with the interactions INSIDE a chunk; beyond 316 nodes there are several chunks (N = 400: 250 nodes per chunk)"""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup(seed=5, use_attention=True, num_attention_heads=2, undirected_graph=undirected)
    rng = np.random.default_rng(N)
    edges, u, ef = _random_graph(rng, N, E)
    rel = rng.integers(0, N, size=(3000, 2)).astype(np.int32)
    probs = gnn_io.gnn_forward(graph, N, edges, u, ef, rel)
    ref = gnn_oracle.forward(N, edges, u, ef, rel, w, cfg)
    assert probs.shape == ref.shape and float(np.abs(probs - ref).max()) <= PROB_TOL
    graph.close()


def test_index_arrays_are_validated_at_the_host_entry():
    """the reference's gather ops raise on an index outside the node range; so does the host entry (the device entry
    documents what it does instead: edge ignored, NaN for the relation)"""
    from citlab_article_separation_new_amd import _lib, gnn_io
    cfg, w, graph = _setup()
    rng = np.random.default_rng(1)
    edges, u, ef = _random_graph(rng, 10, 20)
    bad = edges.copy()
    bad[7, 1] = 10
    with pytest.raises(_lib.AsepError, match="interacting_nodes"):
        gnn_io.gnn_forward(graph, 10, bad, u, ef)
    rel = np.array([[0, 1], [2, -1]], np.int32)
    with pytest.raises(_lib.AsepError, match="relations"):
        gnn_io.gnn_forward(graph, 10, edges, u, ef, rel)
    ok = gnn_io.gnn_forward(graph, 10, edges, u, ef, np.array([[0, 1], [9, 9]], np.int32))
    assert ok.shape == (2, 2) and np.isfinite(ok).all()
    graph.close()


@pytest.mark.parametrize("kw,unfactored", [
    (dict(), "mfma_registers"),
    (dict(node_feature_dim=55, edge_feature_dim=4), "mfma_lds"),
    (dict(node_feature_dim=9, edge_feature_dim=0, num_transition_steps=1), "mfma_lds"),
    (dict(node_feature_dim=20, undirected_graph=False, num_transition_steps=5), "mfma_lds"),
])
def test_factored_step_against_the_unfactored_kernels_and_the_fp64_oracle(kw, unfactored, monkeypatch):
    """round 6: the edge MLP's first layer as per-node terms + a per-edge constant + a K = 32 per-edge-and-step term
    (message_fn_chunk.py:266-363 is linear in u_from, u_to, u_to - u_from, h_from, h_to, h_to - h_from).  Three implementations of the same
    arithmetic on one graph with isolated nodes, duplicate / reversed edges and in-degrees from 0 to > 64: the factored step (default), the
    unfactored fused kernels (ASEP_GNN_FACTOR=0) and the generic FMA kernels (ASEP_GNN_STEP=0) -- each within 1e-5 of the fp64 oracle."""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    rng = np.random.default_rng(11)
    N, E = 90, 1400
    outs = {}
    for name, env in (("factored", {}), (unfactored, {"ASEP_GNN_FACTOR": "0"}), ("generic", {"ASEP_GNN_STEP": "0"})):
        for k in ("ASEP_GNN_FACTOR", "ASEP_GNN_STEP"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)                          # read when the model is loaded
        cfg, w, graph = _setup(seed=23, **kw)
        assert gnn_io.step_mode(graph) == name
        if not outs:
            edges, u, ef = _random_graph(rng, N, E, node_dim=cfg.node_feature_dim, edge_dim=max(cfg.edge_feature_dim, 1))
            edges[:200, 1] = 5                                # one target with a long in-edge list (several tiles per wave)
            edges[edges == 17] = 3                            # node 17 isolated
            ef = ef if cfg.edge_feature_dim else None
            ref, href = gnn_oracle.forward(N, edges, u, ef, None, w, cfg, dtype=np.float64, return_hidden=True)
        probs = gnn_io.gnn_forward(graph, N, edges, u, ef)
        h = gnn_io.gnn_hidden(graph, N)
        assert float(np.abs(h - href).max()) <= PROB_TOL and float(np.abs(probs - ref).max()) <= PROB_TOL, name
        outs[name] = (probs, h)
        graph.close()
    assert float(np.abs(outs["factored"][1] - outs[unfactored][1]).max()) <= 5e-6
