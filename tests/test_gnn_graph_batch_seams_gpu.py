"""asep_gnn_forward_batch at the seams of its page table: pages of several interaction chunks that are not first in the call, directed graphs, the
three step modes and the classifier forms behind a page offset, and pages whose fill / per-node classifier launches are capped and stride.

Every case asserts (a) per page the float32 bit patterns of asep_gnn_forward on the page alone (probabilities and hidden state), in every page order
it names, and (b) per page PROB_TOL = 1e-5 against the float64 oracle (the bound of tests/test_gnn_gpu.py): the batched and
the single-page kernels share their bodies, so (a) alone says nothing about the bodies.  Each case also asserts the inequality that shows it reached
its path (chunk count, fed entries beyond the fill grid, N x h1 beyond the per-node grid, the step mode by name)."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-5
CHUNK_TARGETS = 100000                    # message_fn_chunk.py:77-78: 100000 // N target nodes per interaction chunk
FILL_GRID_CAP, PRE_GRID_CAP = 2048, 1024  # blocks of 256 threads: edge_table_kernel / gnn_pair_pre_kernel stride over what lies beyond
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "citlab-article-separation-new_amd", "csrc")


def _setup(seed=99, **cfg_kw):
    from citlab_article_separation_new_amd.config import GnnConfig
    from citlab_article_separation_new_amd.weights import init_gnn_weights
    from citlab_article_separation_new_amd.gnn_io import GnnGraph
    cfg = GnnConfig(**cfg_kw)
    w = init_gnn_weights(cfg, seed, bias_jitter=0.05)
    return cfg, w, GnnGraph(w, cfg)


def _page(rng, N, E, cfg, R=None):
    edges = rng.integers(0, N, size=(E, 2)).astype(np.int32)       # duplicates, reversed duplicates and self loops among them
    if E > 4:
        edges[1] = edges[0]
        edges[2] = edges[0][::-1]
        edges[3] = [min(3, N - 1), min(3, N - 1)]
    return dict(N=N, edges=edges, u=rng.random((N, cfg.node_feature_dim), dtype=np.float32),
                ef=rng.random((E, cfg.edge_feature_dim), dtype=np.float32) if cfg.edge_feature_dim else None,
                rel=None if R is None else rng.integers(0, N, size=(R, 2)).astype(np.int32))


def _ef(p):
    return p["ef"] if len(p["edges"]) else None


def _single(graph, p):
    """asep_gnn_forward on the page alone -> (class-1 probabilities, hidden state); a page without relations still has a hidden state"""
    from citlab_article_separation_new_amd import gnn_io
    empty = p["rel"] is not None and len(p["rel"]) == 0
    probs = gnn_io.gnn_forward(graph, p["N"], p["edges"], p["u"], _ef(p), None if empty else p["rel"])
    return (np.zeros(0, np.float32) if empty else probs[:, 1].copy()), gnn_io.gnn_hidden(graph, p["N"])


def _oracle(p, w, cfg):
    from oracle import gnn_oracle
    probs, h = gnn_oracle.forward(p["N"], p["edges"], p["u"], p["ef"], p["rel"], w, cfg, dtype=np.float64, return_hidden=True)
    return probs[:, 1], h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max()) if len(a) else 0.0


def _check_call(graph, pages, order, single, oracle, what):
    """one batched call of pages[order]: (a) bits of the single-page call, (b) the float64 oracle"""
    from citlab_article_separation_new_amd import gnn_io
    got = gnn_io.gnn_forward_batch(graph, [pages[k] for k in order])
    assert gnn_io.gnn_batch_launches(graph) > 0
    for slot, k in enumerate(order):
        N = pages[k]["N"]
        h = gnn_io.gnn_page_hidden(graph, slot, N)
        assert got[slot].shape == single[k][0].shape, (what, order, k)
        assert np.array_equal(_bits(got[slot]), _bits(single[k][0])), (what, order, k)
        assert np.array_equal(_bits(h), _bits(single[k][1])), (what, order, k)
        err, err_h = _maxabs(got[slot], oracle[k][0]), _maxabs(h, oracle[k][1])
        print(f"{what} order {order} page {k}: N={N} max|p - oracle| = {err:.3e}, max|h - oracle| = {err_h:.3e}")
        assert err <= PROB_TOL and err_h <= PROB_TOL, (what, order, k)


def _run_case(graph, w, cfg, pages, orders, what):
    single = [_single(graph, p) for p in pages]
    oracle = [_oracle(p, w, cfg) for p in pages]                   # computed once, shared by the orders
    for order in orders:
        _check_call(graph, pages, order, single, oracle, what)


# ---- 1. several interaction chunks per page, the page not first in the call -------------------------------------------------------------------

CHUNK_N, CHUNK_E = (40, 317, 5, 400), (100, 900, 8, 2500)


@pytest.mark.parametrize("kw", [
    dict(use_attention=True, num_attention_heads=2),
    dict(use_attention=True, num_attention_heads=2, multihead_attention_merge_type="average", attention_hidden=[12], undirected_graph=False),
    dict(use_attention=True, num_attention_heads=2, aggregation_type="max"),
], ids=["attention2", "attention2_average_directed", "attention2_max"])
def test_pages_of_several_interaction_chunks_behind_other_pages(kw):
    """edge_chunk_rank_pages_kernel with c > 0 on a page whose node_off and rowptr[node_off] are not 0: N = 317 has chunks of 315 + 2 target nodes,
    N = 400 of 250 + 150; edges cross the chunk boundary in both directions and wrap from the last node to the first"""
    cfg, w, graph = _setup(seed=5, **kw)
    rng = np.random.default_rng(317)
    pages = [_page(rng, N, E, cfg) for N, E in zip(CHUNK_N, CHUNK_E)]
    for p in pages:
        N = p["N"]
        cn = max(1, CHUNK_TARGETS // N)
        if N > 316:
            assert -(-N // cn) >= 2                                 # the path: more than one chunk
            p["edges"][4:8] = [[cn - 1, cn], [cn, cn - 1], [0, N - 1], [N - 1, 0]]
        else:
            assert -(-N // cn) == 1
    _run_case(graph, w, cfg, pages, [[0, 1, 2, 3], [3, 0, 2, 1]], str(kw))
    graph.close()


# ---- 2. directed graphs ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(aggregation_type="max")], ids=["default", "max"])
def test_directed_graphs(kw):
    """undirected_graph=False: E fed entries per page (not 2 E), one-way edges stay one-way; the corrected lists per page against the page alone
    and against the oracle's correction"""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup(seed=17, undirected_graph=False, **kw)
    rng = np.random.default_rng(8)
    empty = _page(rng, 6, 0, cfg)
    messy = _page(rng, 9, 0, cfg)
    messy["edges"] = np.array([[0, 1], [1, 0], [0, 1], [4, 4], [2, 7], [2, 7], [7, 2], [8, 8], [3, 5], [0, 1]], np.int32)
    messy["ef"] = rng.random((10, cfg.edge_feature_dim), dtype=np.float32)
    full = _page(rng, 12, 0, cfg)
    full["edges"] = np.array([[i, j] for i in range(12) for j in range(12) if i != j], np.int32)
    full["ef"] = rng.random((132, cfg.edge_feature_dim), dtype=np.float32)
    pages = [empty, messy, full, _page(rng, 70, 350, cfg)]
    _run_case(graph, w, cfg, pages, [[0, 1, 2, 3]], "directed " + str(kw))
    want = [gnn_io.correct_edges(graph, p["N"], p["edges"], _ef(p)) for p in pages]
    assert [len(e) for e, _ in want[:3]] == [0, 5, 132]            # (0, 1), (1, 0), (2, 7), (7, 2), (3, 5): no (5, 3) is added
    gnn_io.gnn_forward_batch(graph, pages)
    for k, p in enumerate(pages):
        E = p["edges"].shape[0]
        edges, first = gnn_io.gnn_page_edges(graph, k, E)
        ref_e, ref_f = gnn_oracle.correct_edges(p["edges"], _ef(p), p["N"], undirected=False)
        assert np.array_equal(edges, want[k][0]) and np.array_equal(edges, ref_e), k
        if len(edges):
            assert (first < E).all()                                # a directed page has no reversed half
            assert np.array_equal(p["ef"][first], want[k][1]) and np.array_equal(p["ef"][first], ref_f), k
    graph.close()


# ---- 3. the step modes over the nodes of a call ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,env,mode", [
    (dict(), {}, "factored"),
    (dict(), {"ASEP_GNN_FACTOR": "0"}, "mfma_registers"),
    (dict(), {"ASEP_GNN_STEP": "0"}, "generic"),
    (dict(node_feature_dim=55, edge_feature_dim=4), {"ASEP_GNN_FACTOR": "0"}, "mfma_lds"),
    (dict(node_feature_dim=9, edge_feature_dim=0), {}, "factored"),                       # no edge features: ef of a page is None
    (dict(hidden_dim=16, interaction_dim=24, interaction_hidden=[40]), {}, "generic"),    # generic by its widths
], ids=["factored", "unfactored_registers", "generic_by_switch", "unfactored_lds", "no_edge_features", "generic_by_widths"])
def test_step_modes_on_a_page_behind_another(kw, env, mode, monkeypatch):
    """the per-node kernels of every step mode over the nodes of a call: page 1 (node_off = 7) has in-degrees from 0 (node 17 isolated) to > 64
    (200 edges into node 5: several tiles per wave), pages 2 and 3 lie on both sides of a 64-node boundary"""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    for k in ("ASEP_GNN_FACTOR", "ASEP_GNN_STEP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                    # read when the model is loaded
    cfg, w, graph = _setup(seed=23, **kw)
    assert gnn_io.step_mode(graph) == mode
    rng = np.random.default_rng(11)
    pages = [_page(rng, N, E, cfg) for N, E in zip((7, 90, 64, 65), (12, 1400, 320, 325))]
    e1 = pages[1]["edges"]
    e1[:200, 1] = 5
    e1[e1 == 17] = 3
    indeg = np.bincount(gnn_oracle.correct_edges(e1, None, 90, cfg.undirected_graph)[0][:, 1], minlength=90)
    assert indeg[17] == 0 and indeg[5] > 64
    if not cfg.edge_feature_dim:
        assert all(p["ef"] is None for p in pages)
    _run_case(graph, w, cfg, pages, [[0, 1, 2, 3]], mode + " " + str(kw))
    graph.close()


# ---- 4. the classifier forms behind a page offset, listed relations and all pairs ----------------------------------------------------------------

def _pairs_per_block(fast):
    """pairs per block of the two classifier kernels, as the engine's sources state them (the unit table of a call is built from this number)"""
    with open(os.path.join(CSRC, "gnn_kernels.h")) as f:
        generic = int(re.search(r"constexpr int PAIRG_P = (\d+);", f.read()).group(1))
    with open(os.path.join(CSRC, "gnn_engine.hip")) as f:
        specialised = int(re.search(r"cls_fast \? (\d+) : PAIRG_P", f.read()).group(1))
    return specialised if fast else generic


@pytest.mark.parametrize("kw,fast", [
    (dict(classifier_hidden=[48, 20], num_classes=3), False),
    (dict(classifier_hidden=[48]), False),
    (dict(classifier_hidden=[64, 32, 16, 8], num_classes=3, node_feature_dim=20), False),
    (dict(output_type="add_final_hidden_and_input"), True),
], ids=["48_20_3classes", "48", "64_32_16_8_3classes", "output_add"])
def test_classifier_forms_with_listed_relations_and_all_pairs(kw, fast):
    """gnn_pair_cls_generic_pages_kernel (any classifier but 64 / 32 / 2) and the specialised kernel behind output type `add`: relation counts of
    0, 1 and on both sides of a multiple of the kernel's pairs per block, then the same pages with all N x N pairs.  The call returns class 1."""
    cfg, w, graph = _setup(seed=17, **kw)
    ppb = _pairs_per_block(fast)
    assert ppb == (256 if fast else 32)
    rng = np.random.default_rng(3)
    sizes = [(9, 1), (70, 300), (5, 0), (33, 257), (20, ppb - 1), (21, ppb + 1)]
    pages = [_page(rng, N, 4 * N, cfg, R=r) for N, r in sizes]
    _run_case(graph, w, cfg, pages, [list(range(len(pages)))], "listed " + str(kw))
    for p in pages:
        p["rel"] = None                                             # all N x N ordered pairs, row major
    _run_case(graph, w, cfg, pages, [list(range(len(pages)))], "all pairs " + str(kw))
    graph.close()


# ---- 6. pages beyond the launch caps, behind a small page ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(use_attention=True, num_attention_heads=2)], ids=["default", "attention2"])
def test_pages_beyond_the_launch_caps(kw):
    """edge_table_body and gnn_pair_pre_body stride over what their capped grids do not cover; in a call the stride is the page's unit count
    (begin[b + 1] - begin[b]).  N = 800 with 300 000 fed edges: 600 000 entries > 2048 x 256; N = 4200: N x 64 > 1024 x 256 (and, with attention,
    183 interaction chunks of 23 nodes).  Both behind a page of five nodes, then in the reverse order."""
    from citlab_article_separation_new_amd import gnn_io
    from oracle import gnn_oracle
    cfg, w, graph = _setup(seed=17, **kw)
    rng = np.random.default_rng(4200)
    pages = [_page(rng, 5, 8, cfg, R=10), _page(rng, 800, 300000, cfg, R=200), _page(rng, 4200, 8000, cfg, R=500)]
    assert (2 if cfg.undirected_graph else 1) * 300000 > FILL_GRID_CAP * 256
    assert 4200 * cfg.classifier_hidden[0] > PRE_GRID_CAP * 256
    assert -(-4200 // (CHUNK_TARGETS // 4200)) == 183 and CHUNK_TARGETS // 4200 == 23
    assert sum(p["N"] ** 2 for p in pages) < 2 ** 30
    _run_case(graph, w, cfg, pages, [[0, 1, 2], [2, 1, 0]], "caps " + str(kw))       # (the last call: the 300 000-edge page is page 1)
    edges, first = gnn_io.gnn_page_edges(graph, 1, 300000)
    ref_e, ref_f = gnn_oracle.correct_edges(pages[1]["edges"], pages[1]["ef"], 800, undirected=True)
    assert np.array_equal(edges, ref_e) and np.array_equal(pages[1]["ef"][first % 300000], ref_f)
    graph.close()
