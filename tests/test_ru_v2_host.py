"""Graph 'RU_v2' (the reference's backbones/RU_v2.py: the RU-Net with an input pyramid) on the host: no GPU.

tests/golden/model_wiring_ru_v2.npz holds the logits that the reference's own RU_v2_CNN.infer computed on the eager float64 stand-in for
TensorFlow (tests/golden/make_ru_v2_golden.py; this test reads only the fixture).  The float64 restatement tests/ru_v2_oracle.py, which
the GPU tests of tests/test_ru_v2_gpu.py are measured against, has to reproduce them within the gate tests/test_oracle_wiring.py derives:
max |d| <= 1e-6 * max(1, max |golden|).  Also here: the variable inventory, the frozen-graph importer, the linear split of conv1 that
the engine's tap kernel rests on, and the refusals.
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
import ru_v2_oracle  # noqa: E402
from citlab_article_separation_new_amd.config import AruConfig, GnnConfig  # noqa: E402
from citlab_article_separation_new_amd.weights import aru_tensor_shapes, init_aru_weights  # noqa: E402
from oracle.aru_oracle import conv2d_same  # noqa: E402

Z = np.load(os.path.join(HERE, "golden", "model_wiring_ru_v2.npz"))
META = json.loads(bytes(Z["meta"]).decode("utf-8"))
CASES = {c["name"]: c for c in META["cases"]}


def _cfg(case):
    return AruConfig(graph="RU_v2", apply_softmax=False, **case["cfg"])


def _weights(case):
    return {name: mc.variable_value(name, shape) for name, shape in case["variables"]}


def test_the_fixture_holds_the_cases_the_issue_names():
    cfgs = [c["cfg"] for c in META["cases"]]
    assert CASES["ru_v2_defaults"]["cfg"] == {} and CASES["ru_v2_defaults"]["hw"] == [37, 53]
    assert any(c.get("inp4up") is False for c in cfgs) and any(c.get("mvn") for c in cfgs) and any(c.get("channels") == 3 for c in cfgs)
    assert any(c.get("res_depth") == 1 and c.get("scale_space_num") == 3 for c in cfgs)
    assert any(c.get("activation_name") == "elu" for c in cfgs)
    for case in META["cases"]:
        assert np.array_equal(Z[case["name"] + "::image"], mc.aru_image(case))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_the_reference_logits(name):
    case = CASES[name]
    golden = Z[name + "::logits"]
    got = ru_v2_oracle.forward(Z[name + "::image"], _weights(case), _cfg(case), dtype=np.float64)
    assert got.shape == golden.shape
    d = float(np.abs(got - golden).max())
    print(f"{name}: max|d| {d:.3e}, gate {mc.gate(golden):.3e}")
    assert d <= mc.gate(golden)


@pytest.mark.parametrize("name", list(CASES))
def test_weight_inventory_names_the_reference_variables(name):
    case = CASES[name]
    cfg = _cfg(case)
    want = [(n, tuple(s)) for n, s in case["variables"]]
    assert list(aru_tensor_shapes(cfg).items()) == want
    w = init_aru_weights(cfg, 5)
    assert [(k, v.shape) for k, v in w.items()] == want and all(v.dtype == np.float32 for v in w.values())


@pytest.mark.parametrize("name", list(CASES))
def test_conv1_is_its_main_part_plus_the_tap(name):
    """the engine runs conv1(concat[a, I_l]) as conv1_main(a) + tap(I_l), tap = the conv of the pooled page with the LAST `channels` input
    rows of conv1/weights, no bias: exact in real arithmetic, 1e-12 of max|conv| in float64"""
    case = CASES[name]
    cfg, w = _cfg(case), {k: v.astype(np.float64) for k, v in _weights(case).items()}
    log = ru_v2_oracle.conv1_inputs(Z[name + "::image"], w, cfg)
    assert len(log) == (cfg.scale_space_num - 1) * (2 if cfg.inp4up else 1)
    for scope, main, page in log:
        W, b = w[scope + "/weights"], w[scope + "/biases"]
        cm = main.shape[2]
        assert W.shape[2] == cm + cfg.channels and page.shape[2] == cfg.channels
        whole = conv2d_same(np.concatenate([main, page], axis=2), W, b)
        parts = conv2d_same(main, W[:, :, :cm, :], b) + conv2d_same(page, W[:, :, cm:, :])
        assert float(np.abs(whole - parts).max()) <= 1e-12 * float(np.abs(whole).max()), scope


# ---- frozen-graph importer ---------------------------------------------------------------------------------------------------------
pb_cases = pytest.mark.parametrize("kw", [{}, {"inp4up": False}, {"channels": 3}, {"channels": 3, "inp4up": False, "scale_space_num": 3},
                                          {"res_depth": 1, "scale_space_num": 3, "activation_name": "elu"}, {"activation_name": "leaky"}], ids=str)


def _pb_nodes(cfg, w, **kw):
    pytest.importorskip("google.protobuf")
    import tf_ru_v2_graph
    from citlab_article_separation_new_amd import pb_import
    return pb_import, pb_import.parse_graphdef(tf_ru_v2_graph.build_ru_v2_pb(w, cfg, **kw))


@pb_cases
@pytest.mark.parametrize("style", ["tf_names", "renamed"])
def test_importer_gives_config_and_weights_back(kw, style):
    cfg = AruConfig(graph="RU_v2", **kw)
    w = init_aru_weights(cfg, 11, bias_jitter=0.05)
    opts = {} if style == "tf_names" else {"rename": lambda s: "net/" + s.replace("unet_", "u").replace("conv", "c"), "output_softmax": False}
    pb_import, nodes = _pb_nodes(cfg, w, **opts)
    tensors, got = pb_import.aru_from_nodes(nodes)
    assert list(tensors) == list(w)
    for k in w:
        assert np.array_equal(tensors[k], w[k]), k
    for f in ("graph", "inp4up", "channels", "n_classes", "feat_root", "scale_space_num", "res_depth", "filter_size", "mvn", "activation_name"):
        assert getattr(got, f) == getattr(cfg, f), f
    assert got.apply_softmax == (style == "tf_names") and not got.use_attention and got.use_residual


def test_constants_only_container_of_an_ru_v2_net():
    from citlab_article_separation_new_amd import pb_import
    for kw in ({}, {"inp4up": False, "channels": 3}):
        cfg = AruConfig(graph="RU_v2", **kw)
        w = init_aru_weights(cfg, 3)
        nodes = [{"name": k, "op": "Const", "input": [], "attr": {}, "value": v} for k, v in w.items()]
        tensors, got = pb_import.aru_from_constants(nodes, apply_softmax=True)
        assert got.graph == "RU_v2" and got.inp4up == cfg.inp4up and got.channels == cfg.channels and list(tensors) == list(w)


def test_image_operand_that_is_not_last_is_refused():
    cfg = AruConfig(graph="RU_v2", scale_space_num=3)
    pb_import, nodes = _pb_nodes(cfg, init_aru_weights(cfg, 11), image_last=False)
    with pytest.raises(IOError, match="LAST"):
        pb_import.aru_from_nodes(nodes)


def test_pyramid_that_is_not_the_2x2_average_pool_is_refused():
    cfg = AruConfig(graph="RU_v2", scale_space_num=3)
    pb_import, nodes = _pb_nodes(cfg, init_aru_weights(cfg, 11), pyramid_ksize=3)
    with pytest.raises(IOError, match="2x2 / stride 2 / SAME"):
        pb_import.aru_from_nodes(nodes)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_config_of_the_graph_and_its_refusals():
    cfg = AruConfig(graph="RU_v2")
    assert cfg.inp4up and not cfg.use_attention and cfg.use_residual and cfg.input_pyramid and cfg.root_scope == "ru_net"
    assert not AruConfig(graph="RU").input_pyramid and AruConfig(graph="ARU").root_scope == "aru_net"
    cfg.check_channels()
    AruConfig(graph="RU_v2", channels=3).check_channels()
    with pytest.raises(ValueError):
        AruConfig(graph="RU_v2", channels=2).check_channels()
    cfg.check_graph()
    AruConfig(graph="RU", compute_dtype="bf16").check_graph()
    with pytest.raises(ValueError, match="bf16"):
        AruConfig(graph="RU_v2", compute_dtype="bf16").check_graph()
    with pytest.raises(ValueError, match="end points"):
        GnnConfig(backbone={"graph": "RU_v2"}).backbone_cfg()
    GnnConfig(backbone={"graph": "RU"}).backbone_cfg()
