"""GPU parity of graph 'RU_v2' (the reference's backbones/RU_v2.py) on the fp32 engines against the float64 restatement tests/ru_v2_oracle.py,
which tests/test_ru_v2_host.py holds to the reference's own logits.

Gate: every published end point (scale_0_unet_{down,up}_<l>_{conv,deconv}, logits) and the probabilities: max|d| <= 2e-5 * max|ref| --
the project's fp32 gate (README, "Parity status").  Pages: the smallest at which the input-pyramid code can go wrong -- 37 x 53 (odd at every
level: partial pool windows at both borders), 16 x 16 (level 4 is 1 x 1), 5 x 70 (fewer rows than levels), 3 x 3 with three levels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GATE = 2e-5
DTYPES = ["f32", "f32s"]


def _setup(dtype, seed=77, **kw):
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    cfg = AruConfig(graph="RU_v2", compute_dtype=dtype, **kw)
    w = init_aru_weights(cfg, seed, bias_jitter=0.05, logit_scale=0.05)
    return cfg, w, AruGraph(w, cfg)


def _page(H, W, seed, channels=1, scale=1.0):
    rng = np.random.default_rng(seed)
    img = rng.random((H, W) if channels == 1 else (H, W, channels), dtype=np.float32)
    img[H // 3:H // 3 + 2] = 0.05                    # a dark rule, like a separator
    return img * np.float32(scale)


def _check(graph, cfg, w, img, what):
    """one forward: every end point and the probabilities against the restatement; the figures are printed before they are asserted"""
    import ru_v2_oracle
    from citlab_article_separation_new_amd import net_post_processing_helper as helper
    ref, inter = ru_v2_oracle.forward(img, w, cfg, dtype=np.float64, return_intermediates=True)
    out = helper.get_net_output(img, graph, "0")
    assert out.shape == ref.shape and out.dtype == np.float32
    names = sorted(inter)
    assert len(names) == cfg.scale_space_num + 2 * (cfg.scale_space_num - 1) + 1
    worst = []
    for name in names + ["probabilities"]:
        got = out if name == "probabilities" else helper.get_endpoint(graph, name)
        want = ref if name == "probabilities" else inter[name]
        assert got.shape == want.shape, name
        rel = float(np.abs(got - want).max()) / float(np.abs(want).max())
        print(f"{what} {name}: max|d| / max|ref| = {rel:.2e}")
        worst.append((rel, name))
    assert max(worst)[0] <= GATE, f"{what}: {max(worst)}"
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,kw", [(37, 53, {}), (16, 16, {}), (5, 70, {}), (3, 3, {"scale_space_num": 3})], ids=str)
def test_pages_against_the_restatement(dtype, H, W, kw):
    cfg, w, graph = _setup(dtype, **kw)
    _check(graph, cfg, w, _page(H, W, 100 * H + W), f"{dtype} {H}x{W}")
    graph.close()


VARIANTS = [((37, 53), {"inp4up": False}), ((16, 16), {"mvn": True}), ((37, 53), {"channels": 3}), ((5, 70), {"res_depth": 1}),
            ((37, 53), {"activation_name": "elu"}), ((16, 16), {"activation_name": "leaky"}), ((37, 53), {"feat_root": 12, "scale_space_num": 3}),
            ((5, 70), {"channels": 3, "mvn": True, "inp4up": False})]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,kw", VARIANTS, ids=str)
def test_variants_against_the_restatement(dtype, hw, kw):
    cfg, w, graph = _setup(dtype, **kw)
    img = _page(hw[0], hw[1], 7, kw.get("channels", 1), 255.0 if kw.get("mvn") else 1.0)   # standardised pages are fed as 0..255
    _check(graph, cfg, w, img, f"{dtype} {kw}")
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_batch_of_pages_of_different_sizes_equals_the_single_page_calls(dtype):
    import torch
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    cfg, w, graph = _setup(dtype)
    lib, h = _lib.init_device(0), graph.handle(0)
    sizes = [(37, 53), (16, 16), (5, 70)]
    pages = [_page(s[0], s[1], i) for i, s in enumerate(sizes)]
    d_in = [torch.from_numpy(p).cuda() for p in pages]
    d_out = [torch.empty(s[0], s[1], 2, device="cuda") for s in sizes]
    Arr, Ints = C.c_void_p * 3, C.c_int32 * 3
    rc = lib.asep_aru_forward_batch_dev2(h, 3, Arr(*[t.data_ptr() for t in d_in]), Ints(*[s[0] for s in sizes]), Ints(*[s[1] for s in sizes]),
                                         Arr(*[t.data_ptr() for t in d_out]), None, None, 0.5, None)
    _lib.check(rc, "asep_aru_forward_batch_dev2")
    torch.cuda.synchronize()
    batch = [t.cpu().numpy() for t in d_out]
    batch_up0 = helper.get_endpoint(graph, "p1/scale_0_unet_up_0_conv")
    for b in range(3):
        single = helper.get_net_output(pages[b], graph, "0")
        assert np.array_equal(batch[b], single), f"page {b} {sizes[b]}: differs from the single-page call"
        if b == 1:
            assert np.array_equal(batch_up0, helper.get_endpoint(graph, "scale_0_unet_up_0_conv"))
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inp4up", [True, False])
def test_profile_names_the_tap_kernel_and_the_fused_level0_down_block(dtype, inp4up):
    """one 256 x 384 gray page: a tap launch per tapped conv1 (4 down levels, + 4 up levels with inp4up), and the level-0 DOWN block, which has no
    concat, still on its fused kernel; the level-0 UP block leaves its fused form exactly when it reads the page"""
    import kernel_profile as kp
    cfg, w, graph = _setup(dtype, inp4up=inp4up)
    prof = kp.launched(graph, _page(256, 384, 3))
    ran = sorted(kp.kernel_set(prof))
    assert kp.calls(prof, "pyr_tap_kernel<1>") == (8 if inp4up else 4), ran
    assert kp.calls(prof, "pyr_tap_kernel") == kp.calls(prof, "pyr_tap_kernel<1>")
    assert kp.calls(prof, "avgpool2_c1_kernel") == 4, ran
    assert kp.calls(prof, "res8v_down_kernel<0>") + kp.calls(prof, "res8ws_kernel<false>") > 0, ran
    fused_up = kp.calls(prof, "res8v_up_kernel<0>") + kp.calls(prof, "res8ws_kernel<true>")
    assert (fused_up == 0) == inp4up, ran
    for l in range(1, 5):
        assert kp.calls(prof, "pyr_tap_kernel", f"unet_down_{l}/conv1 tap") == 1, ran
        assert kp.calls(prof, "pyr_tap_kernel", f"unet_up_{l - 1}/conv1 tap") == (1 if inp4up else 0), ran
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_ru_is_untouched_by_an_ru_v2_model_in_the_process(dtype):
    from citlab_article_separation_new_amd import net_post_processing_helper as helper
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    cfg_ru = AruConfig(graph="RU", compute_dtype=dtype)
    w_ru = init_aru_weights(cfg_ru, 5, bias_jitter=0.05, logit_scale=0.05)
    img = _page(37, 53, 9)
    g0 = helper.AruGraph(w_ru, cfg_ru)
    before = helper.get_net_output(img, g0, "0").copy()
    g0.close()
    cfg, w, g2 = _setup(dtype)
    helper.get_net_output(img, g2, "0")
    g1 = helper.AruGraph(w_ru, cfg_ru)
    after = helper.get_net_output(img, g1, "0")
    assert np.array_equal(before, after)
    g1.close()
    g2.close()


def test_frozen_graph_through_load_graph_and_the_separator_command_line(tmp_path):
    pytest.importorskip("google.protobuf")
    import tf_ru_v2_graph
    from PIL import Image
    from citlab_article_separation_new_amd import net_post_processing_helper as helper, run_net_post_processing as cli, synth
    from test_net_post_cli_gpu import _page_xml
    cfg, w, g = _setup("f32s")
    g.close()
    pb = tmp_path / "separator_ru_v2.pb"
    pb.write_bytes(tf_ru_v2_graph.build_ru_v2_pb(w, cfg))
    graph = helper.load_graph(str(pb))
    assert graph.cfg.graph == "RU_v2" and graph.cfg.inp4up and graph.cfg.compute_dtype == "f32s"
    out = _check(graph, graph.cfg, graph.tensors, _page(37, 53, 4), "load_graph")
    graph.close()
    data = tmp_path / "data"
    (data / "page").mkdir(parents=True)
    names = []
    for i in range(2):                               # two 96 x 64 scans
        Image.fromarray(synth.synth_page(3 + i, W=64, H=96)).save(data / f"p{i}.png")
        _page_xml(data / "page" / f"p{i}.xml", 64, 96, [(6, 10, 50, 20), (6, 40, 50, 52)])
        names.append(str(data / f"p{i}.png"))
    lst = tmp_path / "images.lst"
    lst.write_text("\n".join(names) + "\n")
    thr = round(float(np.median(out[:, :, 0])), 3)
    assert cli.main(["--path_to_image_list", str(lst), "--path_to_pb", str(pb), "--mode", "separator", "--threshold", str(thr),
                     "--num_processes", "1"]) == 0
    for i in range(2):
        assert (data / "page" / f"p{i}.xml.xml").exists()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_width_that_is_no_multiple_of_4_is_refused_at_load(dtype):
    """feat_root 6: f_0 = 6 -- served or refused with a message, never a wrong result: the engine refuses"""
    from citlab_article_separation_new_amd import _lib
    cfg, w, graph = _setup(dtype, feat_root=6, scale_space_num=3)
    with pytest.raises(_lib.AsepError, match="multiples of 4|Cin"):
        graph.handle(0)


def test_bf16_is_refused_by_the_library_too():
    from citlab_article_separation_new_amd import _lib
    from citlab_article_separation_new_amd.weights import pack_blob
    cfg, w, graph = _setup("f32s")
    lib = _lib.init_device(0)
    blob = pack_blob(w)
    c = _lib.AruCfg(1, 2, 8, 5, 3, 1, 0, 0, 1, 1, 0, 0, 1, 1)            # compute_dtype 1 with input_pyramid
    assert not lib.asep_aru_load(blob, len(blob), C.byref(c)) and "bf16" in _lib.last_error()
    c = _lib.AruCfg(1, 2, 8, 5, 3, 3, 1, 0, 1, 2, 0, 0, 1, 1)            # use_attention with input_pyramid
    assert not lib.asep_aru_load(blob, len(blob), C.byref(c)) and "attention" in _lib.last_error()
