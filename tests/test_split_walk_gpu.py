"""GPU parity of the f32s level-0 blocks as split-product strip walkers (csrc/res8ws_kernels.h) against the vector-ALU form that
ASEP_SPLIT_WALK=0 selects (res8v_*_kernel) and against the CPU oracle at the fp32 gates.  The walkers cover columns [32, 32 + 24 n) x rows
[16, y_end) of a page with room for four strips; res8v computes the frame around them and the pages too small for a strip.  A page runs at
three scales in one launch (pages of different sizes: some on the walker, some not)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-4
ENDPOINT_GATE = 2e-5            # the fp32 gate of tests/test_split_gpu.py
FORM_GATE = 1e-5                # walker against res8v, end points (max |d| / max(1, max |ref|))
LEVEL0 = ("scale_0_unet_down_0_conv", "scale_0_unet_up_0_conv", "scale_1_unet_down_0_conv", "scale_1_unet_up_0_conv")


def _setup(seed=1234, logit_scale=0.05):
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    cfg = AruConfig(compute_dtype="f32s")
    w = init_aru_weights(cfg, seed, bias_jitter=0.05, logit_scale=logit_scale)
    return cfg, w, AruGraph(w, cfg)


def _image(H, W, seed, wide=False):
    rng = np.random.default_rng(seed)
    img = rng.random((H, W), dtype=np.float32)
    img[H // 3:H // 3 + 2, :] = 0.05
    if wide:                                   # values over six decades: the three-part split carries every bit
        img *= np.float32(10.0) ** rng.integers(-3, 3, size=(H, W)).astype(np.float32)
    return img


def _run_both(img, monkeypatch, names):
    import kernel_profile as kp
    from citlab_article_separation_new_amd import net_post_processing_helper as helper
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ASEP_SPLIT_WALK", flag)        # read when the engine is created
        cfg, w, g = _setup()
        out = helper.get_net_output(img, g, "0")
        res[flag] = (out, {n: helper.get_endpoint(g, n) for n in names}, kp.launched(g, img))      # (the launch record: a pass of its own)
        g.close()
    return cfg, w, res


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def _walks(H, W):
    """the engine's rule (csrc/level0_plan.h, walk_region(H, W).fits; checked on the host by test_level0_plan_host.py): room for four 24-column strips right of column 32 and two 16-row bands below row 16"""
    return (W - 4 - 32) // 24 >= 4 and H - 4 - 16 >= 32


# strip / band remainders and odd sizes; 160 x 132 is just big enough for four strips and two bands at scale 0, 140 x 131 too small
@pytest.mark.parametrize("H,W,wide", [(300, 517, False), (333, 250, False), (160, 132, False), (140, 131, False), (257, 301, True)])
def test_walker_matches_vector_alu_form_and_oracle(H, W, wide, monkeypatch):
    from oracle import aru_oracle
    img = _image(H, W, H * 7 + W, wide)
    cfg, w, res = _run_both(img, monkeypatch, LEVEL0)
    ref, inter = aru_oracle.forward_torch(img, w, cfg, return_intermediates=True)
    # the walker ran where it should (another arithmetic than res8v: the results differ) and nowhere else (res8v alone: bit-identical)
    for s, n in ((0, "scale_0_unet_down_0_conv"), (0, "scale_0_unet_up_0_conv"), (1, "scale_1_unet_down_0_conv"), (1, "scale_1_unet_up_0_conv")):
        h, wd = res["0"][1][n].shape[:2]
        if _walks(h, wd):
            assert not np.array_equal(res["1"][1][n], res["0"][1][n]), (n, h, wd)
        else:
            assert np.array_equal(res["1"][1][n], res["0"][1][n]), (n, h, wd)
    assert _walks(H, W) == ((H, W) != (140, 131))
    # ... and the launch records say the same: the walker kernel in the one run of a page with room for it, in no other
    import kernel_profile as kp
    kp.check(res["1"][2], ["res8ws_kernel<false>", "res8ws_kernel<true>"] if _walks(H, W) else [], [] if _walks(H, W) else ["res8ws_kernel"], "ASEP_SPLIT_WALK=1")
    kp.check(res["0"][2], ["res8v_down_kernel", "res8v_up_kernel"], ["res8ws_kernel"], "ASEP_SPLIT_WALK=0")
    for n in LEVEL0:
        a, b = res["1"][1][n], res["0"][1][n]
        assert a.shape == b.shape == inter[n].shape, n
        assert _rel(a, b) <= FORM_GATE, (n, _rel(a, b))
        assert _rel(a, inter[n]) <= ENDPOINT_GATE, (n, _rel(a, inter[n]))
    assert float(np.abs(res["1"][0] - res["0"][0]).max()) <= 1e-5
    assert float(np.abs(res["1"][0] - ref).max()) <= PROB_TOL


def test_pool_output_of_the_down_block(monkeypatch):
    """the walker's 2 x 2 max pool feeds level 1: its input end point and the level-1 block agree with res8v's and the oracle's"""
    from oracle import aru_oracle
    img = _image(290, 410, 5)
    names = ("scale_0_unet_down_0_conv", "scale_0_unet_down_1_conv")
    cfg, w, res = _run_both(img, monkeypatch, names)
    _, inter = aru_oracle.forward_torch(img, w, cfg, return_intermediates=True)
    for n in names:
        assert _rel(res["1"][1][n], res["0"][1][n]) <= FORM_GATE, n
        assert _rel(res["1"][1][n], inter[n]) <= ENDPOINT_GATE, n


def test_walker_really_runs_and_is_deterministic(monkeypatch):
    from citlab_article_separation_new_amd import net_post_processing_helper as helper
    img = _image(300, 517, 11)
    _, _, res = _run_both(img, monkeypatch, LEVEL0[:2])
    assert not np.array_equal(res["1"][1][LEVEL0[0]], res["0"][1][LEVEL0[0]])     # another arithmetic: the walker ran
    monkeypatch.setenv("ASEP_SPLIT_WALK", "1")
    _, _, g = _setup()
    a = helper.get_net_output(img, g, "0")
    b = helper.get_net_output(img, g, "0")
    assert np.array_equal(a, b)
    g.close()


def test_batch_equals_single_pages(monkeypatch):
    """several pages in one call equal the pages run one at a time.  The batch entry point takes one page size per call, so the
    problems of different sizes in one launch are the three scales of every page: at 203 x 389 scale 0 and 1 run on the walker, scale 2
    (51 x 98) on res8v alone, side by side in the same launches.  (The engine runs a level-0 block only inside a whole forward pass: the DOWN
    and UP blocks are checked on their own through their end points, scale_*_unet_down_0_conv and scale_*_unet_up_0_conv, above.)"""
    import torch
    monkeypatch.setenv("ASEP_SPLIT_WALK", "1")
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    from oracle import aru_oracle
    cfg, w, graph = _setup()
    lib = _lib.init_device(0)
    h = graph.handle(0)
    H, W, B = 203, 389, 5                     # 5 pages x 3 scales = 15 problems > MAXP (12): launch splitting
    rng = np.random.default_rng(3)
    pages = [rng.random((H, W), dtype=np.float32) for _ in range(B)]
    d_in = [torch.from_numpy(p).cuda() for p in pages]
    d_out = [torch.empty(H, W, 2, device="cuda") for _ in range(B)]
    d_u8 = [torch.empty(H, W, 2, device="cuda", dtype=torch.uint8) for _ in range(B)]
    Arr = C.c_void_p * B
    rc = lib.asep_aru_forward_batch_dev(h, B, Arr(*[t.data_ptr() for t in d_in]), H, W, Arr(*[t.data_ptr() for t in d_out]),
                                        Arr(*[t.data_ptr() for t in d_u8]), None, 0.05, None)
    _lib.check(rc, "asep_aru_forward_batch_dev")
    torch.cuda.synchronize()
    for b in range(B):
        got = d_out[b].cpu().numpy()
        assert np.array_equal(got, helper.get_net_output(pages[b], graph, "0")), b
        assert float(np.abs(got - aru_oracle.forward_torch(pages[b], w, cfg)).max()) <= PROB_TOL
    graph.close()
