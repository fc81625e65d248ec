"""Which kernels the ARU engine launches: the fast form under the default, its sibling under the switch, the walkers by page size.

Every fast kernel of the engine has a slower sibling behind an environment switch, and the suite's evidence for the fast
forms is "fast run == slow run".  Such a comparison cannot tell whether the fast kernel ran: when a dispatch condition of csrc/aru_engine.hip
stops matching, both runs execute the sibling, are trivially equal, and only the benchmark gets slower.  These tests read the engine's own
launch record (tests/kernel_profile.py) instead of results -- no oracle here.  The kernel names are the ones the launch sites of
csrc/aru_engine.hip give their records (run_conv, run_convb, run_convr, run_res8, run_res8ws, run_res8b / run_res8w, run_resb_tail, run_deconv,
run_deconvb, att_cnn).

Pages of at most 330 x 540 pixels: all three scales of the pyramid have room for the level-0 walkers there, and the level-3 map of scale 1
(21 x 34) still has two 32-column strips."""
import numpy as np
import pytest

import kernel_profile as kp

pytestmark = pytest.mark.gpu

BIG = (330, 540)
MAXP = 12                           # problems (pages x scales) of one launch (csrc/aru_kernels.h)


def _graph(kw, seed=1234):
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    cfg = AruConfig(**kw)
    return cfg, AruGraph(init_aru_weights(cfg, seed, bias_jitter=0.05, logit_scale=0.05), cfg)


def _image(H, W, seed=7):
    return np.random.default_rng(seed).random((H, W), dtype=np.float32)


def _switch_names():
    from citlab_article_separation_new_amd import _lib
    return set(_lib.load_library().asep_engine_switches().decode().split())


def _profile(kw, size, env, monkeypatch):
    for name in _switch_names():
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                            # read when the engine is created
    cfg, graph = _graph(kw)
    try:
        return cfg, kp.launched(graph, _image(*size))
    finally:
        graph.close()


BF, F32S, F32 = {"compute_dtype": "bf16"}, {"compute_dtype": "f32s"}, {"compute_dtype": "f32"}
ELU = {"activation_name": "elu"}

# One row per (switch, value): the engine's arithmetic / graph variant, the page, the kernels that must have been launched, the kernels that must
# not, and -- where the sibling's name also serves other layers -- (kernel, part of the layer text, wanted) for the layer in question.
# value None = the switch unset.  A name without '<' stands for every instantiation of the kernel.
CONVB64, CONVB64_RES = "convb_kernel<3,3,2,2,2,8,2,false,8>", "convb_kernel<3,3,2,2,2,8,2,true,8>"      # >= 64 output channels, eight waves
CONVB32_RES = "convb_kernel<3,3,2,2,1,8,3,true,4>"                                                       # 32 -> 32 convR_2 (+ residual)
C12_DENSE, C12_PADDED = kp.C12_DENSE, kp.C12_PADDED
TABLE = [
    # the 64 -> 64 and 32 -> 64 layers of the bf16 engine: filter in registers (convr_kernel) | convb_kernel
    ("ASEP_BF_CONVR", None, BF, BIG, ["convr_kernel<false,false,false,32>", "convr_kernel<true,true,false,64>", "convr_kernel<false,true,false,64>",
                                      "convr_kernel<false,true,true,64>", "maxpool2b_kernel"], [],
     [("convb_kernel", "unet_down_3/", False), ("convb_kernel", "unet_up_3/convR", False)]),
    ("ASEP_BF_CONVR", "0", BF, BIG, [CONVB64, CONVB64_RES], ["convr_kernel", "maxpool2b_kernel"],
     [("convb_kernel", "unet_down_3/conv1", True), ("convb_kernel", "unet_down_3/convR_0", True), ("convb_kernel", "unet_down_3/convR_2", True),
      ("convb_kernel", "unet_up_3/convR_1", True)]),
    # bf16 level 0: strip walkers + their border tiles | 16 x 32 tile kernels (1: both blocks walk, 2: the up block only, 0: neither)
    ("ASEP_BF_WALK", None, BF, BIG, ["res8w_kernel<false>", "res8w_kernel<true>", "res8wb_kernel<false>", "res8wb_kernel<true>"], ["res8f_kernel", "res8b_kernel"], []),
    ("ASEP_BF_WALK", "1", BF, BIG, ["res8w_kernel<false>", "res8w_kernel<true>", "res8wb_kernel<false>", "res8wb_kernel<true>"], ["res8f_kernel", "res8b_kernel"], []),
    ("ASEP_BF_WALK", "2", BF, BIG, ["res8w_kernel<true>", "res8wb_kernel<true>", "res8f_kernel<false>"], ["res8w_kernel<false>", "res8wb_kernel<false>", "res8f_kernel<true>"], []),
    ("ASEP_BF_WALK", "0", BF, BIG, ["res8f_kernel<false>", "res8f_kernel<true>"], ["res8w_kernel", "res8wb_kernel"], []),
    # bf16 32-channel residual tails: one persistent kernel | three convb_kernel launches
    ("ASEP_BF_RES32", None, BF, BIG, ["res32_tail_kernel<0>"], [CONVB32_RES], [("convb_kernel", "unet_down_2/convR", False), ("convb_kernel", "unet_up_2/convR", False)]),
    ("ASEP_BF_RES32", "0", BF, BIG, [CONVB32_RES], ["res32_tail_kernel"],
     [("convb_kernel", "unet_down_2/convR_0", True), ("convb_kernel", "unet_down_2/convR_2", True), ("convb_kernel", "unet_up_2/convR_1", True)]),
    # f32s level 0: split-product strip walkers over the pages' interior + res8v over the frame | res8v over everything
    ("ASEP_SPLIT_WALK", None, F32S, BIG, ["res8ws_kernel<false>", "res8ws_kernel<true>", "res8v_down_kernel<0>", "res8v_up_kernel<0>"], [],
     [("res8v_down_kernel", "frame", True), ("res8v_up_kernel", "frame", True)]),
    ("ASEP_SPLIT_WALK", "0", F32S, BIG, ["res8v_down_kernel<0>", "res8v_up_kernel<0>"], ["res8ws_kernel"],
     [("res8v_down_kernel", "frame", False), ("res8v_up_kernel", "frame", False)]),
    # f32s deconvolutions with >= 32 input channels: split products | fp32 MFMA
    ("ASEP_SPLIT_DECONV", None, F32S, BIG, ["deconvs_kernel", "deconv8v_kernel"], ["deconv_mfma_kernel"],
     [("deconvs_kernel", "unet_up_3/deconv", True), ("deconvs_kernel", "unet_up_2/deconv", True), ("deconvs_kernel", "unet_up_1/deconv", True)]),
    ("ASEP_SPLIT_DECONV", "0", F32S, BIG, ["deconv_mfma_kernel<2,false>", "deconv_mfma_kernel<1,false>", "deconv8v_kernel"], ["deconvs_kernel"],
     [("deconv_mfma_kernel", "unet_up_3/deconv", True), ("deconv_mfma_kernel", "unet_up_1/deconv", True)]),
    # fused level-0 blocks and attention head | layer by layer (fp32 engines; the bf16 engine reads the switch for its elu / leaky fused forms)
    ("ASEP_FUSED8", None, F32S, BIG, ["res8v_down_kernel<0>", "res8v_up_kernel<0>", "res8ws_kernel", "att_headv_kernel<false>"], ["conv_c1_kernel"], []),
    ("ASEP_FUSED8", "0", F32S, BIG, ["conv_c1_kernel<3,8>", "conv_c1_kernel<4,12>", "maxpool2_kernel"], ["res8v_down_kernel", "res8v_up_kernel", "res8ws_kernel", "att_headv_kernel"],
     [("conv_mfma_kernel", "unet_down_0/convR_0", True), ("conv_mfma_kernel", "unet_up_0/conv1", True)]),
    ("ASEP_FUSED8", None, F32, BIG, ["res8v_down_kernel<0>", "res8v_up_kernel<0>", "att_headv_kernel<false>"], ["conv_c1_kernel", "res8ws_kernel"], []),
    ("ASEP_FUSED8", "0", F32, BIG, ["conv_c1_kernel<3,8>", "conv_c1_kernel<4,12>"], ["res8v_down_kernel", "res8v_up_kernel", "att_headv_kernel"],
     [("conv_mfma_kernel", "unet_down_0/convR_0", True)]),
    ("ASEP_FUSED8", None, {**BF, **ELU}, BIG, ["res8b_kernel<false,1>", "res8b_kernel<true,1>", "resb_tail_kernel<16,1>", "res32_tail_kernel<1>"], ["conv_c1_kernel", "res8w_kernel", "res8f_kernel"], []),
    ("ASEP_FUSED8", "0", {**BF, **ELU}, BIG, ["conv_c1_kernel<3,8,true>"], ["res8b_kernel", "resb_tail_kernel", "res32_tail_kernel"],
     [("convb_kernel", "unet_down_0/convR_0", True), ("convb_kernel", "unet_down_1/convR_2", True), ("convb_kernel", "unet_up_0/conv1", True)]),
    # fp32 level 0, attention head, 16 -> 8 deconvolution, 32 -> 1 conv: vector ALU | MFMA
    ("ASEP_R8_VALU", None, F32, BIG, ["res8v_down_kernel<0>", "res8v_up_kernel<0>", "att_headv_kernel<false>", "deconv8v_kernel", "conv_c1out_kernel"],
     ["res8_down_kernel", "res8_up_kernel", "att_head_kernel"], [("deconv_mfma_kernel", "unet_up_0/deconv", False)]),
    ("ASEP_R8_VALU", "0", F32, BIG, ["res8_down_kernel<false>", "res8_up_kernel<false>", "att_head_kernel"],
     ["res8v_down_kernel", "res8v_up_kernel", "att_headv_kernel", "deconv8v_kernel", "conv_c1out_kernel"],
     [("deconv_mfma_kernel", "unet_up_0/deconv", True), ("conv_mfma_kernel", "attPart/conv4", True)]),
    ("ASEP_R8_VALU", "0", F32S, BIG, ["res8_down_kernel<false>", "res8_up_kernel<false>", "att_head_kernel"], ["res8v_down_kernel", "res8v_up_kernel", "res8ws_kernel", "att_headv_kernel"], []),
    # attention conv2 (12 -> 16, 4 x 4) of the fp32 engine: dense 12-channel K mapping | padded to 16 channels.  (The f32s engine runs this layer
    # on convs_kernel whatever the switch says.)
    ("ASEP_C12", None, F32, BIG, [C12_DENSE], [C12_PADDED], []),
    ("ASEP_C12", "0", F32, BIG, [C12_PADDED], [C12_DENSE], []),
    # 2 x 2 max pool in the producing kernel's epilogue | maxpool2_kernel behind it
    ("ASEP_FUSE_POOL", None, F32S, BIG, ["convs_kernel"], ["maxpool2_kernel"], []),
    ("ASEP_FUSE_POOL", "0", F32S, BIG, ["convs_kernel", "maxpool2_kernel"], [], []),
    # elu / leaky in the producing kernel's epilogue (and with it the fused level-0 blocks and head of the variants) | act_kernel behind every layer
    ("ASEP_FUSE_ACT", None, {**F32S, **ELU}, BIG, ["res8v_down_kernel<1>", "res8v_up_kernel<1>", "att_headv_kernel<false>"], ["act_kernel", "conv_c1_kernel"], []),
    ("ASEP_FUSE_ACT", "0", {**F32S, **ELU}, BIG, ["act_kernel", "conv_c1_kernel<3,8>", "conv_c1_kernel<4,12>"], ["res8v_down_kernel", "res8v_up_kernel", "att_headv_kernel"], []),
]
# switches of the library's list that select no kernel form of the ARU engine: a tile order, the page lanes of a batch call, the relation net
NOT_A_KERNEL_FORM = {"ASEP_XCD_SCHED", "ASEP_LANES", "ASEP_GNN_STEP", "ASEP_GNN_FACTOR", "ASEP_GNN_BATCH", "ASEP_GNN_LANES"}


def test_the_table_covers_every_kernel_switch_of_the_library():
    """every switch of asep_engine_switches() that selects between two kernel forms of the ARU engine has a row for the default and for each other value"""
    rows = {}
    for sw, value, *_ in TABLE:
        rows.setdefault(sw, set()).add(value)
    assert set(rows) == _switch_names() - NOT_A_KERNEL_FORM
    for sw, values in rows.items():
        assert None in values and "0" in values, sw
    assert rows["ASEP_BF_WALK"] == {None, "0", "1", "2"}


@pytest.mark.parametrize("sw,value,kw,size,present,absent,layers", TABLE,
                         ids=[f"{r[0]}={r[1]}-{r[2]['compute_dtype']}{'-elu' if 'activation_name' in r[2] else ''}" for r in TABLE])
def test_each_switch_selects_the_kernels_it_names(sw, value, kw, size, present, absent, layers, monkeypatch):
    _, prof = _profile(kw, size, {} if value is None else {sw: value}, monkeypatch)
    what = f"{sw}={value} {kw} {size[0]}x{size[1]}"
    kp.check(prof, present, absent, what)
    for kernel, part, wanted in layers:
        n = kp.calls(prof, kernel, part)
        assert (n > 0) == wanted, f"{what}: {kernel} on '{part}': {n} launches; launched: {sorted(prof)}"


def _convr_layers(cfg):
    """the layers of the form convr_kernel serves (csrc/convr_kernels.h): 3 x 3, 64 output channels, ONE input tensor of 64
    channels, or of 32 channels without ReLU and residual -- the conv1 that opens the 64-channel down block.  (The up block's conv1 reads the
    concatenation of two tensors and stays on convb_kernel.)  -> [(part of the layer's scope, input channels)]"""
    out = []
    n = cfg.scale_space_num
    for l in range(n):
        if cfg.feat(l) != 64:
            continue
        if l > 0 and cfg.feat(l - 1) == 32:
            out.append((f"unet_down_{l}/conv1", 32))
        out += [(f"unet_down_{l}/convR_{r}", 64) for r in range(cfg.res_depth)]
        if l < n - 1:
            out += [(f"unet_up_{l}/convR_{r}", 64) for r in range(cfg.res_depth)]
    return out


def test_default_bf16_engine_launches_its_fast_forms_and_every_convr_layer(monkeypatch):
    cfg, prof = _profile(BF, BIG, {}, monkeypatch)
    kp.check(prof, ["convr_kernel", "res8w_kernel<false>", "res8w_kernel<true>", "res8wb_kernel<false>", "res8wb_kernel<true>", "res32_tail_kernel<0>",
                    "res16f_kernel", "att_headb_kernel", "deconvb8_kernel", "deconvb_kernel", "maxpool2b_kernel", "conv_c1out_kernel", "chansumb_kernel",
                    "combine_kernel"],
             ["res8f_kernel", "res8b_kernel", "resb_tail_kernel", "att_headv_kernel", "att_head_kernel", "conv_c1_kernel", "act_kernel", "maxpool2_kernel",
              "conv_mfma_kernel", "convs_kernel"], "bf16 default")
    # one launch per layer (the three scales of the page are three problems of one launch), every layer of the form on convr_kernel: a layer that
    # falls back on convb_kernel lowers the count and is named
    layers = _convr_layers(cfg)
    per_layer = -(-cfg.num_scales_att // MAXP)
    assert len(layers) == 1 + 2 * cfg.res_depth == 7
    for scope, cin in layers:
        n = kp.calls(prof, "convr_kernel", scope)
        assert n == per_layer, f"{scope} ({cin} -> 64): {n} convr_kernel launches, {kp.calls(prof, 'convb_kernel', scope)} of convb_kernel"
    assert kp.calls(prof, "convr_kernel") == per_layer * len(layers)
    width = lambda name: int(kp.instance(name).rstrip(">").split(",")[-1])
    by_width = {c: sum(k for name, k in prof.items() if kp.base(name) == "convr_kernel" and width(name) == c) for c in (32, 64)}
    assert by_width == {c: per_layer * sum(1 for _, ci in layers if ci == c) for c in (32, 64)}
    assert by_width[32] == 1 and by_width[64] == 6
    assert kp.calls(prof, "maxpool2b_kernel") == per_layer              # behind unet_down_3/convR_2, the one layer of the form that pools
    assert kp.calls(prof, "res32_tail_kernel") == 2 * per_layer         # unet_down_2, unet_up_2


def test_default_f32s_engine_launches_its_fast_forms(monkeypatch):
    _, prof = _profile(F32S, BIG, {}, monkeypatch)
    kp.check(prof, ["res8ws_kernel<false>", "res8ws_kernel<true>", "res8v_down_kernel<0>", "res8v_up_kernel<0>", "att_headv_kernel<false>", "convs_kernel",
                    "convs16_kernel", "deconvs_kernel", "deconv8v_kernel", "conv_c1out_kernel", "combine_kernel"],
             ["deconv_mfma_kernel", "maxpool2_kernel", "act_kernel", "conv_c1_kernel", "res8_down_kernel", "res8_up_kernel", "att_head_kernel",
              "conv_wino_kernel", "conv_winor_kernel", "convb_kernel", "convr_kernel"], "f32s default")
    assert kp.calls(prof, "deconvs_kernel") == 3                        # unet_up_3, _2, _1 (unet_up_0: deconv8v_kernel)


def test_default_f32_engine_launches_its_fast_forms(monkeypatch):
    _, prof = _profile(F32, BIG, {}, monkeypatch)
    kp.check(prof, ["res8v_down_kernel<0>", "res8v_up_kernel<0>", "att_headv_kernel<false>", "conv_wino_kernel", "conv_winor_kernel", "conv_mfma_kernel",
                    C12_DENSE, "deconv_mfma_kernel", "deconv8v_kernel", "conv_c1out_kernel", "combine_kernel"],
             ["res8ws_kernel", "convs_kernel", "convs16_kernel", "deconvs_kernel", "res8_down_kernel", "res8_up_kernel", "att_head_kernel", "conv_c1_kernel",
              "act_kernel", "convb_kernel", "convr_kernel"], "f32 default")


def test_fuse_pool_off_runs_one_pool_kernel_per_pooling_layer(monkeypatch):
    """f32s: the pools of the attention CNN's conv2 and conv3 and of the down blocks 1 .. n - 2 (level 0 pools inside its fused block, the head
    inside att_headv_kernel, whatever the switch says)"""
    cfg, prof = _profile(F32S, BIG, {"ASEP_FUSE_POOL": "0"}, monkeypatch)
    assert kp.calls(prof, "maxpool2_kernel") == 2 + (cfg.scale_space_num - 2)


# ---- the walkers by page size ------------------------------------------------------------------
def _scales(H, W, n=3):
    return [(-(-H // (1 << s)), -(-W // (1 << s))) for s in range(n)]


@pytest.mark.parametrize("H,W", [(160, 132), (140, 131), (330, 540), (200, 280)])
@pytest.mark.parametrize("dtype", ["bf16", "f32s"])
def test_level0_walkers_run_on_the_pages_with_room_for_them_and_only_there(dtype, H, W, monkeypatch):
    """160 x 132 is just large enough at scale 0 (csrc/level0_plan.h: four 24-column strips right of column 32, two 16-row bands below row 16), its
    coarser scales are not: walker and tile kernel side by side.  140 x 131: no walker.  330 x 540: every scale walks, and the bf16 tile kernel is
    gone (the f32s walkers leave the frame around their region to res8v, which therefore always runs)."""
    from test_split_walk_gpu import _walks
    walks = [_walks(h, w) for h, w in _scales(H, W)]
    assert walks == {(160, 132): [True, False, False], (140, 131): [False] * 3, (330, 540): [True] * 3, (200, 280): [True, True, False]}[(H, W)]
    _, prof = _profile({"compute_dtype": dtype}, (H, W), {}, monkeypatch)
    what = f"{dtype} {H}x{W}"
    walkers = ["res8w_kernel<false>", "res8w_kernel<true>", "res8wb_kernel<false>", "res8wb_kernel<true>"] if dtype == "bf16" else ["res8ws_kernel<false>", "res8ws_kernel<true>"]
    tiles = ["res8f_kernel<false>", "res8f_kernel<true>"] if dtype == "bf16" else ["res8v_down_kernel<0>", "res8v_up_kernel<0>"]
    kp.check(prof, walkers if any(walks) else [], [] if any(walks) else [kp.base(k) for k in walkers], what)
    if dtype == "bf16":
        kp.check(prof, [] if all(walks) else tiles, ["res8f_kernel"] if all(walks) else [], what)
    else:
        kp.check(prof, tiles, [], what)
        for k in ("res8v_down_kernel", "res8v_up_kernel"):              # (with a walker in the launch, res8v's launch is the frame launch)
            assert (kp.calls(prof, k, "frame") > 0) == any(walks), (what, k)
            assert kp.calls(prof, k) == 1, (what, k)
