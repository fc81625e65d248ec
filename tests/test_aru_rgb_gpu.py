"""Colour pages ([H,W,3] float32, R, G, B interleaved) through the RU / U nets on the device, against oracle/aru_oracle.py on the same inputs.

What is new on the device is the first layer (conv_c3_kernel, csrc/aru_kernels.h) and the schedule of level 0 around it: with three channels the
fused level-0 DOWN forms (which contain the 1-channel conv1) are skipped and the block runs as conv_c3_kernel + the block tail (or conv2 for 'U').
Sizes are the kernel's edges (64 x 4 pixel blocks with a 66 x 6 window in LDS): 5 x 19 (less than a block in both axes ... H < 8, W < 32),
37 x 53, 130 x 67 (remainders in both axes, more than one block in both), 64 x 256 (exact blocks).

Gates (the project's own, tests/test_aru_gpu.py):
  f32 / f32s  every end point within 2e-5 max|ref| of the fp32 oracle, probabilities within 1e-4;
  bf16        probabilities within 2e-2 of the fp32 graph (the bound test_graph_variants_on_the_bf16_path asserts against the fp32 graph; the
              end points' distances to it are printed), and every end point block by block against forward_torch(storage="bf16",
              teacher=the engine's end points): rms <= 2e-4 of max|ref|, max <= 1.2e-2 of max|ref| (test_aru_gpu.py's block gate).
Every test here fails on an engine without the feature at asep_aru_load ("only 1-channel input is supported")."""
import ctypes as C

import numpy as np
import pytest

import kernel_profile as kp

pytestmark = pytest.mark.gpu

SIZES = [(5, 19), (37, 53), (130, 67), (64, 256)]
MAXP = 12                                   # problems of one launch (csrc/aru_kernels.h)
F32_ENDPOINT_GATE = 2e-5                    # max|d| / max|ref| per end point
PROB_TOL = 1e-4
BF16_PROB_GATE = 2e-2
BF16_BLOCK_RMS_GATE = 2e-4                  # rms(d) / max|ref| per end point, block by block
BF16_BLOCK_MAX_GATE = 1.2e-2                # max|d| / max|ref| per end point, block by block (tests/test_aru_gpu.py: a few bfloat16 steps)


def _colour(H, W, seed):
    """random page with distinct per-channel statistics: R in [0, 0.3), G in [0.3, 0.7), B in [0.6, 1.0); a dark rule across"""
    rng = np.random.default_rng(seed)
    img = rng.random((H, W, 3), dtype=np.float32) * np.array([0.3, 0.4, 0.4], np.float32) + np.array([0.0, 0.3, 0.6], np.float32)
    img[H // 3:H // 3 + 2, :, :] *= 0.1
    return np.ascontiguousarray(img)


def _pages():
    """[(name, page)]: the four sizes, one page constant per channel (a channel swap changes it: every colour page here would show one, this one
    has nothing else to show), one page constant over all channels (standardisation: std clamped at 1e-4; 0.5 and the three channel values are
    sums of powers of two, so the mean is exact in float32 and in the engine's float64 alike)"""
    out = [(f"{H}x{W}", _colour(H, W, 100 * H + W)) for H, W in SIZES]
    out.append(("const_per_channel", np.ascontiguousarray(np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (37, 53, 3)))))
    out.append(("const", np.full((37, 53, 3), 0.5, np.float32)))
    return out


def _kw(graph, depth, act, mvn, dtype, **more):
    return dict(graph=graph, channels=3, scale_space_num=depth, activation_name=act, mvn=mvn, compute_dtype=dtype, **more)


_setup_cache, _ref_cache = {}, {}


def _setup(kw, seed=77):
    """weights of a configuration (the same for its three arithmetics) + a fresh engine graph"""
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    cfg = AruConfig(**kw)
    key = tuple(sorted((k, v) for k, v in kw.items() if k != "compute_dtype"))
    if key not in _setup_cache:
        _setup_cache[key] = init_aru_weights(cfg, seed, bias_jitter=0.05, logit_scale=0.05)
    return cfg, _setup_cache[key], AruGraph(_setup_cache[key], cfg), key


def _reference(key, cfg, w, name, page):
    """fp32 oracle of a page: computed once per configuration, shared by the arithmetics, never written to"""
    from oracle import aru_oracle
    if (key, name) not in _ref_cache:
        ref, inter = aru_oracle.forward_torch(page, w, cfg, return_intermediates=True)
        for a in [ref, *inter.values()]:
            a.setflags(write=False)
        _ref_cache[(key, name)] = (ref, {n: v for n, v in inter.items() if n.startswith("scale_")})
    return _ref_cache[(key, name)]


def _batch2(graph, pages):
    """one asep_aru_forward_batch_dev2 call over `pages` (device-resident) -> their probability maps"""
    import torch
    from citlab_article_separation_new_amd import _lib
    lib = _lib.init_device(0)
    B = len(pages)
    ncls = graph.cfg.n_classes
    d_in = [torch.from_numpy(p).cuda() for p in pages]
    d_out = [torch.empty(p.shape[0], p.shape[1], ncls, device="cuda") for p in pages]
    Arr, Ints = C.c_void_p * B, C.c_int32 * B
    rc = lib.asep_aru_forward_batch_dev2(graph.handle(0), B, Arr(*[t.data_ptr() for t in d_in]), Ints(*[p.shape[0] for p in pages]),
                                         Ints(*[p.shape[1] for p in pages]), Arr(*[t.data_ptr() for t in d_out]), None, None, 0.5, None)
    _lib.check(rc, "asep_aru_forward_batch_dev2")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in d_out]


def _check_pages(kw, pages):
    """every page through the host entry point: end points and probabilities against the oracle by the gates of the arithmetic; then all pages in
    one batch call, bit for bit the single-page results"""
    from citlab_article_separation_new_amd import net_post_processing_helper as helper
    from oracle import aru_oracle
    cfg, w, graph, key = _setup(kw)
    bf16 = cfg.compute_dtype == "bf16"
    singles, neg = [], 0
    try:
        for name, page in pages:
            ref, inter = _reference(key, cfg, w, name, page)
            out = helper.get_net_output(page, graph, "0")
            singles.append(out)
            assert out.shape == ref.shape and out.dtype == np.float32 and np.isfinite(out).all(), name
            eng = {n: helper.get_endpoint(graph, n) for n in inter}
            assert len(eng) == 2 * cfg.scale_space_num - 1 + (cfg.scale_space_num - 1)       # down blocks, up blocks, deconvolutions
            want_of = aru_oracle.forward_torch(page, w, cfg, return_intermediates=True, storage="bf16", teacher=eng)[1] if bf16 else inter
            rows = []
            for n in sorted(inter):
                want = want_of[n]
                assert eng[n].shape == want.shape, (name, n)
                scale = float(np.abs(want).max())
                d = (eng[n] - want).astype(np.float64)
                d32 = float(np.abs(eng[n] - inter[n]).max()) / max(float(np.abs(inter[n]).max()), 1e-30)
                rows.append((n, float(np.abs(d).max()) / max(scale, 1e-30), float(np.sqrt(np.mean(d ** 2))) / max(scale, 1e-30), d32))
                neg += int((inter[n] < 0).sum())
            perr = float(np.abs(out - ref).max())
            bm, br, b32 = max(rows, key=lambda t: t[1]), max(rows, key=lambda t: t[2]), max(rows, key=lambda t: t[3])
            print(f"\n{cfg.compute_dtype} {cfg.graph} n={cfg.scale_space_num} {cfg.activation_name} mvn={int(cfg.mvn)} {name}: worst end point max {bm[0]} "
                  f"{bm[1]:.2e}, rms {br[0]} {br[2]:.2e} ({'block by block, bf16 oracle' if bf16 else 'fp32 oracle'}); against the fp32 graph {b32[0]} "
                  f"{b32[3]:.2e}; max|dp| {perr:.2e}")
            if bf16:
                assert br[2] <= BF16_BLOCK_RMS_GATE, (name, br)
                assert bm[1] <= BF16_BLOCK_MAX_GATE, (name, bm)
                assert perr <= BF16_PROB_GATE, (name, perr)
            else:
                assert bm[1] <= F32_ENDPOINT_GATE, (name, bm)
                assert perr <= PROB_TOL, (name, perr)
        if cfg.activation_name != "relu":
            assert neg > 0                                   # the negative branch of the activation was exercised
        # a channel swap cannot cancel: the page that is constant per channel gives another result with R and B exchanged
        const_c = dict(pages).get("const_per_channel")
        if const_c is not None:
            swapped = helper.get_net_output(np.ascontiguousarray(const_c[:, :, ::-1]), graph, "0")
            assert float(np.abs(swapped - singles[[n for n, _ in pages].index("const_per_channel")]).max()) > 1e-3
        batch = _batch2(graph, [p for _, p in pages])
        for (name, _), got, single in zip(pages, batch, singles):
            assert got.shape == single.shape and np.array_equal(got, single), f"{name}: the batch call differs from the single-page call"
    finally:
        graph.close()


@pytest.mark.parametrize("dtype", ["f32", "f32s", "bf16"])
@pytest.mark.parametrize("mvn", [False, True], ids=["plain", "mvn"])
@pytest.mark.parametrize("act", ["relu", "elu"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("graph", ["RU", "U"])
def test_colour_pages_match_the_oracle_and_the_batch_call_the_single_calls(graph, depth, act, mvn, dtype):
    _check_pages(_kw(graph, depth, act, mvn, dtype), _pages())


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_sixteen_output_channels_of_the_first_layer(dtype):
    """feat_root 16: conv_c3_kernel<16,false> (the bf16 engine is a feat_root 8 engine)"""
    _check_pages(_kw("RU", 2, "relu", True, dtype, feat_root=16), _pages()[:4])


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_more_pages_than_one_launch_holds_on_one_and_two_lanes(dtype, lanes, monkeypatch):
    """13 pages of mixed sizes in one call: more than MAXP problems, so every layer's launch is cut in two (one lane), or the pages go over
    both page lanes; each page equals its single-page call bit for bit"""
    from citlab_article_separation_new_amd import net_post_processing_helper as helper
    monkeypatch.setenv("ASEP_LANES", lanes)
    cfg, w, graph, _ = _setup(_kw("RU", 2, "relu", True, dtype))
    try:
        pages = [_colour(*SIZES[i % 4], seed=900 + i) for i in range(MAXP + 1)]
        batch = _batch2(graph, pages)
        for i, (page, got) in enumerate(zip(pages, batch)):
            assert np.array_equal(got, helper.get_net_output(page, graph, "0")), f"page {i} {page.shape}"
    finally:
        graph.close()


def test_wrong_channel_counts_are_refused():
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    cfg, w, graph, _ = _setup(_kw("RU", 2, "relu", False, "f32s"))
    try:
        with pytest.raises(ValueError, match="3 input channel"):
            helper.get_net_output(np.zeros((8, 8), np.float32), graph, "0")
        with pytest.raises(ValueError, match="expected 3 channel"):
            helper.get_net_output(np.zeros((8, 8, 1), np.float32), graph, "0")
    finally:
        graph.close()
    # the library's own refusals (the Python rule aside): attention + colour, and any other channel count
    lib = _lib.init_device(0)
    blob = graph.blob()
    for channels, att, text in ((3, 1, "without attention (RU or U)"), (2, 0, "2 input channels")):
        c = _lib.AruCfg(channels, 2, 8, 2, 3, 3, att, 0, 1, 0, 0, 0)
        assert not lib.asep_aru_load(blob, len(blob), C.byref(c))
        assert text in _lib.last_error(), _lib.last_error()


# ---- which kernels ran (tests/kernel_profile.py) -----------------------------------------------------------------------------------------
LEVEL0_DOWN_FUSED = ["res8v_down_kernel", "res8_down_kernel", "res8ws_kernel<false>", "res8w_kernel<false>", "res8wb_kernel<false>", "res8f_kernel<false>",
                     "res8b_kernel<false,0>", "res8b_kernel<false,1>", "res8b_kernel<false,2>", "conv_c1_kernel"]


@pytest.mark.parametrize("dtype,act,new,up", [
    ("f32s", "relu", "conv_c3_kernel<8,false>", ["res8v_up_kernel<0>", "res8ws_kernel<true>"]),
    ("f32", "relu", "conv_c3_kernel<8,false>", ["res8v_up_kernel<0>"]),
    ("f32", "elu", "conv_c3_kernel<8,false>", ["res8v_up_kernel<1>"]),
    ("bf16", "relu", "conv_c3_kernel<8,true>", ["res8w_kernel<true>", "res8wb_kernel<true>"]),
    ("bf16", "elu", "conv_c3_kernel<8,true>", ["res8b_kernel<true,1>"]),
])
def test_the_colour_first_layer_runs_and_no_fused_level0_down_form(dtype, act, new, up, monkeypatch):
    """160 x 132: room for the level-0 strip walkers, which the 1-channel net of the same layout takes (tests/test_kernel_selection_gpu.py).
    Colour: the new kernel, no fused DOWN form or walker, the UP block on its fused form as before.  Gray, same layout: no new kernel, the
    fused DOWN forms."""
    from citlab_article_separation_new_amd import _lib
    for name in _lib.load_library().asep_engine_switches().decode().split():
        monkeypatch.delenv(name, raising=False)
    kw = _kw("RU", 3, act, False, dtype)
    cfg, w, graph, _ = _setup(kw)
    try:
        prof = kp.launched(graph, _colour(160, 132, 4))
    finally:
        graph.close()
    kp.check(prof, [new, *up], LEVEL0_DOWN_FUSED, f"colour {dtype} {act}")
    assert kp.calls(prof, "conv_c3_kernel") == 1
    cfg1, w1, gray, _ = _setup(dict(kw, channels=1))
    try:
        prof1 = kp.launched(gray, _colour(160, 132, 4)[:, :, 0].copy())
    finally:
        gray.close()
    kp.check(prof1, up, ["conv_c3_kernel"], f"gray {dtype} {act}")
    down = {"f32s": "res8ws_kernel<false>", "f32": "res8v_down_kernel", "bf16": "res8w_kernel<false>" if act == "relu" else "res8b_kernel<false,1>"}[dtype]
    kp.check(prof1, [down], [], f"gray {dtype} {act}")
