"""Graph 'RU_v2' on the fp32 engines where tests/test_ru_v2_gpu.py does not look: the seams between the 64 x 4-pixel blocks of pyr_tap_kernel
(csrc/pyr_kernels.h) in gray and in colour, single rows and columns through avgpool2_cn_kernel<3>, a page on the fused level-0 kernels, calls
of more pages than one launch holds (MAXP = 12, csrc/launch_plan.h), batches with per-page statistics, and the widest tapped conv1.

Gate, helpers and reference are those of tests/test_ru_v2_gpu.py: every published end point and the probabilities, max|d| <= 2e-5 * max|ref|
against ru_v2_oracle.forward(..., dtype=np.float64); a batch equals the single-page calls bit for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_ru_v2_gpu import DTYPES, _check, _page, _setup  # noqa: E402


def _seam_page(H, W, seed, channels=1, scale=1.0):
    """_page; below six rows its dark rule would cover half the page or all of it (H < 3: a constant page, on which a wrong column or channel
    reads the same value), so those pages are noise alone"""
    if H >= 6:
        return _page(H, W, seed, channels, scale)
    rng = np.random.default_rng(seed)
    return rng.random((H, W) if channels == 1 else (H, W, channels), dtype=np.float32) * np.float32(scale)


# 9 x 130: level 0 is 3 x 3 blocks (64, 64, 2 wide; 4, 4, 1 high), level 1 (5 x 65) ends in a block one pixel wide; 8 x 128: tile-exact at levels
# 0 and 1, levels 1..3 have 4, 2, 1 rows; 4 x 65 / 5 x 64: one past the seam and exactly at it; 1 x 67, 67 x 1, 1 x 1: every pool window partial
SEAM_PAGES = [(9, 130), (8, 128), (4, 65), (5, 64), (1, 67), (67, 1), (1, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inp4up", [True, False], ids=["inp4up", "down_only"])
@pytest.mark.parametrize("channels", [1, 3], ids=["gray", "colour"])
def test_tile_seams_against_the_restatement(dtype, channels, inp4up):
    cfg, w, graph = _setup(dtype, channels=channels, inp4up=inp4up)
    for H, W in SEAM_PAGES:
        _check(graph, cfg, w, _seam_page(H, W, 1000 * H + W, channels), f"{dtype} ch{channels} inp4up={inp4up} {H}x{W}")
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_colour_seams_with_mvn_pad_with_zeros_after_standardising(dtype):
    """a 0..255 page has a mean near 127: a window padded with the raw zero, then standardised, would put -mean/std around the page"""
    cfg, w, graph = _setup(dtype, channels=3, mvn=True)
    _check(graph, cfg, w, _page(9, 130, 31, 3, 255.0), f"{dtype} colour mvn 9x130")
    graph.close()


# ---- the fused level-0 kernels ---------------------------------------------------------------------------------------------------------------
# f32: the level-0 DOWN block of a gray page is res8v_down_kernel<0> at every size below 2^28 pixels (r8v_fits).  f32s: the strip walkers
# res8ws_kernel need walk_region(H, W).fits (csrc/level0_plan.h): (W - 36) / 24 >= 4 strips and H - 20 >= 32 rows, so 52 x 132 is the smallest
# page; 53 x 133 is that plus one odd row and column of frame, and tests/test_split_walk_gpu.py has 140 x 131 one column short.
FUSED_H, FUSED_W = 53, 133


def _fused_forms(dtype):
    return ("res8ws_kernel<false>", "res8ws_kernel<true>") if dtype == "f32s" else ("res8v_down_kernel<0>", "res8v_up_kernel<0>")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inp4up", [True, False], ids=["inp4up", "down_only"])
def test_a_page_on_the_fused_level0_kernels_against_the_restatement(dtype, inp4up):
    import kernel_profile as kp
    cfg, w, graph = _setup(dtype, inp4up=inp4up)
    img = _page(FUSED_H, FUSED_W, 5)
    prof = kp.launched(graph, img)
    down, up = _fused_forms(dtype)
    ran = sorted(kp.kernel_set(prof))
    assert kp.calls(prof, down) == 1, ran
    assert kp.calls(prof, up) == (0 if inp4up else 1), ran
    assert kp.calls(prof, "pyr_tap_kernel", "unet_down_1/conv1 tap") == 1, ran       # the tapped conv1 that reads the fused block's pool
    assert kp.calls(prof, "pyr_tap_kernel", "unet_up_0/conv1 tap") == (1 if inp4up else 0), ran
    _check(graph, cfg, w, img, f"{dtype} fused level 0 inp4up={inp4up} {FUSED_H}x{FUSED_W}")
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_colour_page_of_that_size_takes_conv_c3_and_the_tail(dtype):
    import kernel_profile as kp
    cfg, w, graph = _setup(dtype, channels=3)
    img = _page(FUSED_H, FUSED_W, 6, 3)
    prof = kp.launched(graph, img)
    kp.check(prof, ["conv_c3_kernel", "pyr_tap_kernel<3>", "avgpool2_cn_kernel<3>"],
             ["res8v_down_kernel", "res8ws_kernel<false>", "pyr_tap_kernel<1>", "avgpool2_c1_kernel"], f"{dtype} colour")
    _check(graph, cfg, w, img, f"{dtype} colour {FUSED_H}x{FUSED_W}")
    graph.close()


# ---- batches -----------------------------------------------------------------------------------------------------------------------------------
def _batch(lib, h, pages, profile=False):
    """asep_aru_forward_batch_dev2 over `pages`; returns the pages' probabilities (and, with profile, {recorded name: calls} of the call)"""
    import torch
    from citlab_article_separation_new_amd import _lib
    B = len(pages)
    d_in = [torch.from_numpy(p).cuda() for p in pages]
    d_out = [torch.empty(p.shape[0], p.shape[1], 2, device="cuda") for p in pages]
    Arr, Ints = C.c_void_p * B, C.c_int32 * B
    if profile:
        _lib.check(lib.asep_aru_profile(h, 2), "asep_aru_profile")
    try:
        rc = lib.asep_aru_forward_batch_dev2(h, B, Arr(*[t.data_ptr() for t in d_in]), Ints(*[p.shape[0] for p in pages]),
                                             Ints(*[p.shape[1] for p in pages]), Arr(*[t.data_ptr() for t in d_out]), None, None, 0.5, None)
        _lib.check(rc, "asep_aru_forward_batch_dev2")
        torch.cuda.synchronize()
        prof = {}
        if profile:
            buf = C.create_string_buffer(1 << 20)
            _lib.check(lib.asep_aru_profile_report(h, buf, len(buf)), "asep_aru_profile_report")
            for rec in json.loads(buf.value.decode()):
                prof[rec["kernel"]] = prof.get(rec["kernel"], 0) + int(rec["calls"])
    finally:
        if profile:
            lib.asep_aru_profile(h, 0)
    out = [t.cpu().numpy() for t in d_out]
    return (out, prof) if profile else out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_thirteen_pages_in_one_call_equal_the_single_page_calls(dtype, lanes, monkeypatch):
    """one page more than a launch holds: the tap launch splits and tile_begin starts again at 0 in the second chunk; the same pages in reversed
    order (other chunks, other tile_begin of every page) give the same results"""
    import kernel_profile as kp
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    monkeypatch.setenv("ASEP_LANES", lanes)                  # read when the engine is created
    cfg, w, graph = _setup(dtype)
    lib, h = _lib.init_device(0), graph.handle(0)
    sizes = [[(5, 70), (9, 130), (16, 16), (4, 65)][i % 4] for i in range(13)]
    pages = [_seam_page(s[0], s[1], 40 + i) for i, s in enumerate(sizes)]
    single = [helper.get_net_output(p, graph, "0").copy() for p in pages]
    for i in range(4):                                       # pages of one size are different pages
        assert not np.array_equal(single[i], single[i + 4])
    batch = _batch(lib, h, pages)
    for b in range(13):
        assert np.array_equal(batch[b], single[b]), f"page {b} {sizes[b]}: differs from the single-page call"
    rev = _batch(lib, h, pages[::-1])[::-1]
    for b in range(13):
        assert np.array_equal(rev[b], single[b]), f"reversed order, page {b} {sizes[b]}: differs from the single-page call"
    _, prof = _batch(lib, h, pages, profile=True)
    assert kp.calls(prof, "pyr_tap_kernel<1>", "unet_down_1/conv1 tap") == 2, sorted(prof)
    assert kp.calls(prof, "pyr_tap_kernel<1>", "unet_up_0/conv1 tap") == 2, sorted(prof)
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_colour_batch_with_mvn_uses_each_page_its_own_statistics(dtype):
    """pages of scales 255, 40, 255 and 120: {mean, 1/std} of another page would move a result by far more than a rounding"""
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    cfg, w, graph = _setup(dtype, channels=3, mvn=True)
    lib, h = _lib.init_device(0), graph.handle(0)
    sizes, scales = [(9, 130), (16, 16), (5, 70), (37, 53)], [255.0, 40.0, 255.0, 120.0]
    pages = [_seam_page(s[0], s[1], 60 + i, 3, k) for i, (s, k) in enumerate(zip(sizes, scales))]
    # the raw pages differ in mean and deviation by the factors above, so a tap that standardised with a neighbour's pair would feed another image
    means = [float(p.mean()) for p in pages]
    assert means[0] > 1.5 * means[3] > 3 * means[1]
    single = [helper.get_net_output(p, graph, "0").copy() for p in pages]
    batch = _batch(lib, h, pages)
    for b in range(4):
        assert np.array_equal(batch[b], single[b]), f"page {b} {sizes[b]} x {scales[b]}: differs from the single-page call"
    _check(graph, cfg, w, pages[1], f"{dtype} colour mvn 16x16 x 40")     # and the single-page call is the restatement's
    graph.close()


# ---- the widest tapped conv1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels", [1, 3], ids=["gray", "colour"])
def test_feat_root_16_reaches_the_documented_bound_of_256_channels(dtype, channels):
    """PYR_MAX_COUT (csrc/pyr_kernels.h): level 4 of a feat_root 16 net has 256 channels, the widest conv1 the tap serves"""
    cfg, w, graph = _setup(dtype, feat_root=16, channels=channels)
    assert cfg.feat(4) == 256
    _check(graph, cfg, w, _page(16, 16, 8, channels), f"{dtype} feat_root 16 ch{channels} 16x16")
    graph.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_conv1_wider_than_the_bound_is_refused_at_load(dtype):
    """feat_root 32: level 4 has 512 channels -- served or refused with a message, never a wrong result: refused at load, nothing is launched"""
    from citlab_article_separation_new_amd import _lib
    cfg, w, graph = _setup(dtype, feat_root=32, channels=3)
    with pytest.raises(_lib.AsepError, match=r"unet_down_4/conv1 has 512 output channels.*up to 256"):
        graph.handle(0)


# ---- seeded fuzz -------------------------------------------------------------------------------------------------------------------------------
def _fuzz_cases():
    rng = np.random.default_rng(20261)
    return [(int(rng.integers(1, 151)), int(rng.integers(1, 151)), int(rng.choice([1, 3])), bool(rng.integers(2)), bool(rng.integers(2)))
            for _ in range(6)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,W,channels,mvn,inp4up", _fuzz_cases(), ids=str)
def test_seeded_pages_against_the_restatement(dtype, H, W, channels, mvn, inp4up):
    print(f"\n{dtype}: {H}x{W} channels={channels} mvn={mvn} inp4up={inp4up}")
    cfg, w, graph = _setup(dtype, channels=channels, mvn=mvn, inp4up=inp4up)
    img = _seam_page(H, W, 7 * H + W, channels, 255.0 if mvn else 1.0)
    _check(graph, cfg, w, img, f"{dtype} fuzz {H}x{W} ch{channels} mvn={mvn} inp4up={inp4up}")
    graph.close()
