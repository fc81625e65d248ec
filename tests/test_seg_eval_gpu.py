"""Segmentation net evaluation on the device (csrc/seg_eval_kernels.h, seg_eval.py) against the numpy restatement of
plot_net_output.py:196-241 (tests/seg_eval_ref.py, held to the reference's functions by tests/test_seg_eval_host.py).

Counters, masks and blends are integers and bytes: everything is compared for equality.

Shapes: a thread takes 4 pixels, a wave 256, a block 4096 (1024 per step).  1x1, 1x63, 3x64, 2x65, 5x257 and 67x130 put the
page's end inside a thread's four pixels, at a wave's end, one pixel behind it, behind a step and in a third block; C in
{1, 2, 3, 5, 8} covers the widths whose 4 C floats are 1, 2, 3, 5 and 8 vector loads."""
import os

import numpy as np
import pytest

import seg_eval_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (3, 64), (2, 65), (5, 257), (67, 130)]
CLASSES = [1, 2, 3, 5, 8]
MAXP = 12                           # pages of one launch (csrc/launch_plan.h)
F06 = np.float32(0.6)
SPECIAL = np.array([0.0, 1.0, F06, np.nextafter(F06, np.float32(1)), np.nextafter(F06, np.float32(0)), 0.5, 0.25, 0.75, 1e-30,
                    np.nextafter(np.float32(1), np.float32(0)), 1.0 / 255, 254.5 / 255], np.float32)


def _prob(H, W, C, seed):
    """half of the pixels from SPECIAL (exact 0 and 1, both sides of 0.6, ties), half random"""
    rng = np.random.default_rng(seed)
    p = rng.random((H, W, C), dtype=np.float32)
    pick = rng.random((H, W, C)) < 0.5
    p[pick] = SPECIAL[rng.integers(0, len(SPECIAL), size=int(pick.sum()))]
    tie = rng.random((H, W)) < 0.2
    p[tie] = p[tie][:, :1]                                   # every class the same value
    return p


def _gt(H, W, C, seed):
    rng = np.random.default_rng(seed + 1000)
    return np.array([0, 255, 255, 0, 128, 1, 254], np.uint8)[rng.integers(0, 7, size=(C, H, W))]


@pytest.fixture(scope="module")
def ev():
    from citlab_article_separation_new_amd import seg_eval
    e = seg_eval.SegEvaluator(0)
    yield e
    e.close()


def _run(ev, probs, gts=None, masks=False, thr=False):
    """-> (counters uint64 [n, SLOTS], masks as numpy [C,H,W] per page or None)"""
    import torch
    d_probs = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in probs]
    d_gts = None if gts is None else [None if g is None else torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in gts]
    cnt, d_masks = ev.score_pages(d_probs, d_gts, want_masks=masks, mask_threshold=thr)
    return cnt, (None if d_masks is None else [m.cpu().numpy() for m in d_masks])


def _want(prob, gt, thr):
    """the counter block the helper's figures make"""
    from citlab_article_separation_new_amd import seg_eval as S
    r = ref.score(prob, gt, mask_threshold=thr)
    H, W, C = prob.shape
    w = np.zeros(S.SLOTS, np.uint64)
    w[S.UNSURE], w[S.PIXELS], w[S.HAS_GT] = r["unsure"], H * W, gt is not None
    for c in range(C):
        w[S.CLASS + c] = r["class_count"][c]
        if gt is not None:
            w[S.EQUAL + c], w[S.TP + c], w[S.FP + c], w[S.FN + c] = r["equal"][c], r["tp"][c], r["fp"][c], r["fn"][c]
    return w, r["masks"]


_REF_CACHE = {}


def _want_cached(key, prob, gt, thr):
    k = (key, gt is not None, thr)
    if k not in _REF_CACHE:
        _REF_CACHE[k] = _want(prob, gt, thr)
    return _REF_CACHE[k]


@pytest.mark.parametrize("C", CLASSES)
def test_seam_shapes_every_mode(ev, C):
    probs = [_prob(H, W, C, 10 * C + i) for i, (H, W) in enumerate(SHAPES)]
    gts = [_gt(H, W, C, 10 * C + i) for i, (H, W) in enumerate(SHAPES)]
    for thr in (False, True):
        for with_gt in (False, True):
            for with_masks in (False, True):
                cnt, masks = _run(ev, probs, gts if with_gt else None, with_masks, thr)
                assert ev.launches() == [f"seg_eval_kernel<{C},{'true' if thr else 'false'}>"]
                for b, (p, g) in enumerate(zip(probs, gts)):
                    want, want_masks = _want_cached((C, b), p, g if with_gt else None, thr)
                    assert np.array_equal(cnt[b], want), (SHAPES[b], thr, with_gt, with_masks, cnt[b], want)
                    if with_masks:
                        assert np.array_equal(masks[b], want_masks), (SHAPES[b], thr)


def test_special_planes(ev):
    H, W, C = 5, 257, 3
    rng = np.random.default_rng(5)
    ties = np.repeat(rng.random((H, W, 1), dtype=np.float32), C, axis=2)
    exact = rng.integers(0, 2, size=(H, W, C)).astype(np.float32)
    inside = np.clip(rng.random((H, W, C), dtype=np.float32), 1e-6, 1 - 1e-6).astype(np.float32)
    gt128 = _gt(H, W, C, 3)
    gt128[:, ::2, ::3] = 128
    background = np.zeros((C, H, W), np.uint8)
    background[0] = 255                                       # class 0 is the background channel: everything is background
    probs, gts = [ties, exact, inside, inside, exact], [gt128, gt128, background, gt128, background]
    for thr in (False, True):
        cnt, masks = _run(ev, probs, gts, True, thr)
        for b in range(len(probs)):
            want, want_masks = _want(probs[b], gts[b], thr)
            assert np.array_equal(cnt[b], want), (b, thr)
            assert np.array_equal(masks[b], want_masks), (b, thr)
        assert cnt[0][8] == H * W and cnt[0][9] == cnt[0][10] == 0            # all ties: the first class takes every pixel
        assert cnt[1][0] == 0 and cnt[2][0] == H * W * C                       # unsure: none of exact 0 / 1, all of (0, 1)


def test_unaligned_buffers_take_the_scalar_paths(ev):
    """probabilities 4 bytes off a 16-byte boundary, ground truth and masks of odd plane sizes (planes 1 and 2 start off a word)"""
    import torch
    H, W, C = 7, 131, 3
    p, g = _prob(H, W, C, 77), _gt(H, W, C, 77)
    buf = torch.zeros(H * W * C + 1, dtype=torch.float32, device="cuda")
    d_p = buf[1:].view(H, W, C)
    d_p.copy_(torch.from_numpy(p))
    assert d_p.data_ptr() % 16 == 4 and d_p.is_contiguous()
    gbuf = torch.zeros(C * H * W + 1, dtype=torch.uint8, device="cuda")
    d_g = gbuf[1:].view(C, H, W)
    d_g.copy_(torch.from_numpy(g))
    for thr in (False, True):
        cnt, d_masks = ev.score_pages([d_p], [d_g], want_masks=True, mask_threshold=thr)
        want, want_masks = _want(p, g, thr)
        assert np.array_equal(cnt[0], want)
        assert np.array_equal(d_masks[0].cpu().numpy(), want_masks)


def test_more_pages_than_one_launch_and_independence_of_the_call(ev):
    C = 2
    sizes = [SHAPES[i % len(SHAPES)] for i in range(MAXP + 3)]
    sizes[MAXP - 1], sizes[MAXP] = (67, 130), (1, 63)          # a small page behind a large one, across the launch boundary
    probs = [_prob(H, W, C, 300 + i) for i, (H, W) in enumerate(sizes)]
    gts = [_gt(H, W, C, 300 + i) for i, (H, W) in enumerate(sizes)]
    cnt, masks = _run(ev, probs, gts, True, False)
    assert ev.launches() == ["seg_eval_kernel<2,false>"] * 2
    again, _ = _run(ev, probs, gts, True, False)
    assert np.array_equal(cnt, again)                          # the call zeroes its counters
    for b in range(len(probs)):
        one, one_masks = _run(ev, [probs[b]], [gts[b]], True, False)
        assert np.array_equal(cnt[b], one[0]), b
        assert np.array_equal(masks[b], one_masks[0]), b
        want, want_masks = _want(probs[b], gts[b], False)
        assert np.array_equal(cnt[b], want) and np.array_equal(masks[b], want_masks), b
    # pages with and without ground truth in one call
    mixed, _ = _run(ev, probs[:3], [gts[0], None, gts[2]], False, True)
    for b, g in enumerate([gts[0], None, gts[2]]):
        assert np.array_equal(mixed[b], _want(probs[b], g, True)[0]), b
    # a page after a larger page (the handle has served 15 pages of up to 67 x 130): the same as alone on a fresh handle
    from citlab_article_separation_new_amd import seg_eval
    fresh = seg_eval.SegEvaluator(0)
    try:
        alone, _ = _run(fresh, [probs[1]], [gts[1]], False, False)
    finally:
        fresh.close()
    assert np.array_equal(alone[0], cnt[1])


def test_counters_of_a_512_page_equal_numpy_int64(ev):
    from citlab_article_separation_new_amd import seg_eval as S
    H = W = 512
    p, g = _prob(H, W, 2, 9), _gt(H, W, 2, 9)
    cnt, _ = _run(ev, [p], [g], False, False)
    am = np.argmax(p, axis=2)
    assert int(cnt[0][S.UNSURE]) == np.sum((p > 0) & (p < 1), dtype=np.int64)
    for c in range(2):
        assert int(cnt[0][S.CLASS + c]) == np.sum(am == c, dtype=np.int64)
        assert int(cnt[0][S.EQUAL + c]) == np.sum(((g[c] == 255) & (am == c)) | ((g[c] == 0) & (am != c)), dtype=np.int64)
        assert int(cnt[0][S.TP + c]) + int(cnt[0][S.FN + c]) == np.sum(g[c] == 255, dtype=np.int64)
        assert int(cnt[0][S.TP + c]) + int(cnt[0][S.FP + c]) == np.sum(am == c, dtype=np.int64)
    assert int(cnt[0][S.PIXELS]) == H * W and ev.kernel_us > 0


@pytest.mark.parametrize("shape", [(1, 1), (2, 65), (67, 130)])
def test_blend(ev, shape):
    import torch
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    scan = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    scan.reshape(-1)[::3] = 0
    scan.reshape(-1)[1::5] = 255
    d_scan = torch.from_numpy(scan).cuda()
    masks = {"mixed": np.array([0, 255, 254, 128], np.uint8)[rng.integers(0, 4, size=(H, W))],
             "zeros": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    for name, mask in masks.items():
        got = ev.blend(d_scan, torch.from_numpy(mask).cuda()).cpu().numpy()
        assert np.array_equal(got, ref.blend(scan, mask)), name
    assert np.array_equal(d_scan.cpu().numpy(), scan)
    # in place, as the ground truth side of plot_with_gt works (:249); and from a scan that starts off a word
    buf = torch.zeros(H * W * 3 + 1, dtype=torch.uint8, device="cuda")
    d_off = buf[1:].view(H, W, 3)
    d_off.copy_(d_scan)
    res = ev.blend(d_off, torch.from_numpy(masks["mixed"]).cuda(), out=d_off)
    assert res.data_ptr() == d_off.data_ptr()
    assert np.array_equal(d_off.cpu().numpy(), ref.blend(scan, masks["mixed"]))
    for color in ((0, 0, 0), (255, 255, 255), (1, 2, 3)):
        got = ev.blend(d_scan, torch.from_numpy(masks["full"]).cuda(), color=color).cpu().numpy()
        assert np.array_equal(got, ref.blend(scan, masks["full"], color=color)), color


# ---- end to end: the command line's function over PNG files, a tiny random net ------------------------------------------
E2E_SIZES = [(72, 88), (61, 77), (88, 56), (64, 64)]        # (h, w) of the scans


@pytest.fixture(scope="module")
def e2e_files(tmp_path_factory):
    """a folder with four gray scans, their C2 ground truth, a list file and a 2-class RU net of three scale levels"""
    from PIL import Image
    from citlab_article_separation_new_amd import weights as W
    from citlab_article_separation_new_amd.config import AruConfig
    root = tmp_path_factory.mktemp("seg_eval_e2e")
    os.makedirs(root / "C2")
    cfg = AruConfig(graph="RU", n_classes=2, scale_space_num=3)
    w = W.init_aru_weights(cfg, 4321, bias_jitter=0.05, logit_scale=0.5)
    W.save_weights(str(root / "net.asepw"), w, {"aru_cfg": cfg.to_dict()})
    rng = np.random.default_rng(99)
    paths, scans, gts = [], [], []
    for k, (h, wd) in enumerate(E2E_SIZES):
        scan = np.clip(rng.normal(215, 12, size=(h, wd)), 0, 255)                   # paper, then dark blocks and two rules
        for _ in range(12):
            y, x = int(rng.integers(0, h - 6)), int(rng.integers(0, wd - 10))
            scan[y:y + 4, x:x + int(rng.integers(4, 10))] = rng.integers(10, 90)
        scan[h // 3, 4:wd - 4] = 0
        scan[5:h - 5, wd // 2] = 255
        scan = np.ascontiguousarray(scan.astype(np.uint8))
        Image.fromarray(scan).save(root / f"page{k}.png")
        fg = rng.random((h, wd)) < 0.3
        planes = np.stack([np.where(fg, 0, 255), np.where(fg, 255, 0)]).astype(np.uint8)
        planes[1, ::7, ::5] = 128
        for i in range(2):
            Image.fromarray(planes[i]).save(root / "C2" / f"page{k}_GT{i}.png")
        paths.append(str(root / f"page{k}.png"))
        scans.append(scan)
        gts.append(planes)
    with open(root / "pages.lst", "w") as f:
        f.write("\n".join(paths) + "\n")
    return {"root": root, "paths": paths, "scans": scans, "gts": gts, "weights": w, "cfg": cfg}


def _single_page_probabilities(files, dtype):
    """what asep_aru_forward returns for each page on its own"""
    from dataclasses import replace
    from citlab_article_separation_new_amd import image_ops, net_post_processing_helper as helper
    graph = helper.AruGraph(files["weights"], replace(files["cfg"], compute_dtype=dtype))
    try:
        return [helper.get_net_output(image_ops.scale_and_gray(s, None, 1.0, want_image=False)[1], graph, "0") for s in files["scans"]]
    finally:
        graph.close()


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path))


@pytest.mark.parametrize("dtype", ["f32s", "bf16"])
def test_end_to_end_lines_and_files(e2e_files, dtype, tmp_path, monkeypatch):
    from citlab_article_separation_new_amd import seg_eval
    files = e2e_files
    probs = _single_page_probabilities(files, dtype)
    lst, net = str(files["root"] / "pages.lst"), str(files["root"] / "net.asepw")
    n = len(probs)

    # 1. counters only: the printed lines; the scoring kernel ran once per group and only counter blocks came to the host
    ev = seg_eval.SegEvaluator(0)
    lines = []

    def no_copy(self, t):
        raise AssertionError("a tensor was copied to the host on the counters-only path")
    with monkeypatch.context() as m:
        m.setattr(seg_eval.SegEvaluator, "to_host", no_copy)
        res = seg_eval.plot_net_output(net, lst, "", rescale=1.0, fixed_height=0, calculate_accuracy=True, dtype=dtype,
                                       pages_per_call=3, out=lines.append, evaluator=ev)
    assert ev.d2h_bytes == n * seg_eval.SLOTS * 8
    assert ev.launches() == ["seg_eval_kernel<2,false>"]       # the last group's call
    ev.close()
    want_lines, accs = [], []
    for k in range(n):
        r = ref.score(probs[k], files["gts"][k])
        h, w = E2E_SIZES[k]
        want_lines += ref.page_lines(r, h * w)
        accs.append(ref.accuracy(r))
    want_lines.append("Overall Accuracy =  " + str(sum(accs) / len(accs)))
    assert [l for l in lines if not l.startswith("Addition")] == want_lines
    assert len([l for l in lines if l.startswith("Addition (not in the reference)")]) == 2 * n
    assert res["overall"] == sum(accs) / len(accs)

    # 2. the written files, page by page and three pages per call: plain masks, thresholded (the flag's value is not the threshold),
    #    blended over the scan, with the ground truth half
    for mode, kw in (("plain", {}), ("thr", {"mask_threshold": 0.9}), ("img", {"plot_with_img": True}),
                     ("gt", {"plot_with_gt": True, "mask_threshold": 0.9}), ("img_gt", {"plot_with_img": True, "plot_with_gt": True})):
        folders = {}
        for per_call in (1, 3):
            folder = tmp_path / f"{mode}_{per_call}"
            os.makedirs(folder)
            got_lines = []
            seg_eval.plot_net_output(net, lst, str(folder), rescale=1.0, fixed_height=0, calculate_accuracy=True, dtype=dtype,
                                     pages_per_call=per_call, out=got_lines.append, show_plot=True, **kw)
            folders[per_call] = folder
            thr = bool(kw.get("mask_threshold"))
            want_lines = []
            for k in range(n):
                r = ref.score(probs[k], files["gts"][k], mask_threshold=thr)
                want_lines += ref.page_lines(r, E2E_SIZES[k][0] * E2E_SIZES[k][1])
                bgr = np.repeat(files["scans"][k][:, :, None], 3, axis=2)
                images = ref.save_images(bgr, r["masks"], files["gts"][k], kw.get("plot_with_gt", False), kw.get("plot_with_img", False))
                for cl in range(2):
                    name = f"page{k}_OUT{cl}.png"
                    assert np.array_equal(_read(folder / name), images[cl]), (mode, per_call, name)
            body = [l for l in got_lines if not l.startswith(("Addition", "show_plot", "Overall"))]
            assert body == want_lines, (mode, per_call)
            assert sum(l.startswith("show_plot") for l in got_lines) <= 1
        for name in sorted(os.listdir(folders[1])):
            assert open(folders[1] / name, "rb").read() == open(folders[3] / name, "rb").read(), (mode, name)
        assert len(os.listdir(folders[1])) == len(os.listdir(folders[3])) == 2 * n


def test_ground_truth_of_another_size_is_refused(e2e_files, tmp_path):
    from PIL import Image
    from citlab_article_separation_new_amd import seg_eval
    files = e2e_files
    os.makedirs(tmp_path / "C2")
    Image.fromarray(files["scans"][0]).save(tmp_path / "p.png")
    for i in range(2):
        Image.fromarray(np.zeros((36, 44), np.uint8)).save(tmp_path / "C2" / f"p_GT{i}.png")
    with pytest.raises(seg_eval.GroundTruthSizeError, match="OpenCV's bilinear default"):
        seg_eval.plot_net_output(str(files["root"] / "net.asepw"), [str(tmp_path / "p.png")], "", rescale=1.0, fixed_height=0,
                                 calculate_accuracy=True, out=lambda s: None)
