"""Segmentation net evaluation on one MI355X: the scoring call (asep_seg_eval_pages_dev) per 3000 x 4500 page, C = 2 and 3.

Per C and mode (counters with ground truth; + masks; + threshold): the device time of the scoring launch per page (device
events around the launches, warmed, the median of --repeats calls of --pages pages), its algorithmic bytes (4 C of
probabilities + C of ground truth in, C of masks out per pixel) over that time against the 8 TB/s of HBM, and the wall time
of the whole call (launch, counters back, synchronise).  In the same run: what the host would do instead -- the copy of the
page's float32 [H,W,C] to the host, and a vectorised numpy restatement of plot_net_output.py:196-241 on the same arrays in
row bands on --threads threads.  The reference's own triple Python loop over every pixel (:221-226) is timed on a 256 x 256
page and named separately.  Behind the forward: asep_aru_forward_batch_dev2 alone and followed by the scoring call.

Usage:  python scripts/seg_eval_bench.py --out profiles/seg_eval/gpu.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
H, W = 4500, 3000


def med(xs):
    return float(np.median(xs))


def page_bytes(ncls, gt, masks):
    return H * W * (4 * ncls + (ncls if gt else 0) + (ncls if masks else 0))


def make_pages(n, ncls, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    probs, gts = [], []
    for _ in range(n):
        p = torch.softmax(6.0 * torch.randn((H, W, ncls), device="cuda", generator=g), dim=2)
        sure = torch.rand((H, W), device="cuda", generator=g) < 0.3            # pixels where the net is sure: exact 0 / 1
        p[sure] = torch.nn.functional.one_hot(p[sure].argmax(dim=1), ncls).float()
        probs.append(p.contiguous())
        gts.append(torch.where(torch.rand((ncls, H, W), device="cuda", generator=g) < 0.5, 255, 0).to(torch.uint8))
    return probs, gts


def numpy_band(p, gt, thr):
    """plot_net_output.py:196-241 of a band of rows, vectorised -> (unsure, class_count, equal)"""
    ncls = p.shape[2]
    unsure = int(np.sum((0 < p) & (p < 1)))
    if thr:
        p = np.array(p > 0.6, np.int32)
    am = np.argmax(p, axis=2)
    cc = [int(np.sum(am == c)) for c in range(ncls)]
    eq = [int(np.sum(((gt[c] == 255) & (am == c)) | ((gt[c] == 0) & (am != c)))) for c in range(ncls)]
    return unsure, cc, eq


def numpy_page(p, gt, thr, threads):
    bands = np.array_split(np.arange(H), threads * 2)
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(lambda r: numpy_band(p[r[0]:r[-1] + 1], gt[:, r[0]:r[-1] + 1], thr), bands))
    ncls = p.shape[2]
    return (sum(x[0] for x in parts), [sum(x[1][c] for x in parts) for c in range(ncls)],
            [sum(x[2][c] for x in parts) for c in range(ncls)])


def python_loop_seconds(size=256, ncls=2):
    """the loop of :221-226 as the reference has it, on a size x size page"""
    out_img = np.random.default_rng(0).random((1, size, size, ncls), dtype=np.float32)
    t0 = time.perf_counter()
    values = np.argmax(out_img, axis=3)
    one_hot = np.zeros_like(out_img)
    counts = {"class_" + str(i): 0 for i in range(ncls)}
    for i in range(out_img.shape[0]):
        for j in range(out_img.shape[1]):
            for k in range(out_img.shape[2]):
                argmax = values[i, j, k]
                one_hot[i, j, k, argmax] = 1
                counts["class_" + str(argmax)] += 1
    return time.perf_counter() - t0


def bench_scoring(ncls, pages, repeats, threads):
    import torch
    from citlab_article_separation_new_amd import seg_eval as S
    ev = S.SegEvaluator(0)
    probs, gts = make_pages(pages, ncls, 100 + ncls)
    res = {"C": ncls, "pages_per_call": pages, "modes": {}}
    for mode, (gt, masks, thr) in {"counters": (True, False, False), "counters_masks": (True, True, False),
                                   "counters_masks_threshold": (True, True, True), "counters_no_gt": (False, False, False)}.items():
        us, wall = [], []
        for it in range(repeats + 2):                                   # two warming calls
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cnt, _ = ev.score_pages(probs, gts if gt else None, want_masks=masks, mask_threshold=thr)
            dt = time.perf_counter() - t0
            if it >= 2:
                us.append(ev.kernel_us / pages)
                wall.append(dt / pages)
        b = page_bytes(ncls, gt, masks)
        res["modes"][mode] = {"kernel_us_per_page": med(us), "kernel_us_per_page_min": float(min(us)), "kernel_us_per_page_max": float(max(us)),
                              "call_wall_us_per_page": 1e6 * med(wall), "bytes_per_page": b, "bytes_per_s": b / (1e-6 * med(us)),
                              "share_of_8TBps": b / (1e-6 * med(us)) / HBM_BYTES_PER_S}
    # the host's way on the same arrays: the copy, then numpy on `threads` threads; results must agree
    cnt, _ = ev.score_pages(probs[:1], gts[:1])
    copy_s, np_s = [], []
    for it in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_p, h_g = probs[0].cpu().numpy(), gts[0].cpu().numpy()
        copy_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        unsure, cc, eq = numpy_page(h_p, h_g, False, threads)
        np_s.append(time.perf_counter() - t0)
    assert unsure == int(cnt[0][S.UNSURE]) and cc == [int(cnt[0][S.CLASS + c]) for c in range(ncls)]
    assert eq == [int(cnt[0][S.EQUAL + c]) for c in range(ncls)]
    res["host_copy_ms_per_page"] = 1e3 * med(copy_s)
    res["numpy_ms_per_page"] = 1e3 * med(np_s)
    res["numpy_threads"] = threads
    res["numpy_equals_device"] = True
    ev.close()
    return res


def bench_behind_forward(dtype, pages, repeats):
    import torch
    from citlab_article_separation_new_amd import _lib, seg_eval as S, synth
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    from citlab_article_separation_new_amd.weights import init_aru_weights
    cfg = AruConfig(compute_dtype=dtype)
    graph = AruGraph(init_aru_weights(cfg, 1234, bias_jitter=0.05, logit_scale=0.05), cfg)
    lib = _lib.init_device(0)
    ev = S.SegEvaluator(0)
    imgs = [torch.from_numpy(synth.synth_page(k, W, H).astype(np.float32) / 255.0).cuda() for k in range(pages)]
    outs = [torch.empty((H, W, cfg.n_classes), dtype=torch.float32, device="cuda") for _ in range(pages)]
    gts = [torch.zeros((cfg.n_classes, H, W), dtype=torch.uint8, device="cuda") for _ in range(pages)]
    Ptr, Ints = C.c_void_p * pages, C.c_int32 * pages
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward():
        _lib.check(lib.asep_aru_forward_batch_dev2(graph.handle(0), pages, Ptr(*[t.data_ptr() for t in imgs]), Ints(*[H] * pages),
                                                   Ints(*[W] * pages), Ptr(*[t.data_ptr() for t in outs]), None, None, 0.0, sp), "forward")
    alone, both = [], []
    for it in range(repeats + 1):                                        # alternating, the first round warms
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        forward()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        forward()
        ev.score_pages(outs, gts)
        t2 = time.perf_counter()
        if it:
            alone.append((t1 - t0) / pages)
            both.append((t2 - t1) / pages)
    ev.close()
    graph.close()
    return {"dtype": dtype, "pages_per_call": pages, "forward_ms_per_page": 1e3 * med(alone), "forward_and_scoring_ms_per_page": 1e3 * med(both),
            "scoring_adds_ms_per_page": 1e3 * (med(both) - med(alone))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pages", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no_forward", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the MI355X and has no other path")
    result = {"page": [H, W], "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "scoring": [bench_scoring(c, args.pages, args.repeats, args.threads) for c in (2, 3)],
              "python_triple_loop_256x256_s": python_loop_seconds()}
    result["python_triple_loop_extrapolated_s_per_page"] = result["python_triple_loop_256x256_s"] * (H * W) / (256 * 256)
    if not args.no_forward:
        result["behind_forward"] = [bench_behind_forward(d, 2, 5) for d in ("f32s", "bf16")]
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
