"""The cases of tests/test_split_walk_down_gpu.py: a plain helper (no fixtures) shared by the test and the recorder of its expectations,
tests/golden/make_split_walk_down_golden.py.

A case = an f32s model with seeded weights in a fresh handle (ASEP_SPLIT_WALK set before the load), ONE asep_aru_forward_batch_dev2 call of the
case's pages, and the level-0 DOWN block's end points of every page at scale 0: its output d0 (scale_0_unet_down_0_conv) and what its 2 x 2 pool
feeds, the level-1 block's output (scale_0_unet_down_1_conv, a function of the pool alone); where the library publishes the pool itself
(scale_0_unet_down_0_pool) that too."""
import ctypes as C
import os
import zlib

import numpy as np

import launch_records as lr

# 160 x 132: the smallest page whose scale 0 walks; 203 x 389: scales 0 and 1 walk, H and W odd (the pool's last row and column are partial);
# 107 x 135: 86 walker rows = at least 2 x 32 + 20, so with the smallest band (32 rows) a seam falls inside it and an item runs 16 + 6 iterations
# of two rows = 44 image rows through a ring of 16
SEAM_PAGE = (107, 135)
SINGLE = [(160, 132), (203, 389), SEAM_PAGE]
BIG = np.float32(1000.0)

# (name, pages, image kind, per-page standardisation)
CASES = []
for _mvn in (False, True):
    _t = "mvn" if _mvn else "raw"
    for _s in SINGLE:
        CASES.append((f"rand_{_s[0]}x{_s[1]}_{_t}", [_s], "rand", _mvn))
    for _s in ((160, 132), SEAM_PAGE):
        CASES.append((f"border_{_s[0]}x{_s[1]}_{_t}", [_s], "border", _mvn))
    CASES.append((f"batch_{_t}", list(lr.PAGES), "rand", _mvn))

D0, D1, POOL = "scale_0_unet_down_0_conv", "scale_0_unet_down_1_conv", "scale_0_unet_down_0_pool"


def walk_region(H, W):
    """csrc/level0_plan.h: (n_strips, rows, fits)"""
    return (W - 4 - 32) // 24, 2 * ((H - 4 - 16) // 2), (W - 4 - 32) // 24 >= 4 and H - 4 - 16 >= 32


def walk_band(pages, num_cus, waves_per_cu):
    """csrc/level0_plan.h: the band of a walker launch over the pages that walk"""
    strip_rows = sum(n * r for n, r, fits in (walk_region(*s) for s in pages) if fits)
    band = min(256, max(32, strip_rows // (6 * waves_per_cu * num_cus)))
    return (band + 1) & ~1


def images(pages, kind, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for H, W in pages:
        img = rng.random((H, W), dtype=np.float32)
        if kind == "border":
            # large values where a wrong padding value would enter: the page's border pixels, and the image rows around the first rows of every
            # 32-row band of the walker (rows 16 + 32 b), which an item reads as the top of its window
            img[0, :] = img[-1, :] = BIG
            img[:, 0] = img[:, -1] = BIG
            for y in range(16, H, 32):
                img[max(y - 5, 0):y + 2, :] = BIG
        out.append(img)
    return out


def run(pages, kind, mvn, walk, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    """{end point name: [array of page 0, ...]} of one case with ASEP_SPLIT_WALK = walk, in a fresh handle"""
    import torch
    from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    for name in lr.switch_names():
        delenv(name)
    setenv("ASEP_SPLIT_WALK", walk)
    cfg = AruConfig(compute_dtype="f32s", mvn=mvn)
    key = ("split_walk_down", mvn)
    if key not in lr._weights:
        lr._weights[key] = init_aru_weights(cfg, 1234, bias_jitter=0.05, logit_scale=0.05)
    graph = helper.AruGraph(lr._weights[key], cfg)
    try:
        lib = _lib.init_device(0)
        h = graph.handle(0)
        B = len(pages)
        d_in = [torch.from_numpy(p).cuda() for p in images(pages, kind)]
        d_out = [torch.empty(s[0], s[1], cfg.n_classes, device="cuda") for s in pages]
        Arr, Ints = C.c_void_p * B, C.c_int32 * B
        rc = lib.asep_aru_forward_batch_dev2(h, B, Arr(*[t.data_ptr() for t in d_in]), Ints(*[s[0] for s in pages]), Ints(*[s[1] for s in pages]),
                                             Arr(*[t.data_ptr() for t in d_out]), None, None, 0.5, None)
        _lib.check(rc, "asep_aru_forward_batch_dev2")
        torch.cuda.synchronize()
        res = {}
        for n in (D0, D1, POOL):
            try:
                res[n] = [helper.get_endpoint(graph, (f"p{b}/" if b else "") + n) for b in range(B)]
            except _lib.AsepError:
                if n != POOL:
                    raise
    finally:
        graph.close()
    return res


def digest(a):
    """what the golden file keeps of a tensor: its shape, its float64 sum and sum of squares (as hex: exact), and the CRC-32 of its bytes"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    d = a.astype(np.float64)
    return {"shape": list(a.shape), "sum": float(d.sum()).hex(), "sum_sq": float((d * d).sum()).hex(), "crc32": zlib.crc32(a.tobytes())}
