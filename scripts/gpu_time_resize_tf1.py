"""The relation net's resize kernel alone on one 4500 x 3000 page -> 1024 x 683: gray, R, G, B kept, and luma.  Run it under
`rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/gpu_time_resize_tf1.py` for the kernel's own time; it also prints the time
of the device entry between two events (launch included).

    python scripts/gpu_time_resize_tf1.py [repeats=20]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def main():
    import torch
    from citlab_article_separation_new_amd import gnn_input, image_ops
    H, W = 4500, 3000
    h, w = gnn_input.compute_new_size(H, W, 256, 1024)
    rng = np.random.default_rng(0)
    for name, channels, mode in (("gray keep", 1, "keep"), ("rgb keep", 3, "keep"), ("rgb luma", 3, "luma")):
        page = torch.from_numpy(rng.integers(0, 256, size=(H, W, channels), dtype=np.uint8)).cuda()
        image_ops.resize_tf1_dev(page, h, w, mode)                                     # (first launch: code object load)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(repeats):
            image_ops.resize_tf1_dev(page, h, w, mode)
        t1.record()
        torch.cuda.synchronize()
        print(f"{name}: {H} x {W} x {channels} -> {h} x {w}: {t0.elapsed_time(t1) / repeats * 1e3:.1f} us per call between events "
              f"({repeats} calls back to back)", flush=True)


if __name__ == "__main__":
    main()
