"""What --device_jpeg buys or costs on one GPU: synthetic 3000 x 4500 scans, gray and colour 4:2:0 at quality 90, written by Pillow.

    python scripts/jpeg_decode_bench.py --out profiles/jpeg/gpu.json [--pages 64] [--workers 14] [--fixed_height 1500]

Per flavour: CPU ms per page of load_image_bgr (Pillow / libjpeg-turbo, one process) and of load_jpeg_coefficients (the Huffman decode
alone), the bytes and the time of the upload either way (page-locked memory, device events), and the device time of the kernels
(device events, two warming calls, median of 20) against their HBM bytes at 8 TB/s.  Then pages/s of the separator command line's path
on --pages JPEG files with and without the flag, same process, same model."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from PIL import Image

W, H = 3000, 4500
HBM_BYTES_PER_S = 8e12


def _median_ms(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def _event_us(fn, stream, warm=2, n=20):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--workers", type=int, default=14)
    ap.add_argument("--fixed_height", type=int, default=1500)
    args = ap.parse_args()
    import ctypes as C
    import torch
    from citlab_article_separation_new_amd import _lib, host_util, image_io, image_ops, net_post_processing_helper as helper, synth
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.separator_net_post_processor import SeparatorNetPostProcessor
    from citlab_article_separation_new_amd.weights import init_aru_weights
    result = {"page": [W, H], "quality": 90, "device": torch.cuda.get_device_name(0), "flavours": {}, "command_line": {}}
    lib, ws = image_ops._workspace(0)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    with tempfile.TemporaryDirectory(prefix="asep_jpeg_") as tmp:
        os.makedirs(os.path.join(tmp, "page"))
        gray = [synth.synth_page(k, W, H) for k in range(4)]
        files = {"gray": [], "colour420": []}
        for k, g in enumerate(gray):
            files["gray"].append(os.path.join(tmp, f"g{k}.jpg"))
            Image.fromarray(g).save(files["gray"][-1], quality=90)
            tint = np.stack([g, np.roll(g, 2, axis=1), (g.astype(np.int32) * 7 // 8).astype(np.uint8)], axis=-1)
            files["colour420"].append(os.path.join(tmp, f"c{k}.jpg"))
            Image.fromarray(tint).save(files["colour420"][-1], quality=90, subsampling=2)
        for name, paths in files.items():
            p = paths[0]
            page = image_io.load_jpeg_coefficients(p)
            assert page is not None
            pix = image_io.load_image_bgr(p).copy()            # (Pillow hands out read-only views)
            r = {"file_bytes": os.path.getsize(p),
                 "cpu_ms_load_image_bgr": _median_ms(lambda: image_io.load_image_bgr(p), 5),
                 "cpu_ms_load_jpeg_coefficients": _median_ms(lambda: image_io.load_jpeg_coefficients(p), 5),
                 "upload_bytes_pixels": int(pix.nbytes), "upload_bytes_coefficients": int(page.coef.nbytes)}
            h_pix, h_coef = torch.from_numpy(pix).pin_memory(), torch.from_numpy(page.coef).pin_memory()
            d_pix, d_coef = torch.empty_like(h_pix, device="cuda:0"), torch.empty_like(h_coef, device="cuda:0")
            r["upload_us_pixels"] = _event_us(lambda: d_pix.copy_(h_pix, non_blocking=True), stream)
            r["upload_us_coefficients"] = _event_us(lambda: d_coef.copy_(h_coef, non_blocking=True), stream)
            out = torch.empty(pix.shape, dtype=torch.uint8, device="cuda:0")

            def kernels():
                _lib.check(lib.asep_jpeg_pixels_dev(ws, C.byref(page.info), d_coef.data_ptr(), page.qt.ctypes.data, _lib.JPEG_ORDERS["bgr"],
                                                    out.data_ptr(), sp), "asep_jpeg_pixels_dev")
            r["kernel_us"] = _event_us(kernels, stream)
            assert np.array_equal(out.cpu().numpy(), pix), "the device page differs from Pillow's"
            samples = page.coef.size
            # coefficients in (2 B) and samples out (1 B); colour: planes read again (1 B per sample at most) and 3 B per pixel out
            hbm = 3 * samples + (0 if page.ncomp == 1 else samples + 3 * W * H)
            r["hbm_bytes"] = int(hbm)
            r["hbm_floor_us"] = hbm / HBM_BYTES_PER_S * 1e6
            r["device_path_us_upload_plus_kernels"] = r["upload_us_coefficients"] + r["kernel_us"]
            r["upload_costs_more_than_pixels"] = r["upload_us_coefficients"] > r["upload_us_pixels"]
            result["flavours"][name] = r
            print(name, json.dumps(r), flush=True)
        # ---- the separator command line's path on JPEG files, with and without the flag ----
        cfg = AruConfig()
        graph = helper.AruGraph(init_aru_weights(cfg, 21, logit_scale=0.05), cfg)
        for name, paths in files.items():
            listed = []
            for k in range(args.pages):                  # four real files, the rest are links to them
                p = os.path.join(tmp, f"{name}_{k:03d}.jpg")
                os.symlink(paths[k % 4], p)
                listed.append(p)
            for flag in (False, True, False, True):      # interleaved, two runs each: the box's drift shows as the spread
                warm = SeparatorNetPostProcessor(listed[:2], graph, args.fixed_height, 1.0, 0.5, "0", host_workers=0)
                warm.device_jpeg = flag
                warm.run()
                proc = SeparatorNetPostProcessor(listed, graph, args.fixed_height, 1.0, 0.5, "0", host_workers=args.workers)
                proc.device_jpeg = flag
                t0 = time.perf_counter()
                proc.run()
                dt = time.perf_counter() - t0
                row = {"pages_per_s": args.pages / dt, "owner_device_fraction": proc.device_seconds / dt,
                       "owner_wait_fraction": proc.wait_seconds / dt, "first_page_s": proc.first_page_seconds}
                result["command_line"].setdefault(name, {}).setdefault("device_jpeg" if flag else "pillow", []).append(row)
                print(name, "device_jpeg" if flag else "pillow", json.dumps(row), flush=True)
        result["command_line_setup"] = {"pages": args.pages, "host_workers": args.workers, "fixed_height": args.fixed_height, "mode": "separator",
                                        "cpus": host_util.effective_cpus()}      # what the container may use, not the machine's count
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
