"""What --device_huffman buys or costs on one GPU: the synthetic 3000 x 4500 quality-90 scans of scripts/jpeg_decode_bench.py, gray and
colour 4:2:0, without and with restart markers (one per MCU row).  One run, gates nothing.

    python scripts/jpeg_huffman_bench.py --out profiles/jpeg_huffman/gpu.json [--pages 64] [--workers 14] [--fixed_height 1500]

Per flavour: CPU ms per page of asep_jpeg_scan_prepare (image_io.load_jpeg_scan), of load_jpeg_coefficients and of load_image_bgr, one
process, median of 5; the bytes uploaded either way; the entropy decode on the device (asep_jpeg_entropy_dev: device events around the whole
call, which includes the host's read of the "changed" word after every launch of the fixed-point loop, two warming calls, median of 20),
its rounds, subsequences and subseq_bits; the coefficients are compared with the host decoder's.  Then pages/s of the separator command
line's path on --pages files with --device_jpeg alone and with --device_huffman added, two runs each, interleaved."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from PIL import Image

from jpeg_decode_bench import H, W, _event_us, _median_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--workers", type=int, default=14)
    ap.add_argument("--fixed_height", type=int, default=1500)
    ap.add_argument("--subseq_bits", type=int, default=0)
    args = ap.parse_args()
    import torch
    from citlab_article_separation_new_amd import host_util, image_io, net_post_processing_helper as helper, synth
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.separator_net_post_processor import SeparatorNetPostProcessor
    from citlab_article_separation_new_amd.weights import init_aru_weights
    result = {"page": [W, H], "quality": 90, "device": torch.cuda.get_device_name(0), "flavours": {}, "command_line": {}}
    stream = torch.cuda.current_stream()
    with tempfile.TemporaryDirectory(prefix="asep_huff_") as tmp:
        os.makedirs(os.path.join(tmp, "page"))
        files = {}
        for k in range(4):
            g = synth.synth_page(k, W, H)
            tint = np.stack([g, np.roll(g, 2, axis=1), (g.astype(np.int32) * 7 // 8).astype(np.uint8)], axis=-1)
            for name, img, kw in (("gray", g, {}), ("gray_rst", g, {"restart_marker_rows": 1}), ("colour420", tint, {"subsampling": 2}),
                                  ("colour420_rst", tint, {"subsampling": 2, "restart_marker_rows": 1})):
                files.setdefault(name, []).append(os.path.join(tmp, f"{name}{k}.jpg"))
                Image.fromarray(img).save(files[name][-1], quality=90, **kw)
        for name, paths in files.items():
            p = paths[0]
            page, scan = image_io.load_jpeg_coefficients(p), image_io.load_jpeg_scan(p)
            assert page is not None and scan is not None
            r = {"file_bytes": os.path.getsize(p), "segments": scan.n_segments,
                 "cpu_ms_scan_prepare": _median_ms(lambda: image_io.load_jpeg_scan(p), 5),
                 "cpu_ms_load_jpeg_coefficients": _median_ms(lambda: image_io.load_jpeg_coefficients(p), 5),
                 "cpu_ms_load_image_bgr": _median_ms(lambda: image_io.load_image_bgr(p), 5),
                 "upload_bytes_scan": int(scan.scan.nbytes + scan.segments.nbytes + 9104), "upload_bytes_coefficients": int(page.coef.nbytes),
                 "upload_bytes_pixels": int(page.width * page.height * (1 if page.ncomp == 1 else 3))}
            keep = {}

            def entropy():
                keep["out"] = image_io.jpeg_scan_entropy_to_device(scan, 0, stream, subseq_bits=args.subseq_bits)
            r["entropy_call_us"] = _event_us(entropy, stream)
            r["rounds"], r["subsequences"] = image_io.jpeg_entropy_rounds()
            r["subseq_bits"] = args.subseq_bits or 128
            r["launches"] = image_io.jpeg_device_launches()
            d_coef, d_status = keep["out"]
            assert int(d_status.cpu()[0]) == 0 and np.array_equal(d_coef.cpu().numpy(), page.coef), "the device's coefficients differ"

            def whole():
                keep["page"] = image_io.jpeg_scan_to_device(scan, 0, "bgr", stream, subseq_bits=args.subseq_bits)
            r["scan_to_page_us"] = _event_us(whole, stream)
            assert np.array_equal(keep["page"][0].cpu().numpy().reshape(page.height, page.width, -1),
                                  image_io.load_image_bgr(p).reshape(page.height, page.width, -1)), "the device page differs from Pillow's"
            result["flavours"][name] = r
            print(name, json.dumps(r), flush=True)
        # ---- the separator command line's path, --device_jpeg alone against --device_huffman added ----
        cfg = AruConfig()
        graph = helper.AruGraph(init_aru_weights(cfg, 21, logit_scale=0.05), cfg)
        for name in ("gray", "colour420"):
            listed = []
            for k in range(args.pages):                  # four real files, the rest are links to them
                p = os.path.join(tmp, f"{name}_{k:03d}.jpg")
                os.symlink(files[name][k % 4], p)
                listed.append(p)
            for flag in (False, True, False, True):      # interleaved, two runs each: the box's drift shows as the spread
                warm = SeparatorNetPostProcessor(listed[:2], graph, args.fixed_height, 1.0, 0.5, "0", host_workers=0)
                warm.device_jpeg, warm.device_huffman = True, flag
                warm.run()
                proc = SeparatorNetPostProcessor(listed, graph, args.fixed_height, 1.0, 0.5, "0", host_workers=args.workers)
                proc.device_jpeg, proc.device_huffman = True, flag
                t0 = time.perf_counter()
                proc.run()
                dt = time.perf_counter() - t0
                row = {"pages_per_s": args.pages / dt, "owner_device_fraction": proc.device_seconds / dt,
                       "owner_wait_fraction": proc.wait_seconds / dt, "first_page_s": proc.first_page_seconds,
                       "huffman_pages": proc.huffman_pages, "huffman_fallbacks": proc.huffman_fallbacks}
                result["command_line"].setdefault(name, {}).setdefault("device_huffman" if flag else "device_jpeg", []).append(row)
                print(name, "device_huffman" if flag else "device_jpeg", json.dumps(row), flush=True)
        result["command_line_setup"] = {"pages": args.pages, "host_workers": args.workers, "fixed_height": args.fixed_height, "mode": "separator",
                                        "cpus": host_util.effective_cpus()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
