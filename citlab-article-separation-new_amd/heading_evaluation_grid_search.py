"""Heading detection grid search: ``heading_evaluation_grid_search.py`` of the reference in one process and one GPU owner.

The reference starts ``heading_evaluation.py`` once per setting (449,064 settings for the seven fixed heights), each run
decoding every scan and measuring it again.  Here every page is measured once (distance transform, stroke width and text
height) and the net runs once per (page, fixed height); ``asep_heading_grid_eval`` scores all settings of a height in one
launch.  Outputs:

- ``--results`` (default ``<log_file_folder>/grid_results.csv``): one row per setting in the reference's order, both
  sw_th_thresh values included, the setting's floats and the 12 averages as ``repr``;
- the per-setting log files of heading_evaluation.py unless ``--no_setting_logs``.  Their name does not carry
  sw_th_thresh, so two settings share each name; the file holds the one the reference writes last under it, the larger
  sw_th_thresh (``min(stroke_width_thresh, text_height_thresh)``);
- the best settings by average binary F1 on stdout.

No ``<page>.xml.xml`` is written (the reference's grid leaves only the last run's copy).
"""
import argparse
import os
import sys
import time

import numpy as np

from . import heading_evaluation as he
from .net_post_processing_helper import _device_of
from .path_util import load_list_file

CHUNK = 8192          # settings per host metric / log batch (bounds the memory of the per-page values)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--path_to_gt_list", type=str, required=True, help='Path to GT image list')
    parser.add_argument("--path_to_pb", type=str, required=True, help='Path to the TensorFlow graph.')
    parser.add_argument("--log_file_folder", type=str, required=True, help='Path to the folder where the log files are stored')
    parser.add_argument("--num_processes", type=int, required=False, default=8,
                        help='Host worker processes that decode the images ahead of the GPU (<= 1: inline).')
    parser.add_argument("--fixed_heights", type=int, nargs="+", default=list(he.FIXED_HEIGHTS),
                        help="Fixed heights of the grid (default 600 ... 1200 in steps of 100).")
    parser.add_argument("--no_setting_logs", action="store_true", help="Write the CSV only, no per-setting log files.")
    parser.add_argument("--results", type=str, default=None, help="CSV path (default <log_file_folder>/grid_results.csv).")
    parser.add_argument("--gpu_devices", type=str, default='0', help="GPU device of the one owner.")
    parser.add_argument("--top", type=int, default=10, help="How many of the best settings to print.")
    return parser


def run_grid(image_paths, path_to_pb, fixed_heights, log_file_folder, results, setting_logs=True, host_workers=0,
             gpu_devices='0', timings=None):
    """Measure, score every setting of the grid, write the CSV (and the logs) -> (heights [N], tenths [N, 9], averages [N, 12]).
    ``timings`` (a dict) receives the wall time of each stage: the measurement stages of ``measure_pages`` and
    ``confidences_s`` (heading_confidences per height), ``kernel_s`` (asep_heading_grid_eval calls, one per height),
    ``kernel_us`` (their device time), ``metrics_s``, ``logs_s``, ``csv_s``, ``total_s``."""
    t_start = time.perf_counter()
    tm = {} if timings is None else timings
    gts, swth, nets = he.measure_pages(image_paths, path_to_pb, fixed_heights, gpu_devices, host_workers,
                                       timings=tm if timings is not None else None)
    heights, tenths = he.grid_settings(fixed_heights)
    averages = np.empty((len(tenths), len(he.METRICS)))
    device = _device_of(gpu_devices)
    tm.update(confidences_s=0.0, kernel_s=0.0, kernel_us=0.0, metrics_s=0.0, logs_s=0.0)
    for h in fixed_heights:
        t0 = time.perf_counter()
        gp = he.page_inputs(gts, swth, nets[h])
        sel = np.flatnonzero(heights == h)
        t1 = time.perf_counter()
        tm["confidences_s"] += t1 - t0
        counts = he.grid_eval(gp, tenths[sel], device)             # one launch for every setting of the height
        tm["kernel_us"] += he.last_kernel_us()
        t2 = time.perf_counter()
        tm["kernel_s"] += t2 - t1
        for c0 in range(0, len(sel), CHUNK):                       # host metrics and logs in batches of settings
            t2 = time.perf_counter()
            idx = sel[c0:c0 + CHUNK]
            per_page = he.page_metrics(counts[c0:c0 + CHUNK])
            averages[idx] = he.average_metrics(per_page)
            t3 = time.perf_counter()
            tm["metrics_s"] += t3 - t2
            if setting_logs:
                for j, i in enumerate(idx):
                    st = tenths[i]
                    if st[7] != min(st[5], st[6]):          # the smaller sw_th_thresh: overwritten by the larger one
                        continue
                    s = he.setting_floats(st)
                    name = he.log_file_name(int(h), *s[:7], s[8])
                    with open(os.path.join(log_file_folder, name), "w") as f:
                        f.write(he.log_text(int(h), s, image_paths, per_page[j], averages[i]))
                tm["logs_s"] += time.perf_counter() - t3
    t4 = time.perf_counter()
    write_csv(results, heights, tenths, averages)
    tm["csv_s"] = time.perf_counter() - t4
    tm["total_s"] = time.perf_counter() - t_start
    return heights, tenths, averages


def write_csv(path, heights, tenths, averages):
    with open(path, "w") as f:
        f.write(",".join(("fixed_height",) + he.FIELDS + he.METRICS) + "\n")
        for h, st, av in zip(heights.tolist(), tenths.tolist(), averages.tolist()):
            f.write(",".join([str(h)] + [repr(k / 10) for k in st] + [repr(x) for x in av]) + "\n")


def read_csv(path):
    """-> list of (fixed_height, setting floats (9), averages (12))"""
    rows = []
    with open(path) as f:
        next(f)
        for line in f:
            v = line.rstrip("\n").split(",")
            rows.append((int(v[0]), tuple(float(x) for x in v[1:10]), tuple(float(x) for x in v[10:22])))
    return rows


def main(argv=None):
    args = build_parser().parse_args(argv)
    image_paths = load_list_file(args.path_to_gt_list)
    os.makedirs(args.log_file_folder, exist_ok=True)
    results = args.results or os.path.join(args.log_file_folder, "grid_results.csv")
    heights, tenths, averages = run_grid(image_paths, args.path_to_pb, args.fixed_heights, args.log_file_folder, results,
                                         setting_logs=not args.no_setting_logs, host_workers=args.num_processes,
                                         gpu_devices=args.gpu_devices)
    f1 = averages[:, he.METRICS.index("F1_BIN")]
    order = sorted(np.flatnonzero(~np.isnan(f1)).tolist(), key=lambda i: -f1[i])[:args.top]
    print(f"{len(tenths)} settings on {len(image_paths)} pages -> {results}")
    print("best settings by average binary F1:")
    for i in order:
        s = he.setting_floats(tenths[i])
        print(f"  F1_BIN {f1[i]:.4f}  fixed_height {int(heights[i])}  " + "  ".join(f"{k} {v}" for k, v in zip(he.FIELDS, s)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
