"""Heading detection evaluation: ``article_separation/image_segmentation/net_post_processing/heading_evaluation.py``.

One setting (this module's command line) runs ``HeadingNetPostProcessor`` over a ground-truth (GT) list like the reference,
writes ``<page>.xml.xml`` and scores the region types of those files against the GT region types: recall, precision and
F1 as binary, micro, macro and weighted (sklearn's ``*_score(..., zero_division=0)``, restated on the four counts), per
page and averaged, in the reference's log file.

Many settings (``heading_evaluation_grid_search``) share the measurements: the stroke-width distance transform and the
per-line stroke width / text height run once per page, the net and the per-line box sums once per (page, fixed height);
``asep_heading_grid_eval`` then applies the fusion rule of every setting to every line of every page on the GPU and
returns the counts.
"""
import argparse
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np

from . import _lib
from .heading_net_post_processor import HEADING, _scale_to_new_interval, line_boxes
from .path_util import get_page_path, load_list_file

FIELDS = ("threshold", "net_weight", "stroke_width_weight", "text_height_weight", "net_thresh", "stroke_width_thresh",
          "text_height_thresh", "sw_th_thresh", "text_line_percentage")
# per-page values and averages in this order: recall, precision, F1, each binary / micro / macro / weighted
METRICS = ("R_BIN", "R_MIC", "R_MAC", "R_WEI", "P_BIN", "P_MIC", "P_MAC", "P_WEI", "F1_BIN", "F1_MIC", "F1_MAC", "F1_WEI")
FIXED_HEIGHTS = tuple(range(600, 1300, 100))


# ---- heading_evaluation.py:20-67 ---------------------------------------------------------------------------------
def get_heading_regions(page_object):
    """:20-29: the text regions of type heading."""
    return [text_region for text_region in page_object.get_text_regions() if text_region.region_type == HEADING]


def get_heading_text_lines(heading_regions):
    """:32-43: all text lines of the regions, as one list."""
    text_lines = []
    for heading_region in heading_regions:
        text_lines.extend(heading_region.text_lines)
    return text_lines


def get_heading_text_line_by_custom_type(heading_regions):
    """:46-67: the text lines of the regions that carry the heading semantic type."""
    text_lines = []
    for heading_region in heading_regions:
        for text_line in heading_region.text_lines:
            try:
                if text_line.custom["structure"]["semantic_type"] == HEADING:
                    text_lines.append(text_line)
            except KeyError:
                continue
    return text_lines


# ---- confidences of one page (apply_heading_values' normalisation) ----------------------------------------------
def heading_confidences(values, text_lines):
    """The three per-line measurement dicts (``collect_boxes`` / ``line_values``) -> (sw_conf, th_conf, net_conf) float64
    arrays in the order of ``text_lines`` and use_swt, with exactly apply_heading_values' steps: Counter.most_common
    mode (first seen wins a tie), differences to the mode, scale_to_new_interval (the data itself when max == min)."""
    stroke_width_dict, height_dict, net_prob_dict = (dict(v) for v in values)
    n = len(text_lines)
    sw, th, net = np.zeros(n), np.zeros(n), np.zeros(n)
    stroke_width_list = list(stroke_width_dict.values())
    use_swt = len(stroke_width_list) > 0
    if use_swt:
        stroke_width_mode = Counter(stroke_width_list).most_common(1)[0][0]
        height_mode = Counter(list(height_dict.values())).most_common(1)[0][0]
        for text_line in text_lines:
            stroke_width_dict[text_line.id] = stroke_width_dict[text_line.id] - stroke_width_mode
            height_dict[text_line.id] = height_dict[text_line.id] - height_mode
        stroke_width_list = list(stroke_width_dict.values())
        stroke_width_min, stroke_width_max = np.min(stroke_width_list), np.max(stroke_width_list)
        height_list = list(height_dict.values())
        height_min, height_max = np.min(height_list), np.max(height_list)
    for i, text_line in enumerate(text_lines):
        net[i] = net_prob_dict[text_line.id]
        if use_swt:
            sw[i] = _scale_to_new_interval(stroke_width_dict[text_line.id], old_min=stroke_width_min, old_max=stroke_width_max)
            th[i] = _scale_to_new_interval(height_dict[text_line.id], old_min=height_min, old_max=height_max)
    return sw, th, net, use_swt


class PageRegions:
    """What the scoring needs of a GT page: its text lines (ids, boxes, outlines), per region the indices of its lines
    (direct TextLine children, as the region rule sees them), the GT label per region and the lines that already carry
    the heading tag (they stay headings in the hypothesis whatever the fusion rule says)."""

    def __init__(self, page):
        self.text_lines = page.get_textlines()
        index = {id(tl.node): i for i, tl in enumerate(self.text_lines)}
        regions = page.get_text_regions()
        self.region_lines = [[index[id(tl.node)] for tl in r.text_lines] for r in regions]
        self.gt = np.array([r.region_type == HEADING for r in regions], dtype=bool)
        self.tagged = np.array([tl.get_semantic_type() == HEADING for tl in self.text_lines], dtype=bool)
        self.ids, self.boxes, self.has = line_boxes(self.text_lines)


def read_gt_page(page_path):
    from .page_xml import Page
    if not os.path.exists(page_path):
        raise FileNotFoundError(f"ground truth PAGE-XML {page_path} does not exist")
    return PageRegions(Page(page_path))


# ---- the grid of heading_evaluation_grid_search.py ---------------------------------------------------------------
def grid_outer(fixed_heights=FIXED_HEIGHTS):
    """heading_evaluation_grid_search.py:93-106: the argument tuples of run_grid_search, in submission order."""
    return [(f, t / 10, nw, nt, swt, tht, tlp) for f in fixed_heights for t in range(4, 10, 1) for nw in range(0, 11, 1)
            for nt in range(8, 11, 1) for swt in range(8, 11, 1) for tht in range(8, 11, 1) for tlp in range(8, 11, 1)]


def grid_inner(fixed_height, threshold, net_weight, net_thresh, stroke_width_thresh, text_height_thresh, text_line_percentage):
    """:11-70: the settings one call of run_grid_search evaluates, as the floats its command line passes:
    (fixed_height, threshold, net_weight, stroke_width_weight, text_height_weight, net_thresh, stroke_width_thresh,
    text_height_thresh, sw_th_thresh, text_line_percentage)."""
    out = []
    ub = min(stroke_width_thresh, text_height_thresh)
    for sw_th_thresh in range(ub - 1, ub + 1, 1):
        for stroke_width_weight in range(0, 10 - net_weight + 1, 1):
            out.append((fixed_height, threshold, net_weight / 10, stroke_width_weight / 10,
                        (10 - net_weight - stroke_width_weight) / 10, net_thresh / 10, stroke_width_thresh / 10,
                        text_height_thresh / 10, sw_th_thresh / 10, text_line_percentage / 10))
    return out


def grid_settings(fixed_heights=FIXED_HEIGHTS):
    """Every setting of the grid in the reference's order -> (fixed heights int64 [N], tenths int32 [N, 9] in FIELDS order).
    The floats are tenths / 10 (``setting_floats``), exactly what the reference's command lines carry."""
    heights, tenths = [], []
    for f, t, nw, nt, swt, tht, tlp in grid_outer(fixed_heights):
        ub = min(swt, tht)
        for swth in range(ub - 1, ub + 1):
            for sww in range(0, 10 - nw + 1):
                heights.append(f)
                tenths.append((round(t * 10), nw, sww, 10 - nw - sww, nt, swt, tht, swth, tlp))
    return np.array(heights, np.int64), np.array(tenths, np.int32).reshape(-1, len(FIELDS))


def setting_floats(tenths):
    """One row of tenths -> the setting's floats (k / 10 as Python divides)."""
    return tuple(int(k) / 10 for k in tenths)


# ---- scoring ---------------------------------------------------------------------------------------------------
def counts_from_labels(is_heading_gt, is_heading_hyp):
    """label lists -> int64 [4] TP, FP, FN, TN"""
    g, h = np.asarray(is_heading_gt, bool), np.asarray(is_heading_hyp, bool)
    if g.shape != h.shape:
        raise ValueError(f"{len(g)} GT labels against {len(h)} hypothesis labels")
    return np.array([np.sum(g & h), np.sum(~g & h), np.sum(g & ~h), np.sum(~g & ~h)], np.int64)


def _div(num, den):
    """sklearn's _prf_divide with zero_division=0: float64 num / den, 0 where den == 0"""
    den = np.asarray(den, np.float64)
    zero = den == 0
    return np.where(zero, 0.0, np.asarray(num, np.float64) / np.where(zero, 1.0, den))


def page_metrics(counts):
    """counts [..., 4] (TP, FP, FN, TN of one page's region labels) -> float64 [..., 12] in METRICS order, bit-equal to
    recall_score / precision_score / f1_score(y_true, y_pred, average=binary|micro|macro|weighted, zero_division=0) on
    the label lists: labels are those present in either list; macro / weighted are nan for a page without regions."""
    c = np.asarray(counts, np.int64)
    tp, fp, fn, tn = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    n = tp + fp + fn + tn
    # per label (False, True): tp, predicted, true
    lab = {False: (tn, tn + fn, tn + fp), True: (tp, tp + fp, tp + fn)}
    present = {False: (tn + fp + fn) > 0, True: (tp + fp + fn) > 0}
    per = {}
    for k, (t_, p_, r_) in lab.items():
        # f: (1 + beta^2) * tp / (beta^2 * true + pred), beta = 1, on float64 sums
        per[k] = (_div(t_, r_), _div(t_, p_), _div(2.0 * t_.astype(np.float64), 1.0 * r_.astype(np.float64) + p_.astype(np.float64)))
    micro_r = _div(tp + tn, n)
    micro_f = _div(2.0 * (tp + tn).astype(np.float64), 1.0 * n.astype(np.float64) + n.astype(np.float64))
    out = np.empty(c.shape[:-1] + (12,))
    n_present = present[False].astype(np.int64) + present[True]
    w_f, w_t = lab[False][2].astype(np.float64), lab[True][2].astype(np.float64)
    for m in range(3):                                  # recall, precision, f1
        vf, vt = per[False][m], per[True][m]
        both = (vf + vt) / 2
        macro = np.where(n_present == 2, both, np.where(present[True], vt, vf))
        weighted = (vf * w_f + vt * w_t) / np.where(n == 0, 1.0, w_f + w_t)
        out[..., 4 * m + 0] = vt
        out[..., 4 * m + 1] = micro_f if m == 2 else micro_r
        out[..., 4 * m + 2] = np.where(n == 0, np.nan, macro)
        out[..., 4 * m + 3] = np.where(n == 0, np.nan, weighted)
    return out


def average_metrics(per_page):
    """[..., P, 12] -> [..., 12]: np.mean over the pages in list order (a page axis of length 0 gives nan)"""
    a = np.ascontiguousarray(np.moveaxis(np.asarray(per_page, np.float64), -1, -2))
    if a.shape[-1] == 0:
        return np.full(a.shape[:-1], np.nan)
    return np.mean(a, axis=-1)


# ---- log file (heading_evaluation.py:150-243) ---------------------------------------------------------------------
def log_file_name(fixed_height, threshold, net_weight, stroke_width_weight, text_height_weight, net_thresh,
                  stroke_width_thresh, text_height_thresh, text_line_percentage):
    """:150-153 (sw_th_thresh is not part of the name)"""
    return f"{fixed_height:04}_{threshold*100:03.0f}_{net_weight*100:03.0f}_" \
           f"{stroke_width_weight*100:03.0f}_{text_height_weight*100:03.0f}_" \
           f"{net_thresh*100:03.0f}_{stroke_width_thresh*100:03.0f}_{text_height_thresh*100:03.0f}_" \
           f"{text_line_percentage*100:03.0f}.log"


def log_text(fixed_height, setting, image_paths, per_page, averages):
    """The log file's text: ``setting`` = the nine floats in FIELDS order, ``per_page`` [P, 12], ``averages`` [12]."""
    (threshold, net_weight, stroke_width_weight, text_height_weight, net_thresh, stroke_width_thresh, text_height_thresh,
     sw_th_thresh, text_line_percentage) = setting
    parts = [f"fixed_height: {fixed_height}\n"
             f"is_heading_threshold: {threshold}\n"
             f"net_weight: {net_weight}\n"
             f"stroke_width_weight: {stroke_width_weight}\n"
             f"text_height_weight: {text_height_weight}\n"
             f"net_thresh: {net_thresh}\n"
             f"stroke_width_thresh: {stroke_width_thresh}\n"
             f"text_height_thresh: {text_height_thresh}\n"
             f"sw_th_thresh: {sw_th_thresh}\n"
             f"text_line_percentage: {text_line_percentage}\n"]
    for image_path, v in zip(image_paths, per_page):
        v = [float(x) for x in v]
        parts.append(f"\nImage path: {image_path}\n")
        for row in range(3):
            end = "\n" if row < 2 else ""
            parts.append("".join(f"\t{METRICS[4 * row + j]:>6}: {v[4 * row + j]:.4f}" for j in range(4)) + end)
    a = [float(x) for x in averages]
    parts.append("\n\nAverage Recall (BIN) \t Average Precision (BIN) \t Average F1 (BIN)\n")
    parts.append(f"{a[0]:.4f}, {a[4]:.4f}, {a[8]:.4f}\n\n")
    parts.append("\nAverage Recall (MIC) \t Average Precision (MIC) \t Average F1 (MIC)\n")
    parts.append(f"{a[1]:.4f}, {a[5]:.4f}, {a[9]:.4f}\n\n")
    parts.append("\nAverage Recall (MAC) \t Average Precision (MAC) \t Average F1 (MAC)\n")
    parts.append(f"{a[2]:.4f}, {a[6]:.4f}, {a[10]:.4f}\n\n")
    parts.append("\nAverage Recall (WEI) \t Average Precision (WEI) \t Average F1 (WEI)\n")
    parts.append(f"{a[3]:.4f}, {a[7]:.4f}, {a[11]:.4f}")
    return "".join(parts)


# ---- the grid kernel ----------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class GridPages:
    """The pages of one grid call in the layout of asep_heading_grid_eval: per page the confidences of its lines
    (``heading_confidences``), use_swt, the regions' line indices, the GT labels and the tagged lines."""

    def __init__(self, pages):
        """pages: iterable of (sw_conf, th_conf, net_conf, use_swt, region_lines, gt, tagged or None)"""
        pages = list(pages)
        self.n_pages = len(pages)
        nl = [len(p[0]) for p in pages]
        nr = [len(p[4]) for p in pages]
        self.line_off = np.zeros(self.n_pages + 1, np.int32)
        self.line_off[1:] = np.cumsum(nl)
        self.reg_off = np.zeros(self.n_pages + 1, np.int32)
        self.reg_off[1:] = np.cumsum(nr)
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0), dtype=dt)  # noqa: E731
        self.sw = cat([np.asarray(p[0], np.float64) for p in pages], np.float64)
        self.th = cat([np.asarray(p[1], np.float64) for p in pages], np.float64)
        self.net = cat([np.asarray(p[2], np.float64) for p in pages], np.float64)
        self.use_swt = np.array([bool(p[3]) for p in pages], np.uint8)
        regions = [list(r) for p in pages for r in p[4]]
        self.reg_line_off = np.zeros(len(regions) + 1, np.int32)
        self.reg_line_off[1:] = np.cumsum([len(r) for r in regions])
        self.reg_lines = np.array([i for r in regions for i in r], np.int32)
        self.gt = cat([np.asarray(p[5], bool) for p in pages], np.uint8)
        self.tagged = cat([np.zeros(n, bool) if p[6] is None else np.asarray(p[6], bool) for n, p in zip(nl, pages)], np.uint8)

    def with_net(self, net):
        """the same pages with other net confidences (another fixed height)"""
        other = object.__new__(GridPages)
        other.__dict__.update(self.__dict__)
        other.net = np.ascontiguousarray(net, np.float64)
        return other


def grid_eval(gp, tenths, device=0):
    """asep_heading_grid_eval: counts int32 [n_settings, n_pages, 4] (TP, FP, FN, TN) of every setting on every page"""
    from .textblock import _handle
    lib, h = _handle(device)
    tenths = np.ascontiguousarray(tenths, np.int32).reshape(-1, len(FIELDS))
    out = np.zeros((len(tenths), gp.n_pages, 4), np.int32)
    _lib.check(lib.asep_heading_grid_eval(h, gp.n_pages, _ptr(gp.line_off), _ptr(gp.sw), _ptr(gp.th), _ptr(gp.net),
                                          _ptr(gp.tagged), _ptr(gp.use_swt), _ptr(gp.reg_off), _ptr(gp.reg_line_off),
                                          _ptr(gp.reg_lines), _ptr(gp.gt), len(tenths), _ptr(tenths), _ptr(out)),
               "asep_heading_grid_eval")
    return out


def last_kernel_us():
    return _lib.load_library().asep_heading_grid_last_kernel_us()


# ---- measure once, score many ------------------------------------------------------------------------------------
def measure_pages(image_paths, path_to_pb, fixed_heights, gpu_devices='0', host_workers=0, timings=None):
    """The measurements of every page for every fixed height through the heading post-processor's device stages, shared by
    all settings: one upload per page, the net and the per-line box sums once per (page, height) on that upload, the distance
    transform and the per-line stroke width / text height once per page.  -> (GT pages (PageRegions), [(sw dict, th dict)]
    per page, {height: [net dict per page]}).

    ``timings`` (a dict) is filled with the wall time of each stage: ``net_s`` {height: s} (resize + net, the lane's stream
    synchronised after each height), ``dt_s`` (gray + distance transform), ``line_features_s`` (stroke width / text height
    and the first height's box sums), ``box_sums_s`` (the other heights' box sums), ``decode_wait_s`` (waiting for decoded
    images, ``first_page_s`` of it before the first one); the stages are synchronised one by one when it is given."""
    import time
    import torch
    from .heading_net_post_processor import HeadingNetPostProcessor
    from .host_pipeline import DecodePool, pin_callbacks
    heights = [int(h) for h in fixed_heights]
    if not heights:
        raise ValueError("no fixed heights")
    proc = HeadingNetPostProcessor(list(image_paths), path_to_pb, heights[0], None)
    proc.gpu_devices = gpu_devices
    proc.SWT.device = proc.device
    gts = [read_gt_page(get_page_path(p)) for p in proc.image_paths]
    swth = [None] * len(gts)
    nets = {h: [None] * len(gts) for h in heights}
    order = {}
    tm = {} if timings is None else timings
    tm.update(net_s={h: 0.0 for h in heights}, dt_s=0.0, line_features_s=0.0, box_sums_s=0.0)

    def stage(lane, key, h=None, t0=None):
        if timings is None:
            return None
        with proc._on_lane(lane) as (_, _, _, stream, _):
            stream.synchronize()
        now = time.perf_counter()
        if t0 is not None:
            if h is None:
                tm[key] += now - t0
            else:
                tm[key][h] += now - t0
        return now

    def enqueue(images, lane):
        t0 = stage(lane, None)
        first = proc._enqueue_net(images, lane)
        per_page = [{heights[0]: t} for t in first]
        t0 = stage(lane, "net_s", heights[0], t0)
        for h in heights[1:]:
            proc.fixed_height = h
            for d, t in zip(per_page, proc._enqueue_net(images, lane, reuse=first)):
                d[h] = t
            t0 = stage(lane, "net_s", h, t0)
        proc.fixed_height = heights[0]
        proc._enqueue_swt(first, lane)                  # the "done" event of a page follows every kernel queued for it
        stage(lane, "dt_s", None, t0)
        for d in per_page:
            for h in heights[1:]:
                d[h]["done"] = d[heights[0]]["done"]
            d["uploaded"] = d[heights[0]]["uploaded"]
        return per_page

    def finish(image_path, per_height):
        k = order.setdefault("next", 0)
        order["next"] = k + 1
        g = gts[k]
        for h in heights:
            t0 = time.perf_counter()
            sw, ht, net = proc.collect_boxes(per_height[h], g.ids, g.boxes, g.has)
            tm["line_features_s" if h == heights[0] else "box_sums_s"] += time.perf_counter() - t0
            if h == heights[0]:
                swth[k] = (sw, ht)
            nets[h][k] = net

    pipelined = host_workers > 1
    reg, unreg = pin_callbacks(proc.device) if pipelined else (None, None)
    group = proc.PAGE_GROUP if pipelined else 1
    decode = DecodePool(proc.image_paths, host_workers if pipelined else 0, register=reg, unregister=unreg, hold=group + 1)
    proc._run_groups(decode, len(proc.image_paths), group, proc.PAGE_LANES if pipelined else 1, enqueue, finish)
    tm["decode_wait_s"] = proc.wait_seconds
    tm["first_page_s"] = proc.first_page_seconds or 0.0
    return gts, swth, nets


def page_inputs(gts, swth, net_dicts):
    """GridPages of one fixed height from the measurements"""
    pages = []
    for g, (sw, ht), net in zip(gts, swth, net_dicts):
        s, t, n, use = heading_confidences((sw, ht, net), g.text_lines)
        pages.append((s, t, n, use, g.region_lines, g.gt, g.tagged))
    return GridPages(pages)


# ---- command line: one setting ------------------------------------------------------------------------------------
NUMERIC_FLAGS = ("fixed_height", "threshold", "net_weight", "stroke_width_weight", "text_height_weight", "net_thresh",
                 "stroke_width_thresh", "text_height_thresh", "sw_th_thresh", "text_line_percentage")


def build_parser():
    """heading_evaluation.py:71-103"""
    parser = argparse.ArgumentParser()
    parser.add_argument('--path_to_gt_list', type=str, required=True, help='Path to the list of GT PAGE XML file paths.')
    parser.add_argument('--path_to_pb', type=str, required=True,
                        help="Path to the TensorFlow pb graph for creating the separator information")
    parser.add_argument('--fixed_height', type=int, required=False,
                        help="If parameter is given, the images will be scaled to this height by keeping the aspect ratio")
    parser.add_argument('--threshold', type=float, required=False,
                        help="Threshold value that decides based on the feature values if a text line is a heading or not.")
    parser.add_argument('--net_weight', type=float, required=False, help="Weight the net output feature.")
    parser.add_argument('--stroke_width_weight', type=float, required=False, help="Weight the stroke width feature.")
    parser.add_argument('--text_height_weight', type=float, required=False, help="Weight the text line height feature.")
    parser.add_argument('--gpu_devices', type=str, required=False, default='0',
                        help='Which GPU device to use (the first of a comma-separated list; "" means device 0: there is no CPU path).')
    parser.add_argument("--net_thresh", type=float, required=False,
                        help="If the net confidence is greater than or equal to this value the text line is considered a heading.")
    parser.add_argument("--stroke_width_thresh", type=float, required=False,
                        help="If the stroke width confidence is greater than or equal to his value the text line is considered a heading.")
    parser.add_argument("--text_height_thresh", type=float, required=False,
                        help="If the text height confidence is greater than or equal to this value the text line is considered a heading.")
    parser.add_argument("--sw_th_thresh", type=float, required=False,
                        help="If the average of stroke width and text height confidence is greater than or equal to this value the "
                             "text line is considered a heading.")
    parser.add_argument("--text_line_percentage", type=float, required=False,
                        help="Declare a region as heading if text_line_percentage percent text lines are considered as headings.")
    parser.add_argument('--log_file_folder', type=str, required=False, help='Where to store the log files.')
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    missing = [f"--{k}" for k in NUMERIC_FLAGS + ("log_file_folder",) if getattr(args, k) is None]
    if missing:
        parser.error("the evaluation needs every setting and the log folder; missing: " + ", ".join(missing))
    return args


def hypothesis_labels(image_paths):
    """(GT labels, hypothesis labels) per page from ``<page>.xml`` and the ``<page>.xml.xml`` written next to it"""
    from .page_xml import Page
    out = []
    for image_path in image_paths:
        xml_path = get_page_path(image_path)
        gt = [tr.region_type == HEADING for tr in Page(xml_path).get_text_regions()]
        hyp = [tr.region_type == HEADING for tr in Page(xml_path + ".xml").get_text_regions()]
        if len(gt) != len(hyp):
            raise ValueError(f"{xml_path}: the GT page has {len(gt)} text regions, the hypothesis {xml_path}.xml has {len(hyp)}")
        out.append((gt, hyp))
    return out


def main(argv=None):
    args = parse_args(argv)
    from .heading_net_post_processor import HeadingNetPostProcessor
    image_paths = load_list_file(args.path_to_gt_list)
    weight_dict = {"net": args.net_weight, "stroke_width": args.stroke_width_weight, "text_height": args.text_height_weight}
    thresh_dict = {"net_thresh": args.net_thresh, "stroke_width_thresh": args.stroke_width_thresh,
                   "text_height_thresh": args.text_height_thresh, "sw_th_thresh": args.sw_th_thresh}
    proc = HeadingNetPostProcessor(image_paths, args.path_to_pb, args.fixed_height, None, weight_dict=weight_dict,
                                   threshold=args.threshold, thresh_dict=thresh_dict, text_line_percentage=args.text_line_percentage)
    proc.run(args.gpu_devices)
    labels = hypothesis_labels(image_paths)
    per_page = page_metrics(np.array([counts_from_labels(g, h) for g, h in labels], np.int64).reshape(-1, 4))
    averages = average_metrics(per_page)
    setting = tuple(getattr(args, k) for k in FIELDS)
    name = os.path.join(args.log_file_folder, log_file_name(args.fixed_height, args.threshold, args.net_weight,
                                                            args.stroke_width_weight, args.text_height_weight, args.net_thresh,
                                                            args.stroke_width_thresh, args.text_height_thresh,
                                                            args.text_line_percentage))
    with open(name, "w") as f:
        f.write(log_text(args.fixed_height, setting, image_paths, per_page, averages))
    return 0


if __name__ == '__main__':
    sys.exit(main())
