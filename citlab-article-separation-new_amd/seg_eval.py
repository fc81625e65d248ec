"""Evaluation of the segmentation nets on the device: mirror of ``article_separation/plot_net_output.py``.

``plot_net_output`` runs a pixel labeller over an image list and prints, per page, the share of values where the net is not
sure, the arg-max share of every class and the pixel accuracy against the ground truth channel images
``<dir>/C<n>/<name>_GT<i>.png``, and writes the per-class masks ``<name>_OUT<cl><ext>``.  Here the probabilities stay where
``asep_aru_forward_batch_dev2`` left them: one scoring call per group of pages (``asep_seg_eval_pages_dev``) brings back
integer counters, and masks only when a save folder is given.  Shares and accuracies are divisions of those integers on the
host, in the reference's order.

Kept from the reference on purpose:
  * ``mask_threshold`` switches thresholding ON; the threshold itself is the constant 0.6 whatever the flag's value (:201-202);
  * the class shares are divided by the ORIGINAL image's ``width * height`` (:220), not by the net output's size;
  * with ``plot_with_img`` the scan's channel order is reversed once per class (:244), so odd classes are drawn over the scan
    with red and blue swapped, and with ``plot_with_gt`` the ground truth blends accumulate on that scan (:249 works in place).
Additions (marked as such in the output): precision, recall, F1 and IoU per class from the same pass.
Not served: ground truth of another size than the net output (the reference resizes it with OpenCV's bilinear default, :213-214,
which this build cannot pin), and the on-screen plots of ``show_plot`` (matplotlib).
"""
import ctypes as C
import os

import numpy as np

from . import _lib

MAX_CLASSES = 8            # ASEP_SEG_EVAL_MAX_CLASSES
SLOTS = 48                 # ASEP_SEG_EVAL_SLOTS and the offsets of a page's counter block (include/asep_hip.h)
UNSURE, PIXELS, HAS_GT, CLASS, EQUAL, TP, FP, FN = 0, 1, 2, 8, 16, 24, 32, 40
MASK_COLOR = (255, 50, 50)  # plot_image_with_net_output, :93 (alpha 0.5 is the kernel's)
REF_THRESHOLD = 0.6         # :202


class GroundTruthSizeError(ValueError):
    pass


# ---- names -------------------------------------------------------------------------------------------------------------
def gt_paths(path_to_img, n_classes):
    """:208-210: the ground truth channel images of a page"""
    dirname = os.path.dirname(path_to_img)
    img_name = os.path.splitext(os.path.basename(path_to_img))[0]
    return [os.path.join(dirname, "C" + str(n_classes), img_name + "_GT" + str(i) + ".png") for i in range(n_classes)]


def out_path(save_folder, path_to_img, cl):
    """:252-253: <save_folder>/<name>_OUT<cl><ext>"""
    img_name, ext = os.path.splitext(os.path.basename(path_to_img))
    return os.path.join(save_folder, img_name + "_OUT" + str(cl) + ext)


def tool_scaling_factor(img_height, rescale, fixed_height):
    """:176-187 -> (the reference's scaling_factor, the factor the scan is resized with: only 0.1 < factor < 1 resizes)"""
    scaling_factor = None
    if fixed_height and rescale and rescale != 1:
        scaling_factor = rescale * fixed_height / img_height
    elif fixed_height:
        scaling_factor = fixed_height / img_height
    elif rescale:
        scaling_factor = rescale
    resize = scaling_factor if scaling_factor is not None and 0.1 < scaling_factor < 1.0 else 1.0
    return scaling_factor, resize


# ---- host figures from a page's counter block -----------------------------------------------------------------------------
def page_figures(counters, n_classes, full_count):
    """one page's counter block -> dict: ``unsure`` (:198-199), ``class_shares`` (:227-228, over ``full_count`` = the original
    image's width * height), ``accuracy`` (:230-241,279: per class equal / (H * W), summed, divided by C; 0.0 without ground
    truth) and, as additions, ``precision`` / ``recall`` / ``f1`` / ``iou`` per class (None where a denominator is 0)"""
    cnt = [int(v) for v in counters]
    npix = cnt[PIXELS]
    fig = {"unsure": cnt[UNSURE] / (npix * n_classes),
           "class_shares": [cnt[CLASS + c] / full_count for c in range(n_classes)],
           "has_gt": bool(cnt[HAS_GT])}
    accuracy = 0
    if fig["has_gt"]:
        for cl in range(n_classes):
            accuracy += cnt[EQUAL + cl] / npix
    accuracy /= n_classes
    fig["accuracy"] = accuracy

    def ratio(a, b):
        return a / b if b else None
    tp, fp, fn = ([cnt[k + c] for c in range(n_classes)] for k in (TP, FP, FN))
    fig["tp"], fig["fp"], fig["fn"] = tp, fp, fn
    fig["precision"] = [ratio(tp[c], tp[c] + fp[c]) for c in range(n_classes)]
    fig["recall"] = [ratio(tp[c], tp[c] + fn[c]) for c in range(n_classes)]
    fig["f1"] = [ratio(2 * tp[c], 2 * tp[c] + fp[c] + fn[c]) for c in range(n_classes)]
    fig["iou"] = [ratio(tp[c], tp[c] + fp[c] + fn[c]) for c in range(n_classes)]
    return fig


def page_lines(fig):
    """the reference's printed lines of one page (:198-199,227-228,281-282), with the additions between them"""
    lines = ["Percentage of Pixels where the net is not 100% sure:  " + str(fig["unsure"])]
    for i, share in enumerate(fig["class_shares"]):
        lines.append(f"Percentage of pixels in class_{i}: {share}")
    if fig["has_gt"]:
        for i in range(len(fig["class_shares"])):
            lines.append(f"Addition (not in the reference) class_{i}: precision = {fig['precision'][i]} recall = {fig['recall'][i]} "
                         f"F1 = {fig['f1'][i]} IoU = {fig['iou'][i]} (tp {fig['tp'][i]} fp {fig['fp'][i]} fn {fig['fn'][i]})")
    lines.append("Accuracy =  " + str(fig["accuracy"]))
    lines.append("+++++++++++++++++++++++")
    return lines


def overall_line(accuracies):
    """:283"""
    return "Overall Accuracy =  " + str(sum(accuracies) / len(accuracies))


# ---- the engine ----------------------------------------------------------------------------------------------------------
def check_classes(n_classes):
    if n_classes < 1:
        raise ValueError(f"{n_classes} classes: a net output has at least one class")
    if n_classes > MAX_CLASSES:
        raise ValueError(f"{n_classes} classes: the scoring kernel is built for 1 .. {MAX_CLASSES} classes")


class SegEvaluator:
    """One ``asep_seg_eval`` handle of a device.  Tensors are torch tensors on that device; calls go to torch's current stream."""

    def __init__(self, device=0):
        self.device = int(device)
        self.lib = _lib.init_device(self.device)
        self.handle = self.lib.asep_seg_eval_create()
        if not self.handle:
            raise _lib.AsepError("asep_seg_eval_create failed: " + _lib.last_error())
        self.d2h_bytes = 0            # what this object copied to the host: counter blocks, and masks when they were asked for

    def close(self):
        if self.handle:
            self.lib.asep_seg_eval_free(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)

    def score_pages(self, d_probs, d_gts=None, want_masks=False, mask_threshold=False):
        """``d_probs``: float32 tensors [H,W,C] of one C; ``d_gts``: per page None or a uint8 tensor [C,H,W] (or a list of C
        [H,W] tensors) -> (counters uint64 [n, SLOTS], masks: per page a uint8 tensor [C,H,W] on the device, or None)"""
        import torch
        n = len(d_probs)
        if n == 0:
            return np.zeros((0, SLOTS), np.uint64), ([] if want_masks else None)
        ncls = int(d_probs[0].shape[2])
        check_classes(ncls)
        keep = []
        for t in d_probs:
            if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or int(t.shape[2]) != ncls or not t.is_contiguous():
                raise ValueError("score_pages takes contiguous float32 [H,W,C] tensors of one C on the device")
        Ptr, Ints = C.c_void_p * n, C.c_int32 * n
        gt_arr = None
        if d_gts is not None and any(g is not None for g in d_gts):
            gt_arr = (C.c_void_p * (n * ncls))()
            for b, g in enumerate(d_gts):
                if g is None:
                    continue
                planes = [g[c] for c in range(ncls)] if isinstance(g, torch.Tensor) else list(g)
                if len(planes) != ncls:
                    raise ValueError(f"page {b}: {len(planes)} ground truth planes for {ncls} classes")
                for c, pl in enumerate(planes):
                    if tuple(pl.shape) != tuple(d_probs[b].shape[:2]):
                        raise GroundTruthSizeError(
                            f"page {b}: ground truth plane {c} is {tuple(pl.shape)}, the net output {tuple(d_probs[b].shape[:2])}: "
                            "the reference resizes it with OpenCV's bilinear default, which this build cannot reproduce byte for "
                            "byte; give ground truth of the net output's size")
                    if pl.dtype != torch.uint8 or not pl.is_cuda:
                        raise ValueError("ground truth planes are uint8 tensors on the device")
                    pl = pl.contiguous()
                    keep.append(pl)
                    gt_arr[b * ncls + c] = pl.data_ptr()
        masks = None
        if want_masks:
            masks = [torch.empty((ncls, t.shape[0], t.shape[1]), dtype=torch.uint8, device=t.device) for t in d_probs]
        counters = np.zeros((n, SLOTS), np.uint64)
        rc = self.lib.asep_seg_eval_pages_dev(
            self.handle, n, Ptr(*[t.data_ptr() for t in d_probs]), gt_arr, Ptr(*[m.data_ptr() for m in masks]) if masks else None,
            Ints(*[t.shape[0] for t in d_probs]), Ints(*[t.shape[1] for t in d_probs]), ncls, 1 if mask_threshold else 0,
            counters.ctypes.data, self._stream())
        _lib.check(rc, "asep_seg_eval_pages_dev")
        self.d2h_bytes += counters.nbytes
        return counters, masks

    def blend(self, d_scan, d_mask, color=MASK_COLOR, out=None):
        """apply_mask(scan, mask, color, 0.5) of :57-70 -> uint8 [H,W,3] on the device (``out`` may be ``d_scan``)"""
        import torch
        if d_scan.dtype != torch.uint8 or d_scan.dim() != 3 or d_scan.shape[2] != 3 or not d_scan.is_contiguous():
            raise ValueError("blend takes a contiguous uint8 [H,W,3] scan on the device")
        if d_mask.dtype != torch.uint8 or tuple(d_mask.shape) != tuple(d_scan.shape[:2]):
            raise ValueError(f"blend: the mask is {tuple(d_mask.shape)}, the scan {tuple(d_scan.shape[:2])}")
        d_mask = d_mask.contiguous()
        if out is None:
            out = torch.empty_like(d_scan)
        _lib.check(self.lib.asep_seg_eval_blend_dev(self.handle, d_scan.data_ptr(), d_mask.data_ptr(), int(d_scan.shape[0]),
                                                    int(d_scan.shape[1]), int(color[0]), int(color[1]), int(color[2]), out.data_ptr(),
                                                    self._stream()), "asep_seg_eval_blend_dev")
        return out

    def to_host(self, d_tensor):
        out = d_tensor.cpu().numpy()
        self.d2h_bytes += out.nbytes
        return out

    @property
    def kernel_us(self):
        return float(self.lib.asep_seg_eval_last_kernel_us(self.handle))

    def launches(self):
        """names of the kernels launched since the start of the last scoring call"""
        n = int(self.lib.asep_seg_eval_last_launches(self.handle, None, 0))
        buf = C.create_string_buffer(n + 1)
        self.lib.asep_seg_eval_last_launches(self.handle, buf, n + 1)
        return [s for s in buf.value.decode().split("\n") if s]


# ---- the tool --------------------------------------------------------------------------------------------------------------
def load_ground_truth(path_to_img, n_classes, size):
    """the page's C ground truth images as gray bytes [C,h,w] (:208-212); ``size`` = the net output's (h, w)"""
    from .heading_net_post_processor import bgr_to_gray_u8
    from .image_io import load_image_bgr
    planes = []
    for p in gt_paths(path_to_img, n_classes):
        if not os.path.isfile(p):
            raise IOError(f"No such ground truth image: {p}")
        g = bgr_to_gray_u8(load_image_bgr(p))
        if tuple(g.shape) != tuple(size):
            raise GroundTruthSizeError(
                f"{p} is {g.shape[0]} x {g.shape[1]}, the net output {size[0]} x {size[1]}: the reference resizes the ground truth "
                "with OpenCV's bilinear default (plot_net_output.py:213-214), which this build cannot reproduce byte for byte; "
                "give ground truth of the net output's size")
        planes.append(g)
    return np.ascontiguousarray(np.stack(planes))


def _write_image(path, array):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(array)).save(path)


_said_show_plot = False


def plot_net_output(path_to_pb, path_to_img_lst, save_folder="", gpu_device="0", rescale=None, fixed_height=None,
                    mask_threshold=None, plot_with_gt=False, plot_with_img=False, show_plot=False, calculate_accuracy=True,
                    figsize=(16, 16), ax=None, pages_per_call=1, dtype=None, out=print, evaluator=None):
    """:131-283 with the reference's arguments; ``pages_per_call`` pages share one forward and one scoring call, ``dtype``
    overrides the model's arithmetic (f32 | bf16 | f32s).  -> {"pages": [figures per page], "overall": float or None}"""
    global _said_show_plot
    import torch
    from . import image_ops
    from .heading_net_post_processor import bgr_to_gray_u8
    from .image_io import load_image_bgr
    from .net_post_processing_helper import COMPUTE_DTYPES, _device_of, load_graph
    from .path_util import load_list_file

    if show_plot and not _said_show_plot:
        out("show_plot: plots on the screen (matplotlib) are not part of this build; everything else runs as asked")
        _said_show_plot = True
    graph = load_graph(path_to_pb)
    if dtype:
        if dtype not in COMPUTE_DTYPES:
            raise ValueError(f"dtype must be one of {sorted(COMPUTE_DTYPES)}, got {dtype!r}")
        if graph.cfg.compute_dtype != dtype:
            graph.close()
            graph.cfg.compute_dtype = dtype
    if graph.cfg.channels != 1:
        raise ValueError(f"the model reads {graph.cfg.channels} image channels: plot_net_output feeds the gray page only (:174,193-194)")
    ncls = graph.cfg.n_classes
    check_classes(ncls)
    need_gt = bool(plot_with_gt or calculate_accuracy)
    paths = [p.rstrip() for p in load_list_file(path_to_img_lst)] if isinstance(path_to_img_lst, str) else list(path_to_img_lst)
    dev = _device_of(gpu_device)
    tdev = torch.device("cuda", dev)
    lib, ws = image_ops._workspace(dev)
    own = evaluator is None
    ev = SegEvaluator(dev) if own else evaluator
    pages, accuracies = [], []
    per_call = max(1, int(pages_per_call or 1))
    try:
        with torch.cuda.device(tdev):
            sp = C.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
            for g0 in range(0, len(paths), per_call):
                group = paths[g0:g0 + per_call]
                tickets = []
                for path in group:
                    img = load_image_bgr(path)
                    if img.ndim == 2:
                        img = np.repeat(img[:, :, None], 3, axis=2)          # (cv2.imread hands out three channels for gray files too)
                    img = np.ascontiguousarray(img)
                    H, W = img.shape[:2]
                    gray = np.ascontiguousarray(bgr_to_gray_u8(img))          # :174 gray first, then the area resize (:185-187)
                    _, sc = tool_scaling_factor(H, rescale, fixed_height)
                    h, w = image_ops.scaled_size(H, W, sc)
                    t = {"path": path, "full_count": W * H, "size": (h, w)}
                    d_gray_u8 = torch.from_numpy(gray).to(tdev)
                    t["d_gray"] = torch.empty((h, w), dtype=torch.float32, device=tdev)
                    _lib.check(lib.asep_prep_scale_gray_dev(ws, d_gray_u8.data_ptr(), H, W, 1, float(sc), None, t["d_gray"].data_ptr(), sp),
                               "asep_prep_scale_gray_dev")
                    if plot_with_img and save_folder:
                        d_bgr = torch.from_numpy(img).to(tdev)
                        t["d_scan"] = torch.empty((h, w, 3), dtype=torch.uint8, device=tdev)
                        d_unused = torch.empty((h, w), dtype=torch.float32, device=tdev)
                        _lib.check(lib.asep_prep_scale_gray_dev(ws, d_bgr.data_ptr(), H, W, 3, float(sc), t["d_scan"].data_ptr(),
                                                                d_unused.data_ptr(), sp), "asep_prep_scale_gray_dev")
                    t["d_out"] = torch.empty((h, w, ncls), dtype=torch.float32, device=tdev)
                    if need_gt:
                        t["d_gt"] = torch.from_numpy(load_ground_truth(path, ncls, (h, w))).to(tdev)
                    tickets.append(t)
                n = len(tickets)
                Ptr, Ints = C.c_void_p * n, C.c_int32 * n
                _lib.check(lib.asep_aru_forward_batch_dev2(
                    graph.handle(dev), n, Ptr(*[t["d_gray"].data_ptr() for t in tickets]), Ints(*[t["size"][0] for t in tickets]),
                    Ints(*[t["size"][1] for t in tickets]), Ptr(*[t["d_out"].data_ptr() for t in tickets]), None, None, 0.0, sp),
                    "asep_aru_forward_batch_dev2")
                counters, masks = ev.score_pages([t["d_out"] for t in tickets], [t.get("d_gt") for t in tickets] if need_gt else None,
                                                 want_masks=bool(save_folder), mask_threshold=bool(mask_threshold))
                for b, t in enumerate(tickets):
                    cnt = counters[b].copy()
                    if not calculate_accuracy:
                        cnt[HAS_GT] = 0                                      # ground truth loaded for the plots only: no accuracy (:240)
                    fig = page_figures(cnt, ncls, t["full_count"])
                    fig["path"] = t["path"]
                    for line in page_lines(fig):
                        out(line)
                    pages.append(fig)
                    accuracies.append(fig["accuracy"])
                    if save_folder:
                        _save_page(ev, t, masks[b], ncls, save_folder, plot_with_gt, plot_with_img)
    finally:
        if own:
            ev.close()
    overall = None
    if accuracies:
        overall = sum(accuracies) / len(accuracies)
        out(overall_line(accuracies))
    return {"pages": pages, "overall": overall}


def _save_page(ev, t, d_masks, ncls, save_folder, plot_with_gt, plot_with_img):
    """:231-253 of one page: per class the mask, with ``plot_with_img`` blended over the scan, with ``plot_with_gt`` the ground
    truth half on the right"""
    import torch
    img = t.get("d_scan")                                         # B, G, R as decoded; reversed once per class like :244
    for cl in range(ncls):
        out_img = d_masks[cl]
        if plot_with_img:
            img = img.flip(-1).contiguous()
            out_img = ev.blend(img, d_masks[cl])
        if plot_with_gt:
            gt_img = t["d_gt"][cl]
            if plot_with_img:
                gt_img = img = ev.blend(img, gt_img, out=img)     # :249 blends into the scan itself: later classes start from it
            out_img = torch.cat((out_img, gt_img), dim=1)
        _write_image(out_path(save_folder, t["path"], cl), ev.to_host(out_img))
