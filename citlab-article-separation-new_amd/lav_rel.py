"""Relation net evaluation ("load and validate"): ``article_separation/gnn/trainer/lav_rel.py`` on the MI355X engine.

    python -m citlab_article_separation_new_amd.lav_rel --model_dir <dir or .pb> --eval_list jsons.lst \\
        --input_params node_feature_dim=15 edge_feature_dim=2 node_input_feature_mask=[1,1,1,1,0,0,0,0,0,0,0,0,1,1,1]

The reference runs the frozen graph over all N * N ordered pairs of every page of ``--eval_list``, concatenates the class-1
probabilities and the ``gt_relations`` labels on the host and hands them to sklearn's ``precision_recall_curve``,
``roc_auc_score`` and ``accuracy_score`` (``lav_rel.py:190-229``).  Here the probabilities never leave HBM: every page's
output buffer is appended to a device accumulator (``asep_releval_*``, include/asep_hip.h) as packed 32-bit keys
``(float_bits(p) << 1) | label``; one radix sort and one scan give sklearn's ``_binary_clf_curve`` -- per distinct score, in
descending order, the score and the counts ``tps`` / ``fps`` -- as exact integers.  Precision, recall, F1, the three tables,
AUC-ROC and accuracy are built from those counts with the float64 divisions sklearn 1.7.2 does (the yardstick: its
``precision_recall_curve`` keeps every threshold; older releases cut the curve where full recall is first reached).
There is no CPU path: without a GPU the accumulator raises the package's usual error.
"""
import ctypes as C
import logging
import os
import sys
import time
import warnings

import numpy as np

from . import _lib, cli_flags

SKLEARN_PIN = "1.7.2"
MAX_PAIRS = (1 << 31) - 1            # one accumulator: every count is a 32-bit number on the device
_BITS_ONE = 0x3F800000


class UndefinedMetricWarning(UserWarning):
    """stands in for sklearn.exceptions.UndefinedMetricWarning (the package does not import sklearn)"""


# ---- the key (host restatement of csrc/relation_eval_kernels.h, for tests and documentation) ---------------------------------
def pack_keys(probs, labels):
    """float32 scores in [0, 1] and 0/1 labels -> uint32 keys whose unsigned order is the order of (score, label)"""
    bits = np.ascontiguousarray(probs, np.float32).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0                                   # -0.0 is 0.0
    if np.any(bits > _BITS_ONE):
        raise ValueError("scores must lie in [0, 1] (no NaN): the key keeps 31 bits of the float")
    return (bits << np.uint32(1)) | (np.asarray(labels) != 0).astype(np.uint32)


def unpack_keys(keys):
    keys = np.asarray(keys, np.uint32)
    return (keys >> np.uint32(1)).view(np.float32), (keys & np.uint32(1)).astype(np.int64)


# ---- from counts to what lav_rel.py logs -------------------------------------------------------------------------------------
class RelationCurve:
    """sklearn's ``_binary_clf_curve`` of an evaluation: ``thresholds`` float32 [T] = the distinct scores in DESCENDING order,
    ``tps`` / ``fps`` int64 [T] = the pairs of label 1 / 0 whose score is >= the threshold; ``n_correct`` = the pairs with
    (score > 0.5) == label; ``a2`` = sum_k (fps_k - fps_{k-1}) (tps_k + tps_{k-1}) if the device computed it."""

    def __init__(self, thresholds, tps, fps, n_correct, a2=None):
        self.thresholds = np.ascontiguousarray(thresholds, np.float32)
        self.tps = np.ascontiguousarray(tps, np.int64)
        self.fps = np.ascontiguousarray(fps, np.int64)
        if not (len(self.thresholds) == len(self.tps) == len(self.fps)) or len(self.tps) == 0:
            raise ValueError("an evaluation needs at least one pair: the list gave no relations to score")
        self.n_pos, self.n_neg = int(self.tps[-1]), int(self.fps[-1])
        self.n_correct = int(n_correct)
        if a2 is None:
            dfp = np.diff(self.fps, prepend=0).astype(np.uint64)
            stp = (self.tps + np.concatenate([[0], self.tps[:-1]])).astype(np.uint64)
            a2 = int(np.sum(dfp * stp, dtype=np.uint64))
        self.a2 = int(a2)

    @property
    def n(self):
        return self.n_pos + self.n_neg

    @property
    def accuracy(self):
        """accuracy_score(targets, probs > 0.5): the mean of exact 0 / 1 values"""
        return self.n_correct / self.n

    @property
    def auc_roc(self):
        """roc_auc_score: the trapezoid area under (fps / Ng, tps / P) as ONE division of exact integers.  One class only:
        sklearn 1.7.2 warns and returns nan (older releases raised ValueError); so does this."""
        if self.n_pos == 0 or self.n_neg == 0:
            warnings.warn("Only one class is present in y_true. ROC AUC score is not defined in that case.", UndefinedMetricWarning)
            return float("nan")
        return self.a2 / (2 * self.n_pos * self.n_neg)

    def precision_recall_curve(self):
        """(precision, recall, thresholds) as sklearn.metrics.precision_recall_curve returns them: float64, float64 and float32,
        thresholds ascending, a final (1, 0) point appended."""
        tps, fps = self.tps.astype(np.float64), self.fps.astype(np.float64)
        ps = tps + fps
        precision = np.zeros_like(tps)
        np.divide(tps, ps, out=precision, where=(ps != 0))
        if tps[-1] == 0:
            warnings.warn("No positive class found in y_true, recall is set to one for all thresholds.")
            recall = np.ones_like(tps)
        else:
            recall = tps / tps[-1]
        sl = slice(None, None, -1)
        return np.hstack((precision[sl], 1)), np.hstack((recall[sl], 0)), self.thresholds[sl]


def f_scores(prec, rec):
    """lav_rel.py:193-194: 2 p r / (p + r), NaN (0 / 0) -> 0"""
    with np.errstate(divide="ignore", invalid="ignore"):
        f_score = (2 * prec * rec) / (prec + rec)
    f_score[np.isnan(f_score)] = 0
    return f_score


_HEAD = (f" |{'Threshold':>10}{'Precision':>12}{'Recall':>12}{'F1-Score':>12}", " | " + "-" * 45)


def _row(thresholds, prec, rec, f_score, i):
    return f" |{thresholds[i]:10f}{prec[i]:12f}{rec[i]:12f}{f_score[i]:12f}"


def relative_rows(n_thresholds, num_p_r_thresholds):
    """lav_rel.py:200-201: the indices of the "relative thresholds" table"""
    return [j * ((n_thresholds - 1) // num_p_r_thresholds) for j in range(num_p_r_thresholds + 1)]


def fixed_rows(thresholds, num_p_r_thresholds):
    """lav_rel.py:208-215: the first threshold at or above every multiple of 1 / num_p_r_thresholds"""
    rows = []
    step = 1 / num_p_r_thresholds
    j = 0
    for i in range(len(thresholds)):
        if thresholds[i] >= j * step:
            rows.append(i)
            j += 1
            if j * step >= 1.0:
                break
    return rows


def table_lines(prec, rec, thresholds, num_p_r_thresholds):
    """the three tables of lav_rel.py:196-222, line for line"""
    f_score = f_scores(prec, rec)
    lines = ["Relative Thresholds:", *_HEAD]
    lines += [_row(thresholds, prec, rec, f_score, i) for i in relative_rows(len(thresholds), num_p_r_thresholds)]
    lines += ["Fixed Thresholds:", *_HEAD]
    lines += [_row(thresholds, prec, rec, f_score, i) for i in fixed_rows(thresholds, num_p_r_thresholds)]
    i_f = np.argmax(f_score)
    lines += ["Best F1-Score:", *_HEAD, _row(thresholds, prec, rec, f_score, i_f)]
    return lines


def report_lines(curve, num_p_r_thresholds):
    """everything lav_rel.py logs between the loop and the time: the tables, AUC-ROC and accuracy"""
    prec, rec, thresholds = curve.precision_recall_curve()
    lines = table_lines(prec, rec, thresholds, num_p_r_thresholds)
    lines.append(f"AUC-ROC: {curve.auc_roc:12f}")
    lines.append(f"Accuracy: {curve.accuracy:12f}")
    return lines


# ---- the device accumulator --------------------------------------------------------------------------------------------------
def _stream(device):
    import torch
    return torch.cuda.current_stream(device).cuda_stream or None


class RelationEval:
    """``asep_releval_*``: (score, label) pairs accumulate in HBM; ``finish`` sorts them and returns a :class:`RelationCurve`.
    Every call is queued on torch's current stream of the device."""

    def __init__(self, device=0):
        self.device = int(device)
        self._lib = _lib.init_device(self.device)                     # AsepError without a GPU: there is no CPU path
        self._h = self._lib.asep_releval_create()
        if not self._h:
            raise _lib.AsepError("asep_releval_create failed: " + _lib.last_error())
        self._keep = []                                                # uploads a queued kernel still reads

    def close(self):
        if self._h:
            self._lib.asep_releval_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._lib.asep_releval_count(self._h))

    def reset(self):
        _lib.check(self._lib.asep_releval_reset(self._h, _stream(self.device)), "asep_releval_reset")
        self._keep = []

    def reserve(self, total_pairs):
        if total_pairs > MAX_PAIRS:
            raise ValueError(f"{total_pairs} pairs: one accumulator holds fewer than 2^31 pairs")
        _lib.check(self._lib.asep_releval_reserve(self._h, int(total_pairs), _stream(self.device)), "asep_releval_reserve")

    def append_page(self, d_probs, N, gt_relations, num_classes=None):
        """One page behind its forward: ``d_probs`` = the net's output [N * N, num_classes] in HBM (a torch tensor, or an
        address with ``num_classes`` given), ``gt_relations`` [G, 3] (host array or device tensor).  Nothing is copied back."""
        import torch
        N = int(N)
        if hasattr(d_probs, "data_ptr"):
            if not d_probs.is_contiguous() or d_probs.dtype != torch.float32 or d_probs.numel() % max(N * N, 1):
                raise ValueError(f"d_probs must be a contiguous float32 [N * N, classes] tensor, N = {N}")
            num_classes = d_probs.numel() // (N * N) if N else (num_classes or 2)
            self._keep.append(d_probs)
            d_probs = d_probs.data_ptr()
        elif num_classes is None:
            raise ValueError("num_classes is needed with a raw address")
        if hasattr(gt_relations, "data_ptr"):
            gt = gt_relations.to(torch.int32).contiguous().reshape(-1, 3)
        else:
            g = np.ascontiguousarray(np.asarray(gt_relations if gt_relations is not None else [], np.int32).reshape(-1, 3))
            if g.size and (g[:, 1:].min() < 0 or g[:, 1:].max() >= N):
                raise IndexError(f"gt_relations names a node outside 0..{N - 1}")
            gt = torch.from_numpy(g).to(f"cuda:{self.device}") if g.size else None
        G = 0 if gt is None else int(gt.shape[0])
        if G:
            self._keep.append(gt)
        _lib.check(self._lib.asep_releval_append_dev(self._h, d_probs, int(num_classes), N * N, gt.data_ptr() if G else None, G, N,
                                                     _stream(self.device)), "asep_releval_append_dev")

    def append(self, probs, labels):
        """host arrays: scores [n] and 0 / 1 labels [n]"""
        p = np.ascontiguousarray(probs, np.float32).reshape(-1)
        y = np.asarray(labels).reshape(-1)
        if p.shape != y.shape:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{len(y)}, {len(p)}]")
        if y.size and not np.isin(y, (0, 1)).all():
            raise ValueError("labels must be 0 or 1")
        y = np.ascontiguousarray(y, np.uint8)
        _lib.check(self._lib.asep_releval_append_host(self._h, p.ctypes.data, y.ctypes.data, p.size, _stream(self.device)),
                   "asep_releval_append_host")

    def finish(self):
        """sort + curve -> RelationCurve.  Refuses what sklearn (or the key) refuses: no pairs, scores that are NaN, negative or
        above 1, ground truth rows outside the page."""
        t = C.c_longlong(0)
        _lib.check(self._lib.asep_releval_finish(self._h, _stream(self.device), C.byref(t)), "asep_releval_finish")
        self._keep = []
        T = int(t.value)
        thresholds, tps, fps = np.empty(T, np.float32), np.empty(T, np.int64), np.empty(T, np.int64)
        cnt = np.zeros(8, np.uint64)
        _lib.check(self._lib.asep_releval_fetch(self._h, _stream(self.device), thresholds.ctypes.data, tps.ctypes.data,
                                                fps.ctypes.data, cnt.ctypes.data), "asep_releval_fetch")
        n, bad, pos, correct, bad_gt, a2, _, pos_sorted = (int(v) for v in cnt)
        if n == 0:
            raise ValueError("an evaluation needs at least one pair: the list gave no relations to score")
        if bad_gt:
            raise IndexError(f"{bad_gt} rows of gt_relations name a node outside their page")
        if bad:
            raise ValueError(f"Input contains NaN, infinity or a value outside [0, 1]: {bad} of {n} scores (class probabilities expected)")
        if pos != pos_sorted or pos != int(tps[-1]) or int(tps[-1] + fps[-1]) != n:
            raise _lib.AsepError(f"relation evaluation: the appends counted {pos} positives of {n} pairs, the sorted keys hold "
                                 f"{pos_sorted} / the curve ends at {int(tps[-1])} + {int(fps[-1])}")
        return RelationCurve(thresholds, tps, fps, correct, a2)

    def stage_us(self):
        """device time of every kernel of the last finish: {name: microseconds}"""
        names = [f"pass{p}_{k}" for p in range(4) for k in ("hist", "scan", "scatter")] + ["curve_count", "curve_scan", "curve_write", "a2"]
        return {nm: float(self._lib.asep_releval_stage_us(self._h, i)) for i, nm in enumerate(names)}


# ---- command line (lav_rel.py:18-61) -----------------------------------------------------------------------------------------
def build_parser():
    p = cli_flags.LineArgumentParser(fromfile_prefix_chars="@")
    b = dict(nargs="?", const=True, type=cli_flags.str2bool)
    p.add_argument("--model_dir", type=str, default="")
    p.add_argument("--model_type", type=str, default="ModelRelation")
    p.add_argument("--eval_list", type=str, default="")
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--num_relation_components", type=int, default=2)
    p.add_argument("--sample_num_relations_to_consider", type=int, default=100)
    p.add_argument("--sample_relations", default=False, **b)
    p.add_argument("--image_input", default=False, **b)
    p.add_argument("--assign_visual_features_to_nodes", default=True, **b)
    p.add_argument("--assign_visual_features_to_edges", default=False, **b)
    p.add_argument("--backbone", type=str, default="ARU_v1")
    p.add_argument("--mvn", default=True, **b)
    cli_flags.define_dict(p, "graph_backbone_params", {})
    cli_flags.define_feature_map_layout(p, {"layer_depth": [-1, -1, -1]})   # (+ the extensions --visual_layers / --visual_layer_depths, as in run_gnn_clustering)
    cli_flags.define_dict(p, "input_params", {})
    p.add_argument("--num_p_r_thresholds", type=int, default=20)
    p.add_argument("--gpu_devices", type=int, nargs="*", default=[])
    p.add_argument("--gpu_memory_fraction", type=float, default=0.95)       # steers TensorFlow only: accepted, ignored
    p.add_argument("--batch_limiter", type=int, default=-1)
    p.add_argument("--try_gpu", default=None, **b)                          # default: True if --gpu_devices is given (:59-60)
    # extensions
    p.add_argument("--num_workers", type=int, default=1)                    # host workers that prepare pages ahead of the GPU owner
    p.add_argument("--pages_per_call", type=cli_flags.pages_per_call, default=1)   # as in run_gnn_clustering: pages of one engine call
    p.add_argument("--device_resize", default=False, **b)                   # as in run_gnn_clustering: True = the uint8 scan is resized on the device
    return p


def parse_flags(argv=None):
    flags = build_parser().parse_known_args(argv)[0]
    if flags.try_gpu is None:
        flags.try_gpu = flags.gpu_devices != []
    return flags


def check_flags(flags):
    if flags.model_type != "ModelRelation":
        raise ValueError(f"--model_type {flags.model_type}: only 'ModelRelation' exists")
    if flags.sample_relations:
        raise ValueError("--sample_relations True: the reference samples the relations at random inside tf.data, so there is no "
                         "result to be equal to; the evaluation runs on the full graph (all N * N ordered pairs)")
    if flags.num_classes < 2:
        raise ValueError("--num_classes must be at least 2")


_eval_state = {}


def _prepare_eval_page(argv, json_path, image_later=False, device_resize=False):
    """host worker: json (+ scan, unless it comes through a decode slot: ``image_later``) -> (feed dict, N, gt_relations) or None.
    ``device_resize`` False: the scan resized on the host under 'image:0'; True (what ``evaluate`` asks for under --device_resize):
    the scan as decoded under 'image_u8:0'"""
    from . import run_gnn_clustering
    from .gnn_input import InputGNN
    key = tuple(argv)
    if key not in _eval_state:
        flags = parse_flags(list(argv))
        _eval_state[key] = (flags, InputGNN(flags))
    flags, input_fn = _eval_state[key]
    if not os.path.isfile(json_path):
        logging.warning(f"No json file {json_path}. Skipping.")
        return None
    targets = {}
    feed, n = run_gnn_clustering._prepare_feed(input_fn, flags, json_path, targets, image_later=image_later, device_resize=device_resize)
    return feed, n, targets["gt_relations"]


def _feed_arrays(feed, cfg):
    """the arrays GnnSession.run takes out of a feed dict (gnn_io.py), without the relations: all pairs are scored"""
    N = int(np.asarray(feed["num_nodes:0"]).reshape(-1)[0])
    E = int(np.asarray(feed["num_interacting_nodes:0"]).reshape(-1)[0])
    a = {"N": N, "E": E, "edges": np.ascontiguousarray(np.asarray(feed["interacting_nodes:0"], np.int32)[0][:E]).reshape(-1, 2)}
    if "node_features:0" in feed:
        u = np.ascontiguousarray(np.asarray(feed["node_features:0"], np.float32)[0][:N])
    elif cfg.visual_dims and cfg.node_feature_dim == 0:
        u = np.zeros((N, 0), np.float32)
    else:
        raise KeyError("feed_dict lacks node_features:0")
    if u.shape[1] != cfg.node_feature_dim:
        raise ValueError(f"node_features has dim {u.shape[1]}, model expects {cfg.node_feature_dim}")
    a["u"] = u
    a["ef"] = None
    if cfg.edge_feature_dim:
        ef = np.ascontiguousarray(np.asarray(feed["edge_features:0"], np.float32)[0][:E])
        if ef.shape[1] != cfg.edge_feature_dim:
            raise ValueError(f"edge_features has dim {ef.shape[1]}, model expects {cfg.edge_feature_dim}")
        a["ef"] = ef
    if cfg.visual_dims:
        from .gnn_io import IMAGE_U8, resize_mode
        from_scan = IMAGE_U8 in feed
        for k in ((IMAGE_U8, "image_shape:0") if from_scan else ("image:0",)) + ("visual_regions_nodes:0",
                                                                                 "num_points_visual_regions_nodes:0"):
            if k not in feed:
                raise KeyError(f"this graph was exported with image_input: feed_dict lacks {k}")
        if from_scan:                                        # the scan as decoded: resized on the device behind its upload
            ish = np.asarray(feed["image_shape:0"]).reshape(-1, 3)[0]
            a["page_u8"] = np.ascontiguousarray(np.asarray(feed[IMAGE_U8])[0])
            a["resize"] = (int(ish[0]), int(ish[1]), resize_mode(a["page_u8"].shape, cfg.backbone_cfg().channels))
        else:
            image = np.asarray(feed["image:0"], np.float32)[0]
            if "image_shape:0" in feed:
                ish = np.asarray(feed["image_shape:0"]).reshape(-1, 3)[0]
                image = image[:int(ish[0]), :int(ish[1])]
            if image.ndim == 3 and cfg.backbone_cfg().channels == 1:
                image = image[:, :, 0]
            a["image"] = np.ascontiguousarray(image)         # [h,w], or [h,w,3] for a colour backbone
        a["regions"] = np.ascontiguousarray(np.asarray(feed["visual_regions_nodes:0"], np.float32)[0][:N])
        a["npts"] = np.ascontiguousarray(np.asarray(feed["num_points_visual_regions_nodes:0"], np.int32)[0][:N])
        if cfg.visual_edges:
            for k in ("visual_regions_edges:0", "num_points_visual_regions_edges:0"):
                if k not in feed:
                    raise KeyError(f"this graph assigns visual features to edges: feed_dict lacks {k}")
            a["eregions"] = np.ascontiguousarray(np.asarray(feed["visual_regions_edges:0"], np.float32)[0][:E])
            a["enpts"] = np.ascontiguousarray(np.asarray(feed["num_points_visual_regions_edges:0"], np.int32)[0][:E])
    return a


class LavGNN(object):
    """lav_rel.py:64-234.  ``evaluate()`` logs what the reference logs and returns the :class:`RelationCurve`."""

    def __init__(self, flags=None, argv=None):
        self._argv = list(sys.argv[1:] if argv is None and flags is None else (argv or []))
        self._flags = flags if flags is not None else parse_flags(self._argv)
        if self._flags.try_gpu is None:
            self._flags.try_gpu = self._flags.gpu_devices != []
        check_flags(self._flags)
        from .run_gnn_clustering import resolve_model_path
        self._pb_path = resolve_model_path(self._flags)
        logging.info(f"Using pb_path: {self._pb_path}")
        self.device = int(self._flags.gpu_devices[0]) if self._flags.gpu_devices else 0
        self.timings = {}

    def _forward_dev(self, graph, a, keep):
        """one page through the device-resident entries on torch's current stream -> its output buffer [N * N, classes] in HBM"""
        return self._launch_pages(graph, [self._upload_page(graph, a)], keep)[0]

    def _launch_pages(self, graph, recs, keep):
        """the uploaded pages of one call (``_upload_page``) -> their output buffers, in order.  One page of a visual model goes through
        asep_gnn_forward_visual_batch_dev as ever, several -- of whatever image sizes -- through ONE asep_gnn_forward_visual_batch_dev2
        call; a model without the visual branch runs page by page, or with --pages_per_call > 1 through ONE asep_gnn_forward_batch_dev call
        (``_launch_graph_batch``: every stage of the graph part one launch over the pages)."""
        from . import gnn_io
        stream = _stream(self.device)
        cfg = graph.cfg
        if cfg.visual_dims and len(recs) == 1 and recs[0]["scan"] is None:
            r = recs[0]
            gnn_io.gnn_forward_visual_batch_dev(graph, [r["page"]], r["h"], r["w"], r["P"], stream, self.device)
        elif cfg.visual_dims:
            if len({r["P"] for r in recs}) != 1:
                raise ValueError("the pages of one call must have regions of one point count")
            fed = [r["page"] for r in recs], [r["h"] for r in recs], [r["w"] for r in recs]
            if all(r["scan"] is not None for r in recs):     # --device_resize: every scan of the call resized in one launch
                gnn_io.gnn_forward_visual_batch_u8_dev(graph, fed[0], [r["scan"] for r in recs], fed[1], fed[2], recs[0]["P"], stream, self.device)
            else:
                gnn_io.gnn_forward_visual_batch_dev2(graph, *fed, recs[0]["P"], stream, self.device)
        elif "a" in recs[0]:                                 # --pages_per_call > 1 without the visual branch (a tail of one page included)
            return self._launch_graph_batch(graph, recs, keep)
        else:
            lib = _lib.init_device(self.device)
            for r in recs:
                q = r["page"]
                _lib.check(lib.asep_gnn_forward_dev(graph.handle(self.device), q["N"], q["E"], q["d_edges"], q["d_node_feat"], q["d_edge_feat"],
                                                    q["R"], None, q["d_probs_out"], stream), "asep_gnn_forward_dev")
        keep.extend(r["t"] for r in recs)
        return [r["out"] for r in recs]

    def _launch_graph_batch(self, graph, recs, keep):
        """the pages of a model without the visual branch (``_upload_page`` with ``to_call``: their host arrays) in ONE
        asep_gnn_forward_batch_dev call: one upload per input, every stage of the graph one launch over all pages -> per page its slice
        [N * N] of the call's class-1 probabilities in HBM (the score column the accumulator reads)"""
        import torch
        from . import gnn_io
        cfg = graph.cfg
        arrays = [r["a"] for r in recs]
        for a in arrays:
            gnn_io._check_node_indices("interacting_nodes", a["edges"], a["N"])
        N, E, R, u, edges, ef, _ = gnn_io.pack_graph_pages(arrays, cfg.node_feature_dim, cfg.edge_feature_dim)
        dev = f"cuda:{self.device}"
        t = [torch.from_numpy(x).to(dev) if x is not None and x.size else None for x in (u, edges, ef)]
        ptr = lambda x: x.data_ptr() if x is not None else None                                    # noqa: E731
        total = int(R.sum(dtype=np.int64))
        out = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        gnn_io.gnn_forward_batch_dev(graph, N, E, R, ptr(t[0]), ptr(t[1]), ptr(t[2]), None, out.data_ptr(), total, _stream(self.device),
                                     self.device)
        keep.append(t)
        ends = np.cumsum(R.astype(np.int64))
        return [out[int(e - r):int(e)] for e, r in zip(ends, R)]

    def _upload_page(self, graph, a, scan_to_call=False, to_call=False):
        """the arrays of one page into HBM (+ the device resize of a scan) -> what ``_launch_pages`` takes.  ``scan_to_call``: a scan is
        left as uploaded, for a call that resizes all its scans in one launch (asep_gnn_forward_visual_batch_u8_dev)"""
        import torch
        if to_call:                                          # no visual branch, several pages per call: the call uploads them together
            return {"a": a, "scan": None}
        dev = f"cuda:{self.device}"
        up = lambda x: torch.from_numpy(x).to(dev) if x is not None and x.size else None            # noqa: E731
        ptr = lambda t: t.data_ptr() if t is not None else None                                    # noqa: E731
        N, E, cfg = a["N"], a["E"], graph.cfg
        # (a blocking copy each: a page that sits in a decode slot is in HBM before the slot goes back to the pool)
        with warnings.catch_warnings():                      # (a page Pillow decoded is read-only: it is only read here)
            warnings.simplefilter("ignore", UserWarning)
            t = {k: up(a.get(k)) for k in ("edges", "u", "ef", "image", "page_u8", "regions", "npts", "eregions", "enpts")}
        scan = None
        h = w = P = 0
        if "resize" in a and scan_to_call:
            h, w, _ = a["resize"]
            sh = a["page_u8"].shape
            scan = (t["page_u8"].data_ptr(), sh[0], sh[1], sh[2] if len(sh) == 3 else 1)
        elif "resize" in a:
            from . import image_ops
            h, w, mode = a["resize"]
            t["image"] = image_ops.resize_tf1_dev(t["page_u8"], h, w, mode, self.device)
            t["page_u8"] = None                              # (queued on torch's current stream: its allocator keeps the block until then)
        out = torch.empty((N * N, cfg.num_classes), dtype=torch.float32, device=dev)
        if cfg.visual_dims:
            if scan is None:
                h, w = t["image"].shape[:2]
            P = a["regions"].shape[2]
        page = dict(N=N, E=E, R=N * N, d_edges=ptr(t["edges"]), d_node_feat=ptr(t["u"]), d_edge_feat=ptr(t["ef"]),
                    d_image=ptr(t["image"]), d_regions=ptr(t["regions"]), d_num_points=ptr(t["npts"]),
                    d_edge_regions=ptr(t["eregions"]), d_edge_num_points=ptr(t["enpts"]), d_relations=None,
                    d_probs_out=out.data_ptr())
        return {"page": page, "h": int(h), "w": int(w), "P": int(P), "t": t, "out": out, "scan": scan}

    def _pages(self, json_paths):
        """(feed, N, gt_relations) or None per list entry, prepared by host workers ahead of the caller when --num_workers > 1"""
        flags = self._flags
        workers = max(1, int(getattr(flags, "num_workers", 1) or 1))
        if workers <= 1 or not self._argv:
            for p in json_paths:
                yield _prepare_eval_page(self._argv_key(), p, False, bool(getattr(flags, "device_resize", False)))
            return
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        from . import run_gnn_clustering
        from .host_pipeline import single_threaded_children
        later = bool(flags.image_input and getattr(flags, "device_resize", False))    # the json half only: the scan comes through a slot
        scans = None
        if later:                                                    # the decoders start first
            _, input_fn = self._eval_objects()
            scans = run_gnn_clustering._ScanSlots(json_paths, input_fn.input_params["load_mode"], self.device, workers)
        with ProcessPoolExecutor(max(1, workers - run_gnn_clustering._slot_decoders(workers)) if later else workers,
                                 mp_context=mp.get_context("spawn")) as pool:
            def submit(p):
                with single_threaded_children():
                    return pool.submit(_prepare_eval_page, self._argv_key(), p, later, False)     # (host resize, or the json half)
            ahead = 2 * workers
            pending = [submit(p) for p in json_paths[:ahead]]
            try:
                for k in range(len(json_paths)):
                    page = pending[k].result()
                    pending[k] = None
                    if k + ahead < len(json_paths):
                        pending.append(submit(json_paths[k + ahead]))
                    if page is not None and scans is not None:
                        _, scan = next(scans)                        # (valid until the next one is asked for)
                        page[0].update(input_fn.image_feeds(scan, True))
                        del scan
                    yield page
                    page = None
            finally:
                page = None
                if scans is not None:
                    scans.close()

    def _eval_objects(self):
        key = self._argv_key()
        if key not in _eval_state:
            from .gnn_input import InputGNN
            flags = parse_flags(list(key))
            _eval_state[key] = (flags, InputGNN(flags))
        return _eval_state[key]

    def _argv_key(self):
        if not self._argv:                                           # flags were handed in as an object: the same process prepares
            key = ("<flags>", id(self._flags))
            if key not in _eval_state:
                from .gnn_input import InputGNN
                _eval_state[key] = (self._flags, InputGNN(self._flags))
            return key
        return tuple(self._argv)

    def evaluate(self):
        import torch
        from . import gnn_io
        from .path_util import load_list_file
        flags = self._flags
        logging.info("Start evaluation...")
        json_paths = [p for p in load_list_file(flags.eval_list) if p]
        acc = RelationEval(self.device)                              # (no GPU: the package's error, before any work)
        layers, depths = cli_flags.visual_layout(flags)
        graph = gnn_io.load_graph(self._pb_path, visual_layers=layers, visual_layer_depths=depths)
        if graph.cfg.visual_dims and not flags.image_input:
            raise ValueError("this model was exported with image_input: pass --image_input True")
        from .gnn_input import check_load_mode
        check_load_mode(flags.input_params, graph.cfg)               # before the model goes to the device
        if graph.cfg.num_classes != flags.num_classes:
            raise ValueError(f"--num_classes {flags.num_classes}, the model has {graph.cfg.num_classes}")
        tm = self.timings = {"net_s": 0.0, "append_s": 0.0, "finish_s": 0.0, "prepare_wait_s": 0.0, "pages": 0}
        keep = []
        batch_counter = 0
        start_timer = time.time()
        if flags.batch_limiter != -1:
            limited = json_paths[:max(0, flags.batch_limiter)]
        else:
            limited = json_paths
        pages = self._pages(limited)
        per_call = max(1, int(getattr(flags, "pages_per_call", 1) or 1))
        group = []

        def flush():
            """the collected pages through one engine call; their pairs reach the accumulator in input order"""
            t0 = time.perf_counter()
            outs = self._launch_pages(graph, [r for r, _, _ in group], keep)
            t1 = time.perf_counter()
            for out, (_, n, gt_relations) in zip(outs, group):
                acc.append_page(out, n, gt_relations)
            del group[:]
            tm["net_s"] += t1 - t0
            tm["append_s"] += time.perf_counter() - t1
            if len(keep) > 64:                                        # bounded backlog of uploads the queued kernels read
                torch.cuda.current_stream(self.device).synchronize()
                del keep[:]
        try:
            while True:
                if flags.batch_limiter != -1 and flags.batch_limiter <= batch_counter:
                    logging.info(f"Stop validation after {batch_counter} batches with")
                    break
                t0 = time.perf_counter()
                try:
                    page = next(pages)
                except StopIteration:
                    break
                tm["prepare_wait_s"] += time.perf_counter() - t0
                if page is None:
                    continue
                batch_counter += 1
                feed, n, gt_relations = page
                t0 = time.perf_counter()
                group.append((self._upload_page(graph, _feed_arrays(feed, graph.cfg), scan_to_call=per_call > 1,
                                                to_call=per_call > 1 and gnn_io.graph_batch_serves(graph.cfg)), n, gt_relations))
                feed = page = None                                    # (a scan fed from a decode slot: no view outlives its slot)
                tm["net_s"] += time.perf_counter() - t0
                if len(group) >= per_call:
                    flush()
            if group:                                                 # the tail: fewer pages than a full call
                flush()
        finally:
            pages.close()
        tm["pages"] = batch_counter
        t0 = time.perf_counter()
        curve = acc.finish()
        tm["finish_s"] = time.perf_counter() - t0
        tm["stage_us"] = acc.stage_us()
        for line in report_lines(curve, flags.num_p_r_thresholds):
            logging.info(line)
        logging.info(f"Time: {time.time() - start_timer:.2f} seconds")
        acc.close()
        graph.close()
        logging.info("Evaluation finished.")
        return curve


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    warnings.filterwarnings("ignore")
    logging.getLogger().setLevel("INFO")
    if not logging.getLogger().handlers:
        logging.basicConfig(level=logging.INFO)
    logging.info("Running Evaluation.")
    eval_rel = LavGNN(argv=argv)
    return eval_rel.evaluate()


if __name__ == "__main__":
    main()
    sys.exit(0)
