"""Article separation measure (the reference's ``article_separation_measure`` package) on the GPU.

    BaselineMeasure(Result)      baseline_measure.py:6-90                      (host, restated)
    BaselineMeasureEval          eval_measure.py:10-258 (use_java_code=False)  -> asep_measure_run / asep_measure_fetch
    run_eval, get_greedy_sum     run_measure.py:14-244                         (host over the device's sparse results)
    f_measure                    python_util/math/measure.py:5-18

The ICDAR 2017 baseline detection measure (R / P / F over all baselines and over the baselines with an article id) and
the ICPR 2020 article / block segmentation measure built on it.  The results are those of the reference's Python path;
the Java class it can call instead has no source and is not used.

One device call serves every job of a file pair, and the file pairs of a batch share it: the minimum L1 distance of a
reco point to truth polygon j does not depend on the subset that is scored, only j's tolerance does, and the HY
articles partition the reco polygons.  The device returns, for candidate polygon pairs only (bounding boxes at most
3 * largest tolerance apart), ``count_rel_hits`` per (reco, truth) pair and ``count_rel_hits_list`` per (truth, HY
article), per truth against all reco polygons and per truth against the reco polygons with an id; the greedy
alignments, the weighting and the averaging run here on those sparse results.  No CPU fallback: without the HIP library
every evaluation raises ``AsepError``.
"""
import ctypes as C
import math

import numpy as np

from . import textblock_geometry as geo

MAX_D = 250          # calc_tols' max_d as eval_measure.py:74 passes it


# ---- baseline_measure.py --------------------------------------------------------------------------------------------

class BaselineMeasureResult(object):
    def __init__(self):
        self.page_wise_per_dist_tol_tick_per_line_recall = []
        self.page_wise_per_dist_tol_tick_recall = []
        self.page_wise_recall = []
        self.recall = 0.0
        self.page_wise_per_dist_tol_tick_per_line_precision = []
        self.page_wise_per_dist_tol_tick_precision = []
        self.page_wise_precision = []
        self.precision = []


def _page_value(per_tick_per_line):
    """baseline_measure.py:34-42: mean over the lines per tick, then mean over the ticks, in numpy's order."""
    per_tick = np.sum(per_tick_per_line, axis=1)
    per_tick /= per_tick_per_line.shape[1]
    value = np.sum(per_tick)
    value /= per_tick.shape[0]
    return per_tick, value


class BaselineMeasure(object):
    def __init__(self):
        self.result = BaselineMeasureResult()

    def add_per_dist_tol_tick_per_line_recall(self, per_dist_tol_tick_per_line_recall):
        """#distTolTicks x #truthBaseLines matrix of recalls"""
        r = self.result
        r.page_wise_per_dist_tol_tick_per_line_recall.append(per_dist_tol_tick_per_line_recall)
        per_tick, value = _page_value(per_dist_tol_tick_per_line_recall)
        r.page_wise_per_dist_tol_tick_recall.append(per_tick)
        r.page_wise_recall.append(value)
        self.calc_recall()

    def add_per_dist_tol_tick_per_line_precision(self, per_dist_tol_tick_per_line_precision):
        """#distTolTicks x #recoBaseLines matrix of precisions"""
        r = self.result
        r.page_wise_per_dist_tol_tick_per_line_precision.append(per_dist_tol_tick_per_line_precision)
        per_tick, value = _page_value(per_dist_tol_tick_per_line_precision)
        r.page_wise_per_dist_tol_tick_precision.append(per_tick)
        r.page_wise_precision.append(value)
        self.calc_precision()

    def calc_recall(self):
        avg = 0.0
        for v in self.result.page_wise_recall:
            avg += v
        self.result.recall = avg / len(self.result.page_wise_recall)

    def calc_precision(self):
        avg = 0.0
        for v in self.result.page_wise_precision:
            avg += v
        self.result.precision = avg / len(self.result.page_wise_precision)


def f_measure(precision, recall):
    if precision == 0 and recall == 0:
        return 0.0
    return 2.0 * precision * recall / (precision + recall)


# ---- greedy alignment on sparse entries --------------------------------------------------------------------------------

def greedy_alignment(rows, cols, vals, stop_below=0.0, inclusive=False):
    """The loop of eval_measure.py:108-123 / run_measure.py:115-135 on the entries (rows[k], cols[k]) -> vals[k] of a
    matrix whose other entries are zero: repeatedly take the largest remaining entry (numpy's argmax: the first in
    row-major order among equals) and strike its row and column.  Returns the chosen entry indices in order.  Entries
    below ``stop_below`` end the sweep (``inclusive``: entries equal to it too -- zero entries of a non-negative matrix
    change neither a precision nor a sum, which is why the sparse form may leave them out)."""
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, np.float64)
    order = np.lexsort((cols, rows, -vals))
    used_r, used_c, chosen = set(), set(), []
    for k in order.tolist():
        v = vals[k]
        if v < stop_below or (inclusive and v == stop_below):
            break
        r, c = int(rows[k]), int(cols[k])
        if r in used_r or c in used_c:
            continue
        used_r.add(r)
        used_c.add(c)
        chosen.append(k)
    return chosen


def get_greedy_sum(array):
    """run_measure.py:115-135 on a dense matrix."""
    a = np.asarray(array, np.float64)
    rr, cc = np.indices(a.shape)
    rr, cc, vv = rr.ravel(), cc.ravel(), a.ravel()
    s = 0
    for k in greedy_alignment(rr, cc, vv):
        s += vv[k]
    return s


# ---- tolerances ------------------------------------------------------------------------------------------------------

def tols_from_distances(dists, max_d=MAX_D, rel_tol=0.25):
    """util.py:880-900 (calc_tols after its distance loop): ``dists`` are the interline distances with max_d where none
    was found below max_d.  0 for "not below max_d" (a distance of exactly 0 counts as that too), the mean of the
    non-zero ones (max_d if there is none), min(tol, mean), times rel_tol."""
    tols = [float(d) if d < max_d else 0 for d in dists]
    sum_tols, num_tols = 0.0, 0
    for t in tols:
        if t != 0:
            sum_tols += t
            num_tols += 1
    mean_tols = max_d
    if num_tols:
        mean_tols = sum_tols / num_tols
    out = []
    for t in tols:
        if t == 0:
            t = mean_tols
        out.append(min(t, mean_tols) * rel_tol)
    return out


def check_tolerances(min_tol, max_tol, rel_tol=0.25, poly_tick_dist=5):
    assert type(min_tol) == int and type(max_tol) == int, "min_tol and max_tol have to be ints"
    assert 0.0 < rel_tol <= 1.0, "rel_tol has to be in the range (0,1]"
    assert type(poly_tick_dist) == int, "poly_tick_dist has to be int"
    if not ((min_tol == -1 and max_tol == -1) or 1 <= min_tol <= max_tol):
        raise ValueError(
            f"unsupported tolerances min_tol={min_tol}, max_tol={max_tol}: use -1 / -1 (dynamic tolerances) or "
            f"1 <= min_tol <= max_tol; what the reference computes for other combinations is an accident of numpy "
            f"broadcasting or a division by zero and is not restated")


# ---- one file pair, prepared for the device ---------------------------------------------------------------------------

def _as_xy(poly):
    if hasattr(poly, "x_points"):
        return list(poly.x_points), list(poly.y_points)
    return list(poly[0]), list(poly[1])


class _Prepared:
    """Normed truth / reco polygons of one file pair in dict order, their article structure and the tolerance table."""

    def __init__(self, gt_dict, hy_dict, poly_tick_dist, dynamic):
        from .textblock import NormedPage
        self.dynamic = dynamic
        self.gt_ids = list(gt_dict)
        self.hy_ids = list(hy_dict)
        self.t_art = np.array([g for g, k in enumerate(self.gt_ids) for _ in gt_dict[k]], np.int64)
        self.r_art = np.array([a for a, k in enumerate(self.hy_ids) for _ in hy_dict[k]], np.int64)
        self.t_has_id = np.array([self.gt_ids[g] is not None for g in self.t_art], bool)
        self.r_has_id = np.array([self.hy_ids[a] is not None for a in self.r_art], bool)
        self.truth = NormedPage(geo.norm_poly_dists([_as_xy(p) for k in self.gt_ids for p in gt_dict[k]], poly_tick_dist))
        self.reco = NormedPage(geo.norm_poly_dists([_as_xy(p) for k in self.hy_ids for p in hy_dict[k]], poly_tick_dist))
        self.art_sizes = [len(hy_dict[k]) for k in self.hy_ids]
        self.tols = None

    def truth_subsets(self):
        """index arrays of the truth subsets whose tolerances are computed within the subset: all, with id, per article"""
        subs = [np.arange(self.truth.n), np.flatnonzero(self.t_has_id)]
        subs += [np.flatnonzero(self.t_art == g) for g, k in enumerate(self.gt_ids) if k is not None]
        return subs


def _subpage(page, idx):
    from .textblock import NormedPage
    sub = NormedPage.__new__(NormedPage)
    sub.polys = [page.polys[i] for i in idx]
    sub.n = len(idx)
    sub.boxes = np.ascontiguousarray(page.boxes[idx]).reshape(-1, 4)
    sub.orient = np.ascontiguousarray(page.orient[idx]).reshape(-1, 2)
    return sub


def _set_tolerances(preps, min_tol, max_tol, rel_tol, poly_tick_dist, device):
    """tols [n_truth][n_tols] per file pair.  Fixed ticks: the ticks.  Dynamic: one column per subset kind (all, with id,
    own article), 0 where the polygon is not in a subset of that kind; the interline distances of every subset of every
    file come from one asep_textblock_interline_dists call (each subset a "page")."""
    if min_tol >= 0:
        ticks = np.arange(min_tol, max_tol + 1).astype(np.float64)
        for p in preps:
            p.tols = np.tile(ticks, [p.truth.n, 1])
        return
    from . import textblock
    subsets = [(p, kind if kind < 2 else 2, idx) for p in preps for kind, idx in enumerate(p.truth_subsets()) if len(idx)]
    for p in preps:
        p.tols = np.zeros((p.truth.n, 3), np.float64)
    if not subsets:
        return
    dists = textblock.interline_distances([_subpage(p.truth, idx) for p, _, idx in subsets], poly_tick_dist, MAX_D, device)
    for (p, col, idx), d in zip(subsets, dists):
        p.tols[idx, col] = tols_from_distances(d.tolist(), MAX_D, rel_tol)


def _csr(pages):
    lens = [len(xs) for p in pages for xs, _ in p.polys]
    off = np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    pts = np.zeros((int(off[-1]), 2), np.int32)
    if len(lens):
        pts[:, 0] = np.concatenate([xs for p in pages for xs, _ in p.polys])
        pts[:, 1] = np.concatenate([ys for p in pages for _, ys in p.polys])
    boxes = np.ascontiguousarray(np.concatenate([p.boxes for p in pages]) if pages else np.zeros((0, 4), np.int32), np.int32)
    return off, pts, boxes


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return off


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class DeviceResult:
    """The sparse results of one file pair (indices local to the pair)."""
    __slots__ = ("pair_i", "pair_j", "pair_hits", "rec_j", "rec_a", "rec_hits", "truth_hits", "pair_hist", "rec_hist",
                 "truth_hist", "dmax")


def device_rel_hits(preps, want_hist=False, device=0):
    """asep_measure_run + asep_measure_fetch over the prepared file pairs (tolerances set): one DeviceResult per pair."""
    from . import _lib
    from .textblock import _handle
    lib, h = _handle(device)
    n_tols = preps[0].tols.shape[1] if preps else 1
    t_file_off = _offsets([p.truth.n for p in preps])
    r_file_off = _offsets([p.reco.n for p in preps])
    art_file_off = _offsets([len(p.art_sizes) for p in preps])
    art_off = _offsets([s for p in preps for s in p.art_sizes])
    art_has_id = np.array([k is not None for p in preps for k in p.hy_ids], np.int32)
    t_off, t_pts, t_box = _csr([p.truth for p in preps])
    r_off, r_pts, r_box = _csr([p.reco for p in preps])
    tols = np.ascontiguousarray(np.concatenate([p.tols for p in preps]) if preps else np.zeros((0, n_tols)), np.float64)
    dmax = int(math.floor(3.0 * float(tols.max()))) if tols.size else 0
    counts = np.zeros(2, np.int64)
    _lib.check(lib.asep_measure_run(h, len(preps), _ptr(t_file_off), _ptr(r_file_off), _ptr(t_off), _ptr(t_pts), _ptr(t_box),
                                    _ptr(r_off), _ptr(r_pts), _ptr(r_box), _ptr(art_file_off), _ptr(art_off),
                                    _ptr(art_has_id), n_tols, _ptr(tols), dmax, 1 if want_hist else 0, _ptr(counts)),
               "asep_measure_run")
    n_pairs, n_recs, n_truth = int(counts[0]), int(counts[1]), int(t_file_off[-1])
    pair_ij = np.zeros((n_pairs, 2), np.int32)
    pair_hits = np.zeros((n_pairs, n_tols), np.float64)
    rec_ja = np.zeros((n_recs, 2), np.int32)
    rec_hits = np.zeros((n_recs, n_tols), np.float64)
    truth_hits = np.zeros((n_truth, 2, n_tols), np.float64)
    hists = [np.zeros((n, dmax + 2), np.uint32) if want_hist else None for n in (n_pairs, n_recs, 2 * n_truth)]
    _lib.check(lib.asep_measure_fetch(h, _ptr(pair_ij), _ptr(pair_hits), _ptr(rec_ja), _ptr(rec_hits), _ptr(truth_hits),
                                      *[_ptr(x) for x in hists]), "asep_measure_fetch")
    # pairs are ordered by global reco index, records by global truth index: each file owns one slice
    p_lo = np.searchsorted(pair_ij[:, 0], r_file_off)
    c_lo = np.searchsorted(rec_ja[:, 0], t_file_off)
    out = []
    for k in range(len(preps)):
        r = DeviceResult()
        ps, cs, ts = slice(p_lo[k], p_lo[k + 1]), slice(c_lo[k], c_lo[k + 1]), slice(t_file_off[k], t_file_off[k + 1])
        r.pair_i = pair_ij[ps, 0].astype(np.int64) - int(r_file_off[k])
        r.pair_j = pair_ij[ps, 1].astype(np.int64) - int(t_file_off[k])
        r.pair_hits = pair_hits[ps]
        r.rec_j = rec_ja[cs, 0].astype(np.int64) - int(t_file_off[k])
        r.rec_a = rec_ja[cs, 1].astype(np.int64)
        r.rec_hits = rec_hits[cs]
        r.truth_hits = truth_hits[ts]
        r.pair_hist = hists[0][ps] if want_hist else None
        r.rec_hist = hists[1][cs] if want_hist else None
        r.truth_hist = hists[2].reshape(n_truth, 2, dmax + 2)[ts] if want_hist else None
        r.dmax = dmax
        out.append(r)
    return out


def last_kernel_us(which):
    """device time of the candidate count (0) / pair (1) / recall (2) kernel of this thread's last call, microseconds"""
    from . import _lib
    return float(_lib.load_library().asep_measure_last_kernel_us(which))


# ---- the jobs of one file pair over the sparse results -----------------------------------------------------------------

def precision_from_pairs(n_ticks, n_reco, rows, cols, hits):
    """eval_measure.py:108-123 per tick on the candidate entries hits[k] = rel_hits[:, rows[k], cols[k]]."""
    precision = np.zeros([n_ticks, n_reco])
    for t in range(n_ticks):
        v = hits[:, t]
        for k in greedy_alignment(rows, cols, v, inclusive=True):
            precision[t, rows[k]] = v[k]
    return precision


def _index_map(n, members):
    m = np.full(n, -1, np.int64)
    m[members] = np.arange(len(members))
    return m


def job_matrices(prep, res, truth_idx, reco_idx, kind, article=None):
    """The per-line precision [ticks, len(reco_idx)] and recall [ticks, len(truth_idx)] matrices of one job: ``kind`` 0
    all baselines, 1 baselines with an id, 2 one (GT article, HY article) pair with ``article`` the HY article index."""
    cols = slice(kind, kind + 1) if prep.dynamic else slice(None)
    n_ticks = 1 if prep.dynamic else prep.tols.shape[1]
    tmap, rmap = _index_map(prep.truth.n, truth_idx), _index_map(prep.reco.n, reco_idx)
    sel = (rmap[res.pair_i] >= 0) & (tmap[res.pair_j] >= 0)
    precision = precision_from_pairs(n_ticks, len(reco_idx), rmap[res.pair_i[sel]], tmap[res.pair_j[sel]],
                                     res.pair_hits[sel][:, cols])
    recall = np.zeros([n_ticks, len(truth_idx)])
    if kind < 2:
        recall[:, :] = res.truth_hits[truth_idx, kind][:, cols].T
    else:
        s = (res.rec_a == article) & (tmap[res.rec_j] >= 0)
        recall[:, tmap[res.rec_j[s]]] = res.rec_hits[s][:, cols].T
    return precision, recall


def prepare(pairs, min_tol, max_tol, rel_tol, poly_tick_dist, device=0):
    check_tolerances(min_tol, max_tol, rel_tol, poly_tick_dist)
    preps = [_Prepared(gt, hy, poly_tick_dist, min_tol < 0) for gt, hy in pairs]
    _set_tolerances(preps, min_tol, max_tol, rel_tol, poly_tick_dist, device)
    return preps


class BaselineMeasureEval(object):
    def __init__(self, min_tol=10, max_tol=30, rel_tol=0.25, poly_tick_dist=5, device=0):
        check_tolerances(min_tol, max_tol, rel_tol, poly_tick_dist)
        self.min_tol, self.max_tol = min_tol, max_tol
        self.max_tols = np.arange(min_tol, max_tol + 1)
        self.rel_tol = rel_tol
        self.poly_tick_dist = poly_tick_dist
        self.truth_line_tols = None
        self.device = device
        self.measure = BaselineMeasure()

    def calc_measure_for_page_baseline_polys(self, polys_truth, polys_reco, use_java_code=False):
        """BaselineMeasure stats of the truth and reco polygons (``Polygon``-like objects with x_points / y_points, or
        (xs, ys) pairs) of one page, added to ``self.measure``.  ``use_java_code`` is accepted with either value: the
        results are always those of the reference's Python path."""
        assert type(polys_truth) == list and type(polys_reco) == list, "polys_truth and polys_reco have to be lists"
        prep = prepare([({"a": polys_truth}, {"a": polys_reco})], self.min_tol, self.max_tol, self.rel_tol,
                       self.poly_tick_dist, self.device)[0]
        res = device_rel_hits([prep], device=self.device)[0]
        precision, recall = job_matrices(prep, res, np.arange(prep.truth.n), np.arange(prep.reco.n), 0)
        self.measure.add_per_dist_tol_tick_per_line_precision(precision)
        self.measure.add_per_dist_tol_tick_per_line_recall(recall)


def _page_rp(precision, recall):
    return _page_value(recall)[1], _page_value(precision)[1]


def baseline_detection(prep, res):
    """compute_baseline_detection_measure (run_measure.py:49-112) without its two printed lines."""
    out = []
    for kind, (t_idx, r_idx) in enumerate(((np.arange(prep.truth.n), np.arange(prep.reco.n)),
                                           (np.flatnonzero(prep.t_has_id), np.flatnonzero(prep.r_has_id)))):
        if len(t_idx) == 0:
            out += [None, None]
        elif len(r_idx) == 0:
            out += [0, 0]
        else:
            out += list(_page_rp(*job_matrices(prep, res, t_idx, r_idx, kind)))
    return tuple(out)


def article_matrices(prep, res):
    """r_matrix / p_matrix [GT articles with id, HY articles with id] before weighting (run_measure.py:190-220) and
    the block weighting factors.  Only (GT article, HY article) blocks that hold a candidate pair can be non-zero."""
    gt_arts = [g for g, k in enumerate(prep.gt_ids) if k is not None]
    hy_arts = [a for a, k in enumerate(prep.hy_ids) if k is not None]
    gpos, apos = {g: n for n, g in enumerate(gt_arts)}, {a: n for n, a in enumerate(hy_arts)}
    r_matrix = np.zeros((len(gt_arts), len(hy_arts)), dtype=float)
    p_matrix = np.zeros((len(gt_arts), len(hy_arts)), dtype=float)
    t_members = {g: np.flatnonzero(prep.t_art == g) for g in gt_arts}
    r_members = {a: np.flatnonzero(prep.r_art == a) for a in hy_arts}
    blocks = {(int(g), int(a)) for g, a in zip(prep.t_art[res.pair_j], prep.r_art[res.pair_i]) if g in gpos and a in apos}
    for g, a in sorted(blocks):
        r, p = _page_rp(*job_matrices(prep, res, t_members[g], r_members[a], 2, article=a))
        r_matrix[gpos[g], apos[a]] = r
        p_matrix[gpos[g], apos[a]] = p
    gt_w = [float(len(t_members[g])) for g in gt_arts]
    hy_w = [float(len(r_members[a])) for a in hy_arts]
    return r_matrix, p_matrix, gt_w, hy_w


def weight_matrices(r_matrix, p_matrix, gt_w, hy_w):
    """run_measure.py:224-232: rows of r by the share of GT baselines, columns of p by the share of HY baselines."""
    gt_weighting = np.asarray([1 / sum(gt_w) * x for x in gt_w], dtype=float)
    hy_weighting = np.asarray([1 / sum(hy_w) * x for x in hy_w], dtype=float)
    return r_matrix * np.expand_dims(gt_weighting, axis=1), p_matrix * hy_weighting


def evaluate(prep, res, log=print, matrices=None):
    """run_eval (run_measure.py:138-244) after the files have been read: its prints, early returns and three tuples.
    ``matrices(prep, res)`` may replace ``baseline_detection`` / ``article_matrices`` (the host tests feed recorded ones)."""
    bd = baseline_detection if matrices is None else matrices[0]
    am = article_matrices if matrices is None else matrices[1]
    log("{:<100s} {:>10d} {:<1s} {:>10d}".format("number of ground truth baselines / hypotheses baselines",
                                                 len(prep.t_art), "/", len(prep.r_art)))
    log("{:<100s} {:>10d} {:<1s} {:>10d}".format(
        "number of ground truth baselines with article ID's / hypotheses baselines with article ID's",
        int(prep.t_has_id.sum()), "/", int(prep.r_has_id.sum())))
    bd_r, bd_p, bd_r_wn, bd_p_wn = bd(prep, res)
    if bd_r is None:
        log("!! Ground truth Page XML has no baselines !!\n")
        return None, None, None
    if bd_r_wn is None:
        log("!! Ground truth Page XML has no article / block ID's !!\n")
        return (bd_r, bd_p, f_measure(recall=bd_r, precision=bd_p)), None, None
    bd_f = f_measure(recall=bd_r, precision=bd_p)
    bd_f_wn = f_measure(recall=bd_r_wn, precision=bd_p_wn)
    n_gt = sum(k is not None for k in prep.gt_ids)
    n_hy = sum(k is not None for k in prep.hy_ids)
    log("{:<100s} {:>10d} {:<1s} {:>10d}\n".format("number of ground truth articles / hypotheses articles", n_gt, "/", n_hy))
    if n_hy == 0:
        return (bd_r, bd_p, bd_f), (bd_r_wn, bd_p_wn, bd_f_wn), (0, 0, 0)
    r_matrix, p_matrix = weight_matrices(*am(prep, res))
    as_r, as_p = get_greedy_sum(r_matrix), get_greedy_sum(p_matrix)
    return (bd_r, bd_p, bd_f), (bd_r_wn, bd_p_wn, bd_f_wn), (as_r, as_p, f_measure(recall=as_r, precision=as_p))


def get_data_from_pagexml(path_to_pagexml):
    """run_measure.py:14-46: {article id (None for lines without one): [(xs, ys), ...]} over the text lines whose
    baseline holds more than one point, in document order."""
    from .page_xml import Page
    out = {}
    for article_id, lines in Page(path_to_pagexml).get_article_dict().items():
        for tl in lines:
            if len(tl.baseline) > 1:
                out.setdefault(article_id, []).append(([p[0] for p in tl.baseline], [p[1] for p in tl.baseline]))
    return out


def run_eval_dicts(pairs, min_tol=10, max_tol=30, rel_tol=0.25, poly_tick_dist=5, device=0):
    """The device part of run_eval for a batch of (gt_dict, hy_dict) pairs: [(prepared, DeviceResult)], one device
    round trip for the tolerances (dynamic mode) and one for the relative hits, whatever the number of pairs."""
    preps = prepare(pairs, min_tol, max_tol, rel_tol, poly_tick_dist, device)
    return list(zip(preps, device_rel_hits(preps, device=device)))


def run_eval(gt_file, hy_file, min_tol=10, max_tol=30, rel_tol=0.25, poly_tick_dist=5, log=print, device=0):
    """run_measure.py:138-244: the baseline detection measure over all baselines, over the baselines with an article
    id, and the article / block segmentation measure, each as (R, P, F) or None."""
    if not gt_file.endswith(".xml") or not hy_file.endswith(".xml"):
        log("!! Ground truth and hypotheses file have to be in Page XML format !!\n")
        return None, None, None
    pair = (get_data_from_pagexml(gt_file), get_data_from_pagexml(hy_file))
    prep, res = run_eval_dicts([pair], min_tol, max_tol, rel_tol, poly_tick_dist, device)[0]
    return evaluate(prep, res, log)
