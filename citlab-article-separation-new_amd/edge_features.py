"""The per-edge and per-pair part of ``feature_generation.py`` on the device (``asep_edge_features_run``): the separator flags of
every edge (``get_edge_separator_feature_bb`` / ``_line``), the convex hull of every edge's two regions (``get_edge_visual_region``)
and the pair bits of the confidence masking (``is_aligned_heading_separated`` / ``is_aligned_horizontally_separated``), for all
pages of a call at once.  Everything is integer geometry on int32 points, so the arrays equal the host functions' results exactly.

A page is anything with ``text_regions`` (objects with ``points`` and ``region_type``), ``separator_regions`` (``points`` and
``get_orientation()``) and ``edges`` ([E, 2] region indices); ``EdgePage`` is the plain form.  There is no CPU fallback: without a
GPU ``edge_features_device`` raises.  The ``line`` rule is pinned by this package's restatement of the reference only
(``feature_generation.get_edge_separator_feature_line``): the reference's own needs shapely.
"""
import ctypes as C
import json

import numpy as np

from . import _lib

# Most bytes of hull rows (edges x widest edge x 8) one engine call returns; the device holds twice that as scratch.  Beyond it the
# edges are split over several calls; a single edge whose row alone exceeds it is refused by the engine with the reason.
HULL_BYTE_BUDGET = 64 << 20

last_kernel_us = 0.0        # device time of the kernels of the last edge_features_device (all its engine calls)
last_launches = []          # [(kernel, blocks)] of that call, in launch order


class EdgePage:
    def __init__(self, text_regions, separator_regions, edges):
        self.text_regions = list(text_regions)
        self.separator_regions = list(separator_regions or [])
        self.edges = np.asarray(edges, dtype=np.int32).reshape(-1, 2)


def is_heading(text_region):
    return (getattr(text_region, "region_type", None) or "").lower() == "heading"


def orientation_code(separator_region):
    o = separator_region.get_orientation()
    return _lib.SEP_ORIENTATIONS.get(o, 3)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    np.cumsum(counts, out=off[1:])
    return off


def _pack_polygons(groups):
    """[[points of a polygon, ...] per page] -> (poly_off over pages, pt_off over polygons, int32 points [n, 2])"""
    polys = [np.asarray(pts, dtype=np.int32).reshape(-1, 2) for g in groups for pts in g]
    pts = np.concatenate(polys + [np.zeros((0, 2), np.int32)]).astype(np.int32, copy=False)
    return _offsets([len(g) for g in groups]), _offsets([len(p) for p in polys]), np.ascontiguousarray(pts)


def pack_pages(pages):
    """-> the engine's tables (include/asep_hip.h): int32 offsets and points (as ``np.asarray(points, dtype=np.int32)`` gives them),
    uint8 heading and orientation bytes, int32 edges within the page"""
    node_off, node_pt_off, node_pts = _pack_polygons([[r.points for r in p.text_regions] for p in pages])
    sep_off, sep_pt_off, sep_pts = _pack_polygons([[s.points for s in p.separator_regions] for p in pages])
    edges = [np.asarray(p.edges, dtype=np.int32).reshape(-1, 2) for p in pages]
    return {"n_pages": len(pages), "node_off": node_off, "node_pt_off": node_pt_off, "node_pts": node_pts,
            "node_heading": np.array([is_heading(r) for p in pages for r in p.text_regions], np.uint8),
            "sep_off": sep_off, "sep_pt_off": sep_pt_off, "sep_pts": sep_pts,
            "sep_orient": np.array([orientation_code(s) for p in pages for s in p.separator_regions], np.uint8),
            "edge_off": _offsets([len(e) for e in edges]),
            "edges": np.ascontiguousarray(np.concatenate(edges + [np.zeros((0, 2), np.int32)]).astype(np.int32, copy=False))}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _edge_points(t):
    """points of the two regions of every edge of the call together (the width of its hull row)"""
    n_pts = np.diff(t["node_pt_off"]).astype(np.int64)
    page = np.repeat(np.arange(t["n_pages"]), np.diff(t["edge_off"]))
    base = t["node_off"][:-1].astype(np.int64)[page]
    return n_pts[base + t["edges"][:, 0]] + n_pts[base + t["edges"][:, 1]]


def hull_chunks(widths, budget):
    """consecutive edge ranges [e0, e1) whose hull rows (edges x widest x 8 bytes) stay within ``budget``; an edge that does not fit
    alone gets a range of its own (the engine refuses it with the reason)"""
    n = len(widths)
    if n == 0 or n * int(widths.max()) * 8 <= budget:
        return [(0, n)]
    chunks, e0, widest = [], 0, 0
    for e in range(n):
        w = max(widest, int(widths[e]))
        if e > e0 and (e - e0 + 1) * w * 8 > budget:
            chunks.append((e0, e))
            e0, w = e, int(widths[e])
        widest = w
    chunks.append((e0, n))
    return chunks


def run_tables(t, rule=0, flags=True, hulls=False, pair_bits=False, edge_range=None, hull_budget=None, hull_cap=None, device=0):
    """One ``asep_edge_features_run`` over packed tables, optionally over the edges ``edge_range`` = (e0, e1) of the call alone.
    ``hull_cap``: the width of the hull rows, by default the widest edge of the call.
    -> (flags uint8 [E, 2] | None, hull int32 [E, cap, 2] | None, hull_n int32 [E] | None, pairs uint8 [sum N_k^2] | None)"""
    from .textblock import _handle
    lib, h = _handle(device)            # raises without the library or a GPU
    edge_off, edges = t["edge_off"], t["edges"]
    if edge_range is not None:
        e0, e1 = edge_range
        edge_off = (np.clip(edge_off, e0, e1) - e0).astype(np.int32)
        edges = np.ascontiguousarray(edges[e0:e1])
    n_edges = int(edge_off[-1])
    out_flags = np.zeros((n_edges, 2), np.uint8) if flags else None
    out_hull = out_n = None
    cap = 0
    if hulls:
        if hull_cap is None:
            hull_cap = int(_edge_points(dict(t, edge_off=edge_off, edges=edges)).max()) if n_edges else 0
        cap = int(hull_cap)
        out_hull = np.zeros((n_edges, cap, 2), np.int32)
        out_n = np.zeros(n_edges, np.int32)
    out_pairs = None
    if pair_bits:
        n = np.diff(t["node_off"]).astype(np.int64)
        out_pairs = np.zeros(int((n * n).sum()), np.uint8)
    hull_ptr = (out_hull.ctypes.data_as(C.c_void_p) if out_hull.size else C.c_void_p(out_n.ctypes.data)) if hulls else None
    rc = lib.asep_edge_features_run(
        h, t["n_pages"], t["node_off"].ctypes.data_as(C.c_void_p), _ptr(t["node_pt_off"]), _ptr(t["node_pts"]),
        _ptr(t["node_heading"]), t["sep_off"].ctypes.data_as(C.c_void_p), _ptr(t["sep_pt_off"]), _ptr(t["sep_pts"]),
        _ptr(t["sep_orient"]), edge_off.ctypes.data_as(C.c_void_p), _ptr(edges), int(rule),
        out_flags.ctypes.data_as(C.c_void_p) if flags else None, hull_ptr,
        out_n.ctypes.data_as(C.c_void_p) if hulls else None, cap,
        int(HULL_BYTE_BUDGET if hull_budget is None else hull_budget),
        out_pairs.ctypes.data_as(C.c_void_p) if pair_bits else None)
    _lib.check(rc, "asep_edge_features_run")
    return out_flags, out_hull, out_n, out_pairs


def launches():
    """[(kernel, blocks)] of the calling thread's last engine call"""
    lib = _lib.load_library()
    buf = C.create_string_buffer(1 << 12)
    _lib.check(lib.asep_edge_features_last_launches(buf, len(buf)), "asep_edge_features_last_launches")
    return [(r["kernel"], r["blocks"]) for r in json.loads(buf.value.decode())]


def edge_features_device(pages, rule="bb", hulls=False, pair_bits=False, device=0):
    """All pages in one engine call (more only when the hull rows exceed ``HULL_BYTE_BUDGET``).  -> one dict per page:
    ``flags`` uint8 [E, 2] = (horizontally, vertically separated) under ``rule`` ('bb' | 'line'); with ``hulls``: ``hull`` int32
    [E, widest hull of the page, 2], zero behind ``hull_n`` int32 [E] (``convex_hull`` of the two regions' points); with
    ``pair_bits``: ``pair_bits`` uint8 [N, N], bit 0 heading separated, bit 1 horizontally separated (diagonal 0)"""
    global last_kernel_us, last_launches
    if rule not in _lib.EDGE_RULES:
        raise ValueError(f"separator rule '{rule}': the engine computes {', '.join(_lib.EDGE_RULES)}")
    lib = _lib.load_library()
    t = pack_pages(pages)
    last_kernel_us, last_launches = 0.0, []

    def run(**kw):
        global last_kernel_us
        res = run_tables(t, _lib.EDGE_RULES[rule], device=device, **kw)
        last_kernel_us += float(lib.asep_edge_features_last_kernel_us())
        last_launches.extend(launches())
        return res

    n_edges = int(t["edge_off"][-1])
    chunks = hull_chunks(_edge_points(t), HULL_BYTE_BUDGET) if hulls else [(0, n_edges)]
    if len(chunks) == 1:
        flags, hull, hull_n, pairs = run(hulls=hulls, pair_bits=pair_bits)
    else:
        flags, _, _, pairs = run(pair_bits=pair_bits)
        parts = [run(flags=False, hulls=True, edge_range=c)[1:3] for c in chunks]
        hull_n = np.concatenate([n for _, n in parts])
        hull = np.zeros((n_edges, int(hull_n.max()), 2), np.int32)
        for (e0, e1), (rows, _) in zip(chunks, parts):
            w = min(rows.shape[1], hull.shape[1])
            hull[e0:e1, :w] = rows[:, :w]
    out = []
    n = np.diff(t["node_off"]).astype(np.int64)
    pair_off = np.concatenate([[0], np.cumsum(n * n)])
    for k in range(len(pages)):
        e0, e1 = int(t["edge_off"][k]), int(t["edge_off"][k + 1])
        res = {"flags": flags[e0:e1]}
        if hulls:
            width = int(hull_n[e0:e1].max()) if e1 > e0 else 0
            res["hull"] = np.ascontiguousarray(hull[e0:e1, :width])
            res["hull_n"] = hull_n[e0:e1]
        if pair_bits:
            res["pair_bits"] = pairs[pair_off[k]:pair_off[k + 1]].reshape(int(n[k]), int(n[k]))
        out.append(res)
    return out


def mask_from_pair_bits(bits, shape, mask_heading=True, mask_horizontal=True):
    """``mask_horizontally_separated_confs``'s int32 mask of ``shape`` from a page's pair bits: 0 where a selected bit is set"""
    sel = (1 if mask_heading else 0) | (2 if mask_horizontal else 0)
    masked = np.ones(shape, dtype=np.int32)
    n = bits.shape[0]
    masked[:n, :n][(bits & sel) != 0] = 0
    return masked
