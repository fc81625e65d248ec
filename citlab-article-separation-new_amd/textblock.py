"""Text block detection (the reference's README "Text Block Detection" stage) on the GPU.

    interline_distances      dbscan_baselines.py:35-110 (use_java_code=False)     -> asep_textblock_interline_dists
    neighbour_lists          dbscan_baselines.py:253-307 region_query, all rows    -> asep_textblock_neighbours
    DBSCAN labels            dbscan_baselines.py:113-251, 309-333                  (host, over the device neighbour lists)
    text regions             textregion_generation.py:17-172                       (host alpha shapes; device_regions=True:
                                                                                    host triangulation -> asep_alpha_shapes;
                                                                                    device_triangulation=True as well:
                                                                                    asep_alpha_shapes_points, no scipy)

Every function takes a BATCH of pages (one list of polygons per page) so that one kernel launch serves all of them.
The results are those of the reference's Python path; the Java class the reference can call instead
(``use_java_code=True``) is not used.  No CPU fallback: without the HIP library every device function
raises ``AsepError``.

``device_triangulation=True`` promises the same polygon as the host function, not the same bytes.  The host function starts its
ring at the first boundary edge in Qhull's triangle order, which nobody can restate; the device triangulates in its own order.  So
that path gives the same cyclic vertex sequence as ``textblock_geometry.alpha_shape`` after the same number of alpha retries,
written in a canonical form (``canonical_ring``): from the vertex with the smallest (y, x), in the direction of positive shoelace
area sum(x_i * y_i+1 - x_i+1 * y_i) (counter-clockwise with y up, clockwise as a page is displayed), the first vertex repeated at
the end.  Cocircular points may be split differently than Qhull splits them; the triangles of such a cell share one circumcircle
and are accepted or refused together, so the boundary can differ only where a circumradius lies within rounding of an alpha that
is tried (supposed from the geometry; tests/test_delaunay_host.py checks it on its inputs).  Articles the device does not
triangulate (a bounding box over ``delaunay_max_extent()`` pixels, fewer than 3 distinct points, all points on one line) and
articles of more than ``DEVICE_TRIANGULATION_MAX_POINTS`` points go through the host function one by one.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from . import textblock_geometry as geo

_handles = {}


def _handle(device=0):
    lib = _lib.init_device(device)
    if device not in _handles:
        h = lib.asep_post_create()
        if not h:
            raise _lib.AsepError("asep_post_create failed: " + _lib.last_error())
        _handles[device] = h
    return lib, _handles[device]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class NormedPage:
    """The normed polygons of one page with what the distance kernel reads: CSR points, boxes and (cos, sin)."""

    def __init__(self, normed):
        normed = [(np.asarray(xs, np.int64), np.asarray(ys, np.int64)) for xs, ys in normed]
        self.polys = normed
        self.n = len(normed)
        if any(len(xs) == 0 for xs, _ in normed):
            # the reference indexes x_points[0] of every normed polygon (an IndexError there)
            raise ValueError("a baseline whose bounding box exceeds 100000 px has no normed points")
        self.boxes = np.array([geo.bounds(xs, ys) for xs, ys in normed], np.int32).reshape(-1, 4)
        self.angles = np.array([geo.calc_reg_line_angle(xs, ys) for xs, ys in normed], np.float64)
        self.orient = np.array([(math.cos(a), math.sin(a)) for a in self.angles], np.float64).reshape(-1, 2)


def normed_pages(pages_polys, des_dist):
    return [NormedPage(geo.norm_poly_dists(polys, des_dist)) for polys in pages_polys]


def normed_pages_or_errors(pages_polys, des_dist):
    """normed_pages, with the exception of a page that cannot be normed (a baseline box over 100000 px, malformed
    points) in that page's place: one bad page of a batch fails alone, as a file of the reference's per-file runs does."""
    out = []
    for polys in pages_polys:
        try:
            out.append(NormedPage(geo.norm_poly_dists(polys, des_dist)))
        except Exception as e:      # noqa: BLE001 (reported per file by the command lines)
            out.append(e)
    return out


def interline_distances_or_errors(pages, des_dist=5, max_d=500, device=0):
    """interline_distances over the NormedPage entries of ``pages`` (one launch); exceptions are passed through."""
    good = [p for p in pages if not isinstance(p, Exception)]
    dists = iter(interline_distances(good, des_dist, max_d, device))
    return [p if isinstance(p, Exception) else next(dists) for p in pages]


def interline_distances(pages, des_dist=5, max_d=500, device=0):
    """``pages``: list of NormedPage.  Returns one float64 array of interline distances per page (one launch)."""
    lib, h = _handle(device)
    page_off = np.zeros(len(pages) + 1, np.int32)
    page_off[1:] = np.cumsum([p.n for p in pages])
    n_polys = int(page_off[-1])
    lens = [len(xs) for p in pages for xs, _ in p.polys]
    poly_off = np.zeros(n_polys + 1, np.int32)
    poly_off[1:] = np.cumsum(lens)
    pts = np.zeros((int(poly_off[-1]), 2), np.int32)
    if n_polys:
        pts[:, 0] = np.concatenate([xs for p in pages for xs, _ in p.polys])
        pts[:, 1] = np.concatenate([ys for p in pages for _, ys in p.polys])
    boxes = np.ascontiguousarray(np.concatenate([p.boxes for p in pages]) if pages else np.zeros((0, 4), np.int32))
    orient = np.ascontiguousarray(np.concatenate([p.orient for p in pages]) if pages else np.zeros((0, 2)))
    out = np.zeros(n_polys, np.float64)
    _lib.check(lib.asep_textblock_interline_dists(h, len(pages), _ptr(page_off), _ptr(poly_off), _ptr(pts), _ptr(boxes),
                                                  _ptr(orient), float(des_dist), float(max_d), _ptr(out)),
               "asep_textblock_interline_dists")
    return [out[page_off[k]:page_off[k + 1]] for k in range(len(pages))]


def neighbour_lists(pages, dists, avgs, fac=1.25, device=0):
    """region_query of every polygon of every page (one launch): per page a list of index-ordered neighbour lists."""
    lib, h = _handle(device)
    page_off = np.zeros(len(pages) + 1, np.int32)
    page_off[1:] = np.cumsum([p.n for p in pages])
    words = int(lib.asep_textblock_neighbour_words(len(pages), _ptr(page_off)))
    bits = np.zeros(max(words, 1), np.uint32)
    boxes = np.ascontiguousarray(np.concatenate([p.boxes for p in pages]) if pages else np.zeros((0, 4), np.int32))
    d = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64) for x in dists]) if pages else np.zeros(0))
    av = np.asarray(avgs, np.float64)
    _lib.check(lib.asep_textblock_neighbours(h, len(pages), _ptr(page_off), _ptr(boxes), _ptr(d), _ptr(av), float(fac),
                                             _ptr(bits), words), "asep_textblock_neighbours")
    out, off = [], 0
    for p in pages:
        n = p.n
        w = (n + 31) // 32
        m = np.unpackbits(bits[off:off + n * w].view(np.uint8), bitorder="little").reshape(n, w * 32)[:, :n]
        out.append([np.flatnonzero(row).tolist() for row in m])
        off += n * w
    return out


def last_kernel_us(which):
    """device time of the last distance (0) / neighbour (1) kernel of this thread, microseconds"""
    return float(_lib.load_library().asep_textblock_last_kernel_us(which))


# ---- DBSCAN (host) ----------------------------------------------------------------------------------------------------

def average_positive(dists, eps=0.0):
    """``1 / (len + eps) * sum`` over the positive distances (dbscan_baselines.py:135, 151, 160)."""
    al = [float(v) for v in dists if v > 0]
    return 1 / (len(al) + eps) * sum(al) if eps else 1 / len(al) * sum(al)


def dbscan_prepare(pages_polys, des_dist=5, max_d=500, target_average_interline_distance=50, device=0):
    """DBSCANBaselines.__init__ (dbscan_baselines.py:113-172) for a batch of pages: two device passes over all pages.
    Returns per page a dict with the normed polygons (a NormedPage), the distances, avg and the first pass, or the
    exception that stopped that page."""
    first = normed_pages_or_errors(pages_polys, des_dist)
    d1 = interline_distances_or_errors(first, des_dist, max_d, device)
    out = [None] * len(pages_polys)
    rescale = []
    for k, polys in enumerate(pages_polys):
        if isinstance(first[k], Exception):
            out[k] = first[k]
            continue
        al = [v for v in d1[k].tolist() if v > 0]
        rec = {"first": first[k], "dists1": d1[k]}
        if target_average_interline_distance > 0 and len(al) > 0:
            avg1 = 1 / len(al) * sum(al)
            rec["avg1"] = avg1
            rec["scale_fac"] = target_average_interline_distance / avg1
            rescale.append(k)
        else:
            rec["normed"], rec["dists"] = first[k], d1[k]
            rec["avg"] = 1 / (len(al) + 1e-8) * sum(al)
        out[k] = rec
    if rescale:
        second = normed_pages_or_errors([geo.scale_polygons(pages_polys[k], out[k]["scale_fac"]) for k in rescale],
                                        des_dist)
        d2 = interline_distances_or_errors(second, des_dist, max_d, device)
        for j, k in enumerate(rescale):
            if isinstance(second[j], Exception):
                out[k] = second[j]
                continue
            al = [v for v in d2[j].tolist() if v > 0]
            out[k]["normed"], out[k]["dists"] = second[j], d2[j]
            out[k]["avg"] = 1 / (len(al) + 1e-8) * sum(al)
    return out


def dbscan_labels(neighbours, min_polygons_for_cluster=2):
    """clustering_polygons + grow_cluster (dbscan_baselines.py:185-251): the FIFO of neighbour indices may hold duplicates."""
    labels = [0] * len(neighbours)
    label = 0
    for idx in range(len(neighbours)):
        if labels[idx] != 0:
            continue
        queue = list(neighbours[idx])
        if len(queue) < min_polygons_for_cluster:
            labels[idx] = -1
            continue
        label += 1
        labels[idx] = label
        i = 0
        while i < len(queue):
            k = queue[i]
            if labels[k] == -1:
                labels[k] = label
            elif labels[k] == 0:
                labels[k] = label
                nxt = neighbours[k]
                if len(nxt) >= min_polygons_for_cluster:
                    queue += nxt
            i += 1
    return labels


def cluster_of_polygons(labels, min_polygons_for_article=1):
    """get_cluster_of_polygons (dbscan_baselines.py:309-333).  Returns (labels, number of articles incl. noise)."""
    labels = list(labels)
    if min_polygons_for_article == 1:
        noise_id = max(labels) + 1                     # (a ValueError on a page without baselines, as in the reference)
        for index, lab in enumerate(labels):
            if lab == -1:
                labels[index] = noise_id
                noise_id += 1
    else:
        counts = {}
        for lab in labels:
            counts[lab] = counts.get(lab, 0) + 1
        small = {lab for lab, c in counts.items() if c < min_polygons_for_article and lab != -1}
        labels = [-1 if x in small else x for x in labels]
    return labels, len(set(labels))


def cluster_baselines(pages_polys, min_polygons_for_cluster=2, min_polygons_for_article=1, rectangle_interline_factor=1.25,
                      des_dist=5, max_d=500, target_average_interline_distance=50, device=0):
    """baseline_clustering.py:66-99 cluster_baselines_dbscan for a batch of pages: per page (labels, n_articles) or the
    exception that stops that page (the reference's for a page without baselines, or one from norming)."""
    prep = dbscan_prepare(pages_polys, des_dist, max_d, target_average_interline_distance, device)
    good = [r for r in prep if not isinstance(r, Exception)]
    neigh = iter(neighbour_lists([r["normed"] for r in good], [r["dists"] for r in good], [r["avg"] for r in good],
                                 rectangle_interline_factor, device))
    out = []
    for r in prep:
        if isinstance(r, Exception):
            out.append(r)
            continue
        labels = dbscan_labels(next(neigh), min_polygons_for_cluster)
        try:
            out.append(cluster_of_polygons(labels, min_polygons_for_article))
        except ValueError as e:
            out.append(e)
    return out


# ---- text regions (host) ----------------------------------------------------------------------------------------------

def shifted_outline(xs, ys, dist):
    """textregion_generation.py:59-66 / 141-148: the normed points and a copy shifted right by 1 and up by
    max(int(0.95 * dist), 1); returns the shifted x / y lists."""
    y_shift = max(int(0.95 * float(dist)), 1)
    return [int(x) + 1 for x in xs], [int(y) - y_shift for y in ys]


def synthetic_coords(xs, ys, dist):
    """textregion_generation.py:56-72: the surrounding polygon of a line without Coords."""
    xsh, ysh = shifted_outline(xs, ys, dist)
    return list(zip([int(x) for x in xs] + xsh[::-1], [int(y) for y in ys] + ysh[::-1]))


def create_text_regions(art_lines, line_geom, alpha=75, log=print, device_regions=False, device=0, device_triangulation=False):
    """textregion_generation.py:129-172.  ``art_lines``: {article id or None: [line id, ...]} in the page's order;
    ``line_geom``: {line id: ((xs, ys) normed polygon, interline distance)}.  Returns
    [("tr_<n>", boundary points, [line id, ...], n), ...].  ``device_regions``: the alpha shapes behind the
    triangulations come from one engine call (create_text_regions_pages), the result and the logged lines are the same.
    ``device_triangulation`` (needs ``device_regions``): the triangulations come from that call too; the same polygons in
    the canonical form of ``canonical_ring`` (module docstring), the same logged lines."""
    if device_triangulation and not device_regions:
        raise ValueError("device_triangulation needs device_regions")
    if device_regions:
        res = create_text_regions_pages([(art_lines, line_geom)], alpha, [log], device,
                                        device_triangulation=device_triangulation)[0]
        if isinstance(res, Exception):
            raise res
        return res
    regions = []
    counter = 0

    def outline(lid):
        (xs, ys), d = line_geom[lid]
        xsh, ysh = shifted_outline(xs, ys, d)
        return list(zip([int(x) for x in xs] + xsh, [int(y) for y in ys] + ysh))

    for article_id, lines in art_lines.items():
        if article_id is None:
            for lid in lines:
                if lid in line_geom:
                    bp = alpha_shape_int(outline(lid), alpha, log)
                    regions.append(("tr_" + str(counter), bp, [lid], counter))
                    counter += 1
        else:
            pts, members = [], []
            for lid in lines:
                if lid in line_geom:
                    members.append(lid)
                    pts += outline(lid)
            if not pts:
                raise IndexError(f"article {article_id} has no line with a baseline")   # (the reference: list index out of range)
            bp = alpha_shape_int(pts, alpha, log)
            regions.append(("tr_" + str(counter), bp, members, counter))
            counter += 1
    return regions


def alpha_shape_int(pts, alpha, log=print):
    return [[int(j) for j in i] for i in geo.alpha_shape(np.array(pts), alpha, log)]


# ---- text regions (device alpha shapes behind the host triangulation) -------------------------------------------------

def triangulate(points):
    """scipy's Delaunay of an (n, 2) integer array, as textblock_geometry.alpha_shape calls it: (points, simplices,
    neighbors).  Its triangle order decides the boundary's first edge, so the engine takes it as it is."""
    from scipy.spatial import Delaunay
    points = np.asarray(points)
    tri = Delaunay(points)
    return points, np.ascontiguousarray(tri.simplices, np.int32), np.ascontiguousarray(tri.neighbors, np.int32)


def alpha_shapes_device(pages, max_retries=None, device=0, debug=False):
    """One asep_alpha_shapes call.  ``pages``: per page a list of articles (points (n, 2) int, simplices, neighbors,
    alpha0) as ``triangulate`` gives them.  Returns per page a list of (ring: point indices in the reference's order
    without the repeated first one, retries, failed); with ``debug`` each entry also holds the circumradii and the
    boundary half-edge mask of the article's last round."""
    import sys
    lib, h = _handle(device)
    arts = [a for pg in pages for a in pg]
    art_off = np.zeros(len(pages) + 1, np.int32)
    art_off[1:] = np.cumsum([len(pg) for pg in pages])
    pt_off = np.zeros(len(arts) + 1, np.int64)
    tri_off = np.zeros(len(arts) + 1, np.int64)
    pt_off[1:] = np.cumsum([len(a[0]) for a in arts])
    tri_off[1:] = np.cumsum([len(a[1]) for a in arts])
    if pt_off[-1] > np.iinfo(np.int32).max or 3 * tri_off[-1] > np.iinfo(np.int32).max:
        raise ValueError(f"alpha_shapes_device: {pt_off[-1]} points / {tri_off[-1]} triangles exceed one call")
    pt_off, tri_off = pt_off.astype(np.int32), tri_off.astype(np.int32)
    n_pts, n_tri = int(pt_off[-1]), int(tri_off[-1])
    pts = np.zeros((max(n_pts, 1), 2), np.int32)
    simp = np.zeros((max(n_tri, 1), 3), np.int32)
    neigh = np.zeros((max(n_tri, 1), 3), np.int32)
    for k, (p, s, nb, _) in enumerate(arts):
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != 2 or (p.size and (p.min() < -2 ** 31 or p.max() >= 2 ** 31)):
            raise ValueError(f"alpha_shapes_device: article {k} needs (n, 2) points within int32")
        pts[pt_off[k]:pt_off[k + 1]] = p
        simp[tri_off[k]:tri_off[k + 1]] = s
        neigh[tri_off[k]:tri_off[k + 1]] = nb
    alpha0 = np.array([float(a[3]) for a in arts] + [0.0], np.float64)
    ring = np.zeros(max(n_pts, 1), np.int32)
    res = np.zeros((3, max(len(arts), 1)), np.int32)
    circ = np.zeros(max(n_tri, 1), np.float64) if debug else None
    mask = np.zeros(max(n_tri, 1), np.uint8) if debug else None
    _lib.check(lib.asep_alpha_shapes(h, len(pages), _ptr(art_off), _ptr(pt_off), _ptr(tri_off), _ptr(pts), _ptr(simp), _ptr(neigh),
                                     _ptr(alpha0), int(sys.getrecursionlimit() if max_retries is None else max_retries),
                                     _ptr(ring), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]),
                                     _ptr(circ) if debug else None, _ptr(mask) if debug else None), "asep_alpha_shapes")
    out, k = [], 0
    for pg in pages:
        rows = []
        for _ in pg:
            row = (ring[pt_off[k]:pt_off[k] + res[0, k]].copy(), int(res[1, k]), bool(res[2, k]))
            if debug:
                row += (circ[tri_off[k]:tri_off[k + 1]].copy(), mask[tri_off[k]:tri_off[k + 1]].copy())
            rows.append(row)
            k += 1
        out.append(rows)
    return out


def last_alpha_shape_kernel_us(which):
    """device time of the last circumradius (0) / boundary (1) kernel of this thread, microseconds"""
    return float(_lib.load_library().asep_alpha_shapes_last_kernel_us(which))


RETRY_LINE = "alpha value not suitable -> is increased"


def _region_jobs(art_lines, line_geom, alpha):
    """The point sets create_text_regions hands to alpha_shape, in its order: ([(points array or the exception its
    triangulation raises, members), ...], the exception that ends the page behind them or None)."""
    jobs = []

    def outline(lid):
        (xs, ys), d = line_geom[lid]
        xsh, ysh = shifted_outline(xs, ys, d)
        return list(zip([int(x) for x in xs] + xsh, [int(y) for y in ys] + ysh))

    try:
        for article_id, lines in art_lines.items():
            if article_id is None:
                for lid in lines:
                    if lid in line_geom:
                        jobs.append((np.array(outline(lid)), [lid]))
            else:
                pts, members = [], []
                for lid in lines:
                    if lid in line_geom:
                        members.append(lid)
                        pts += outline(lid)
                if not pts:
                    raise IndexError(f"article {article_id} has no line with a baseline")
                jobs.append((np.array(pts), members))
    except Exception as e:      # noqa: BLE001 (the host path meets it after the regions in front of it)
        return jobs, e
    return jobs, None


def _triangulate_or_error(points):
    if points.shape[0] <= 3:
        return None                                   # util.py:620: returned as they are
    try:
        return triangulate(points)
    except Exception as e:      # noqa: BLE001 (Qhull's refusal of e.g. collinear points, raised where the host path raises it)
        return e


def create_text_regions_pages(pages, alpha=75, logs=None, device=0, pool=None, device_triangulation=False):
    """create_text_regions for a group of pages with ONE engine call: ``pages`` = [(art_lines, line_geom), ...].
    The host triangulates every article once (``pool.map`` when a thread pool is given); the circumradii, the boundary
    edges, the walk and the alpha * 1.2 retries run on the device.  Returns per page the regions or the exception the
    host path raises for it; ``logs[k]`` receives the page's retry lines, one per retry, in the host's order.
    ``device_triangulation``: the point lists go up once and the engine triangulates them too (no scipy); rings in the
    canonical form, articles the device flags through the host function (module docstring)."""
    import sys
    logs = logs or [print] * len(pages)
    max_retries = sys.getrecursionlimit()
    plans = [_region_jobs(art, geom, alpha) for art, geom in pages]
    if device_triangulation:
        return _regions_from_points(plans, alpha, logs, max_retries, device)
    flat = [pts for jobs, _ in plans for pts, _ in jobs]
    tris = iter((pool.map if pool is not None else lambda f, xs: list(map(f, xs)))(_triangulate_or_error, flat))
    tris = [[next(tris) for _ in jobs] for jobs, _ in plans]
    dev_pages = []
    for tri in tris:
        # (behind an article that ends the page the host path computes nothing more)
        stop = next((i for i, t in enumerate(tri) if isinstance(t, Exception)), len(tri))
        dev_pages.append([t + (alpha,) for t in tri[:stop] if t is not None] if alpha > 0 else [])
    rings = alpha_shapes_device(dev_pages, max_retries, device) if any(dev_pages) else [[] for _ in pages]
    out = []
    for (jobs, end), tri, got, log in zip(plans, tris, rings, logs):
        got = iter(got)
        regions = []
        try:
            for counter, ((points, members), t) in enumerate(zip(jobs, tri)):
                assert alpha > 0, "alpha value has to be greater than zero"
                if isinstance(t, Exception):
                    raise t
                if t is None:
                    bp = points.tolist()
                else:
                    ring, retries, failed = next(got)
                    for _ in range(retries):
                        log(RETRY_LINE)
                    if failed:
                        raise RecursionError(f"alpha_shape: no single boundary after {retries} increases of alpha")
                    bp = points[ring].tolist()
                bp.append(bp[0])
                regions.append(("tr_" + str(counter), [[int(j) for j in i] for i in bp], members, counter))
            if end is not None:
                raise end
            out.append(regions)
        except Exception as e:      # noqa: BLE001 (the page's error, as the host path raises it)
            out.append(e)
    return out


# ---- text regions (device triangulation and alpha shapes) --------------------------------------------------------------

def canonical_ring(ring):
    """A closed ring [[x, y], ...] (first vertex repeated at the end) in the canonical form of the device triangulation path:
    the same cycle from the vertex with the smallest (y, x), in the direction of positive shoelace area."""
    pts = [[int(x), int(y)] for x, y in ring[:-1]]
    n = len(pts)
    area2 = sum(pts[i][0] * pts[(i + 1) % n][1] - pts[(i + 1) % n][0] * pts[i][1] for i in range(n))
    if area2 < 0:
        pts.reverse()
    k = min(range(n), key=lambda i: (pts[i][1], pts[i][0]))
    pts = pts[k:] + pts[:k]
    return pts + [list(pts[0])]


def delaunay_lds_points():
    """the largest article (in points) the device triangulates in LDS"""
    return int(_lib.load_library().asep_delaunay_lds_points())


def delaunay_max_extent():
    """the largest bounding-box extent (max - min, per axis) of an article the device triangulates"""
    return int(_lib.load_library().asep_delaunay_max_extent())


def last_delaunay_kernel_us():
    """device time of the last triangulation kernel of this thread, microseconds"""
    return float(_lib.load_library().asep_delaunay_last_kernel_us())


def _packed_points(fn, arts):
    """(pt_off int32 [n + 1], points int32 (max(sum, 1), 2)) of a list of (n, 2) integer arrays"""
    pt_off = np.zeros(len(arts) + 1, np.int64)
    pt_off[1:] = np.cumsum([len(a) for a in arts])
    if pt_off[-1] > np.iinfo(np.int32).max // 20:
        raise ValueError(f"{fn}: {pt_off[-1]} points exceed one call")
    pts = np.zeros((max(int(pt_off[-1]), 1), 2), np.int32)
    for k, p in enumerate(arts):
        p = np.asarray(p)
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer) \
                or (p.size and (p.min() < -2 ** 31 or p.max() >= 2 ** 31)):
            raise ValueError(f"{fn}: article {k} needs (n, 2) integer points within int32")
        pts[pt_off[k]:pt_off[k + 1]] = p
    return pt_off.astype(np.int32), pts


def delaunay_device(arts, device=0):
    """One asep_delaunay call.  ``arts``: a list of (n, 2) integer arrays.  Returns per article (simplices (T, 3) int32,
    neighbors (T, 3) int32, status): scipy.spatial.Delaunay's two tables, or no triangles and a status other than 0."""
    lib, h = _handle(device)
    pt_off, pts = _packed_points("delaunay_device", arts)
    cap_off = (2 * pt_off).astype(np.int32)
    cap = int(cap_off[-1])
    simp = np.zeros((max(cap, 1), 3), np.int32)
    neigh = np.zeros((max(cap, 1), 3), np.int32)
    res = np.zeros((2, max(len(arts), 1)), np.int32)
    _lib.check(lib.asep_delaunay(h, len(arts), _ptr(pt_off), _ptr(pts), _ptr(cap_off), _ptr(simp), _ptr(neigh), _ptr(res[0]),
                                 _ptr(res[1])), "asep_delaunay")
    return [(simp[cap_off[k]:cap_off[k] + res[0, k]].copy(), neigh[cap_off[k]:cap_off[k] + res[0, k]].copy(), int(res[1, k]))
            for k in range(len(arts))]


def alpha_shapes_points_device(pages, max_retries=None, device=0):
    """One asep_alpha_shapes_points call.  ``pages``: per page a list of articles (points (n, 2) int, alpha0).  Returns per
    page a list of (ring: point indices of the boundary cycle without the repeated first one, from the first boundary edge of
    the device's triangle order; retries; failed; status of the triangulation)."""
    import sys
    lib, h = _handle(device)
    arts = [a for pg in pages for a in pg]
    art_off = np.zeros(len(pages) + 1, np.int32)
    art_off[1:] = np.cumsum([len(pg) for pg in pages])
    pt_off, pts = _packed_points("alpha_shapes_points_device", [a[0] for a in arts])
    alpha0 = np.array([float(a[1]) for a in arts] + [0.0], np.float64)
    ring = np.zeros(max(int(pt_off[-1]), 1), np.int32)
    res = np.zeros((4, max(len(arts), 1)), np.int32)
    _lib.check(lib.asep_alpha_shapes_points(h, len(pages), _ptr(art_off), _ptr(pt_off), _ptr(pts), _ptr(alpha0),
                                            int(sys.getrecursionlimit() if max_retries is None else max_retries),
                                            _ptr(ring), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3])),
               "asep_alpha_shapes_points")
    out, k = [], 0
    for pg in pages:
        rows = []
        for _ in pg:
            rows.append((ring[pt_off[k]:pt_off[k] + res[0, k]].copy(), int(res[1, k]), bool(res[2, k]), int(res[3, k])))
            k += 1
        out.append(rows)
    return out


# One workgroup inserts an article's points one after the other, with passes over all its triangles for each: quadratic in the
# article's points (0.9 ms at 280, 4.4 ms at 896, 22 ms at 2,000, 76 ms at 4,000, 255 ms at 7,681 points on an MI355X, where Qhull
# takes 0.33 / 1.5 / 3.6 / 7.8 / 15.5 ms).  The device wins by triangulating a call's hundreds of articles side by side, so an
# article stays on it while it cannot hold up a call of 32 pages for longer than the host needs for a few of those pages.
DEVICE_TRIANGULATION_MAX_POINTS = 4096


def _regions_from_points(plans, alpha, logs, max_retries, device):
    """create_text_regions_pages behind the plans when the device triangulates too"""
    def on_device(pts):
        return 3 < pts.shape[0] <= DEVICE_TRIANGULATION_MAX_POINTS
    dev_pages = [[(pts, alpha) for pts, _ in jobs if on_device(pts)] if alpha > 0 else [] for jobs, _ in plans]
    rings = alpha_shapes_points_device(dev_pages, max_retries, device) if any(dev_pages) else [[] for _ in plans]
    out = []
    for (jobs, end), got, log in zip(plans, rings, logs):
        got = iter(got)
        regions = []
        try:
            for counter, (points, members) in enumerate(jobs):
                assert alpha > 0, "alpha value has to be greater than zero"
                if points.shape[0] <= 3:
                    bp = points.tolist()              # util.py:620: returned as they are
                    bp.append(bp[0])
                else:
                    ring, retries, failed, status = next(got) if on_device(points) else (None, 0, False, -1)
                    if status != 0:                   # not triangulated on the device: the host function, with what it prints or raises
                        bp = canonical_ring(geo.alpha_shape(points, alpha, log))
                    else:
                        for _ in range(retries):
                            log(RETRY_LINE)
                        if failed:
                            raise RecursionError(f"alpha_shape: no single boundary after {retries} increases of alpha")
                        bp = points[ring].tolist()
                        bp = canonical_ring(bp + [bp[0]])
                regions.append(("tr_" + str(counter), [[int(j) for j in i] for i in bp], members, counter))
            if end is not None:
                raise end
            out.append(regions)
        except Exception as e:      # noqa: BLE001 (the page's error, as the host path raises it)
            out.append(e)
    return out


def reading_order(baselines):
    """textregion_generation.py:80-99: the lines' indices sorted (stably) by the mean y of their baselines;
    returns the reading order index of each line."""
    keys = [1 / len(ys) * sum(int(y) for y in ys) for _, ys in baselines]
    order = sorted(range(len(baselines)), key=lambda i: keys[i])
    ro = [0] * len(baselines)
    for r, i in enumerate(order):
        ro[i] = r
    return ro
