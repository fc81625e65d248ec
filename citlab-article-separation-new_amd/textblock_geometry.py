"""Host geometry of the text block detection stage, restated exactly from the reference's ``python_util/geometry``.

    round_to_nearest_integer   python_util/math/rounding.py:19-31   x % 1 >= 0.5 -> int(x) + 1 (int truncates toward zero)
    blow_up / thin_out         python_util/geometry/polygon.py:168-246
    norm_poly_dists            polygon.py:249-271 (a box wider or higher than 100000 px becomes the polygon [(0, 0)])
    calc_reg_line_stats        polygon.py:274-319 with linear_regression.py:6-59 (np.matmul, as the reference calls it)
    scale_polygons             dbscan_baselines.py:13-32 (float64 scale, then astype(int))
    alpha_shape                python_util/geometry/util.py:568-697 (edge toggling, ordered circles, alpha * 1.2 retries)

A polygon is a pair of int64 numpy arrays (xs, ys).  The vectorised forms evaluate every float64 operation in the
reference's order (elementwise numpy arithmetic is IEEE double, like Python's float), so their results are identical.
"""
import math
import sys

import numpy as np

BOX_LIMIT = 100000


def round_to_nearest_integer(x):
    """rounding.py:19-31 on a float64 array: Python's ``x % 1`` (fmod, then + 1 for a negative remainder)."""
    x = np.asarray(x, dtype=np.float64)
    r = np.fmod(x, 1.0)
    r = np.where(r < 0, r + 1.0, r)
    t = np.trunc(x).astype(np.int64)
    return np.where(r >= 0.5, t + 1, t)


def blow_up(xs, ys):
    """polygon.py:168-215: the pixels on the segments between adjacent points (x-major or y-major steps)."""
    xs = [int(v) for v in xs]
    ys = [int(v) for v in ys]
    n = len(xs)
    out_x, out_y = [], []
    for i in range(1, n):
        x1, y1, x2, y2 = xs[i - 1], ys[i - 1], xs[i], ys[i]
        diff_x, diff_y = abs(x2 - x1), abs(y2 - y1)
        if max(diff_x, diff_y) < 1:
            if i == n - 1:
                out_x.append(np.array([x2], np.int64))
                out_y.append(np.array([y2], np.int64))
            continue
        out_x.append(np.array([x1], np.int64))
        out_y.append(np.array([y1], np.int64))
        if diff_x >= diff_y:
            j = np.arange(1, diff_x, dtype=np.int64)
            xn = x1 + j if x1 < x2 else x1 - j
            yn = round_to_nearest_integer(y1 + (xn - x1) * (y2 - y1) / (x2 - x1))
        else:
            j = np.arange(1, diff_y, dtype=np.int64)
            yn = y1 + j if y1 < y2 else y1 - j
            xn = round_to_nearest_integer(x1 + (yn - y1) * (x2 - x1) / (y2 - y1))
        out_x.append(xn)
        out_y.append(yn)
        if i == n - 1:
            out_x.append(np.array([x2], np.int64))
            out_y.append(np.array([y2], np.int64))
    if not out_x:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(out_x).astype(np.int64), np.concatenate(out_y).astype(np.int64)


def thin_out(xs, ys, des_dist):
    """polygon.py:218-246: at most max(20, int((n-1)/des_dist)+1) points, indices int(i * step); <= 20 points unchanged."""
    n = len(xs)
    if n <= 20:
        return xs, ys
    dist = n - 1
    des_pts = max(20, int(dist / des_dist) + 1)
    step = dist / (des_pts - 1)
    idx = (np.arange(des_pts - 1, dtype=np.float64) * step).astype(np.int64)
    return np.append(xs[idx], xs[-1]), np.append(ys[idx], ys[-1])


def bounds(xs, ys):
    """polygon.py:84-92 calculate_bounds: (x, y, w, h) with w = max - min + 1."""
    x0, y0 = int(xs.min()), int(ys.min())
    return x0, y0, int(xs.max()) - x0 + 1, int(ys.max()) - y0 + 1


def norm_poly_dists(polys, des_dist):
    """polygon.py:249-271 for a list of (xs, ys) polygons."""
    out = []
    for xs, ys in polys:
        xs = np.asarray(xs, np.int64)
        ys = np.asarray(ys, np.int64)
        if len(xs) and (int(xs.max()) - int(xs.min()) + 1 > BOX_LIMIT or int(ys.max()) - int(ys.min()) + 1 > BOX_LIMIT):
            xs, ys = np.zeros(1, np.int64), np.zeros(1, np.int64)
        bx, by = blow_up(xs, ys)
        out.append(thin_out(bx, by, des_dist))
    return out


def _calc_line_slope(x_points, y_points):
    """linear_regression.py:6-59 calc_line, second component (the slope); the normal equations through np.matmul on
    the same (n, 2) / (n,) float64 arrays as the reference, so that BLAS sums in the same order."""
    n_points = len(x_points)
    min_x = min(min(x_points), 100000)
    max_x = max(max(x_points), 0)
    if max_x - min_x < 2:
        return float("inf")
    a = np.zeros([n_points, 2])
    y = np.zeros([n_points])
    y[:] = y_points
    a[:, 0] = 1.0
    a[:, 1] = x_points
    a_t = np.transpose(a)
    ls = np.matmul(a_t, a)
    rs = np.matmul(a_t, y)
    det = ls[0, 0] * ls[1, 1] - ls[0, 1] * ls[1, 0]
    if det < 1e-9:
        print("LinearRegression Error: Numerically unstable.")
        return float("inf")
    d = 1.0 / det
    inv = np.empty_like(ls)
    inv[0, 0] = d * ls[1, 1]
    inv[1, 1] = d * ls[0, 0]
    inv[1, 0] = -d * ls[1, 0]
    inv[0, 1] = -d * ls[0, 1]
    return np.matmul(inv, rs)[1]


def calc_reg_line_angle(xs, ys):
    """polygon.py:274-319: the angle of calc_reg_line_stats (the orientation of the baseline, in [0, 2*pi))."""
    xs = [int(v) for v in xs]
    ys = [int(v) for v in ys]
    n = len(xs)
    if n <= 1:
        return 0.0
    if n > 2:
        if max(xs) == min(xs):
            m = float("inf")
        else:
            m = _calc_line_slope(xs, [-y for y in ys])
    else:
        x1, x2 = xs
        y1, y2 = [-y for y in ys]
        m = float("inf") if x1 == x2 else (y2 - y1) / (x2 - x1)
    angle = math.pi / 2 if m == float("inf") else math.atan(m)
    if -math.pi / 2 < angle <= -math.pi / 4:
        if ys[0] > ys[-1]:
            angle += math.pi
    if -math.pi / 4 < angle <= math.pi / 4:
        if xs[0] > xs[-1]:
            angle += math.pi
    if math.pi / 4 < angle < math.pi / 2:
        if ys[0] < ys[-1]:
            angle += math.pi
    if angle < 0:
        angle += 2 * math.pi
    return angle


def scale_polygons(polys, scaling_factor):
    """dbscan_baselines.py:13-32 get_list_of_scaled_polygons."""
    return [((scaling_factor * np.array([np.asarray(xs, np.int64)])).astype(int)[0],
             (scaling_factor * np.array([np.asarray(ys, np.int64)])).astype(int)[0]) for xs, ys in polys]


def _edge_key(e):
    return (e[0], e[1]) if e[0] < e[1] else (e[1], e[0])


def _ordered_circle(edges):
    """util.py:588-613 get_ordered_circles: the visited test (edge or its reverse in the circle) on a set of
    undirected keys -- the toggled edge list never holds both directions of one edge."""
    if not edges:
        return [], []
    circle = [edges[0]]
    visited = {_edge_key(edges[0])}
    while len(circle) < len(edges):
        nothing = True
        for e in edges:
            k = _edge_key(e)
            if k in visited:
                continue
            if e[0] == circle[-1][1]:
                circle.append(e)
                visited.add(k)
                nothing = False
            elif e[1] == circle[-1][1]:
                circle.append((e[1], e[0]))
                visited.add(k)
                nothing = False
        if nothing:
            break
    return circle, [e for e in edges[1:] if _edge_key(e) not in visited]


def alpha_shape(points, alpha, log=print):
    """util.py:568-697.  ``points``: int array (n, 2).  Returns the boundary as a closed list of [x, y]; each retry with
    alpha * 1.2 reports the reference's line through ``log``.  The reference retries by recursion and so gives up with
    a RecursionError after about sys.getrecursionlimit() retries (e.g. when a sliver triangle's Heron area is NaN and
    its hole never closes); the loop here stops at that count with the same error."""
    from scipy.spatial import Delaunay
    assert alpha > 0, "alpha value has to be greater than zero"
    points = np.asarray(points)
    max_retries = sys.getrecursionlimit()
    retries = 0
    while True:
        if points.shape[0] <= 3:
            boundary_points = points.tolist()
            boundary_points.append(boundary_points[0])
            return boundary_points
        tri = Delaunay(points).simplices
        pa, pb, pc = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]

        def side(u, v):              # np.linalg.norm of an integer difference: sqrt of an exact sum of squares
            d = (u - v).astype(np.float64)
            return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        a, b, c = side(pa, pb), side(pb, pc), side(pc, pa)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (a + b + c) / 2.0
            area = np.sqrt(s * (s - a) * (s - b) * (s - c))
            circum_r = a * b * c / (4.0 * (area + 1e-8))
        edges = {}                                    # undirected key -> directed edge, in list order
        for t in np.flatnonzero(circum_r < alpha):
            ia, ib, ic = (int(v) for v in tri[t])
            for e in ((ia, ib), (ib, ic), (ic, ia)):
                k = _edge_key(e)
                if k in edges:
                    del edges[k]
                else:
                    edges[k] = e
        rest = list(edges.values())
        boundaries = []
        while True:
            circle, rest = _ordered_circle(rest)
            boundaries.append(circle)
            if not rest:
                break
        retry = boundaries == [[]] or len(boundaries) > 1
        if not retry:
            counts = {}
            for e in boundaries[0]:
                for v in e:
                    counts[v] = counts.get(v, 0) + 1
            retry = any(c > 2 for c in counts.values())
        if retry:
            log("alpha value not suitable -> is increased")
            retries += 1
            if retries >= max_retries:
                raise RecursionError(f"alpha_shape: no single boundary after {retries} increases of alpha")
            alpha = alpha + alpha * 0.2
            continue
        boundary_points = [points[e[0]].tolist() for e in boundaries[0]]
        boundary_points.append(boundary_points[0])
        return boundary_points
