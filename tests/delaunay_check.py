"""Exact checks of a 2-D Delaunay triangulation in scipy's two tables (tests/test_delaunay_host.py, tests/test_delaunay_gpu.py):
``check_triangulation`` asserts in integers what makes the tables a Delaunay triangulation of the points, whichever way cocircular
points were split; ``same_cycle`` compares two rings up to rotation and reversal; ``canonical_ring`` restates the form the
``--device_triangulation`` path writes; ``flip_cocircular`` turns one valid triangulation into another.  numpy and Python ints only."""
import numpy as np


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_with_collinear(points):
    """the convex hull of distinct integer points, counter-clockwise, points on its edges included (monotone chain)"""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) < 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) < 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _incircle(pa, pb, pc, pd):
    """> 0 where d is strictly inside the circle through the counter-clockwise a, b, c; arrays broadcast.  Exact in the dtype's range."""
    adx, ady = pa[..., 0] - pd[..., 0], pa[..., 1] - pd[..., 1]
    bdx, bdy = pb[..., 0] - pd[..., 0], pb[..., 1] - pd[..., 1]
    cdx, cdy = pc[..., 0] - pd[..., 0], pc[..., 1] - pd[..., 1]
    return ((adx * adx + ady * ady) * (bdx * cdy - cdx * bdy) + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy)
            + (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady))


def _exact(points):
    """int64 where the in-circle determinant fits it (extents below 2^14: below 3 * 2^58), Python ints otherwise"""
    p = np.asarray(points).reshape(-1, 2).astype(np.int64)
    if len(p) and max(int(p[:, 0].max() - p[:, 0].min()), int(p[:, 1].max() - p[:, 1].min())) < 2 ** 14:
        return p - p.min(axis=0)
    return p.astype(object)


def check_triangulation(points, simplices, neighbors):
    """asserts that (simplices, neighbors) is a Delaunay triangulation of the distinct points of ``points``"""
    pts = _exact(points)
    simp = np.asarray(simplices, np.int64).reshape(-1, 3)
    neigh = np.asarray(neighbors, np.int64).reshape(-1, 3)
    T = len(simp)
    assert neigh.shape == simp.shape
    assert T > 0 and simp.min() >= 0 and simp.max() < len(pts), "a corner is not a point"
    assert neigh.min() >= -1 and neigh.max() < T, "a neighbour is not a triangle"
    coords = [(int(x), int(y)) for x, y in pts]
    distinct = set(coords)
    # every triangle strictly counter-clockwise
    a, b, c = pts[simp[:, 0]], pts[simp[:, 1]], pts[simp[:, 2]]
    orient = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    assert (orient > 0).all(), "triangle %d is not counter-clockwise" % int(np.flatnonzero(~(orient > 0))[0])
    # every distinct point is a corner, one index per point
    used = sorted(set(simp.ravel().tolist()))
    assert len(set(coords[i] for i in used)) == len(used), "two corners are the same point"
    assert set(coords[i] for i in used) == distinct, "a point is in no triangle"
    # neighbours: opposite corner j lies the edge (corner j + 1, corner j + 2); its other side lists it reversed and points back
    owner = {}
    for t in range(T):
        for j in range(3):
            e = (int(simp[t, (j + 1) % 3]), int(simp[t, (j + 2) % 3]))
            assert e not in owner, "edge %s is on the same side of triangles %d and %d" % (e, owner[e][0], t)
            owner[e] = (t, j)
    boundary = []
    for (u, v), (t, j) in owner.items():
        other = owner.get((v, u))
        if other is None:
            assert neigh[t, j] == -1, "triangle %d: nothing lies across edge %d, neighbors says %d" % (t, j, neigh[t, j])
            boundary.append((u, v))
        else:
            assert neigh[t, j] == other[0], "triangle %d: %d lies across edge %d, neighbors says %d" % (t, other[0], j, neigh[t, j])
            assert neigh[other[0], other[1]] == t, "triangle %d: %d lies across edge %d, neighbors says %d" % (
                other[0], t, other[1], neigh[other[0], other[1]])
    # no point strictly inside a circumcircle
    up = pts[used]
    inside = _incircle(a[:, None, :], b[:, None, :], c[:, None, :], up[None, :, :]) > 0
    assert not inside.any(), "point %d is inside the circumcircle of triangle %d" % (used[int(np.argwhere(inside)[0][1])],
                                                                                    int(np.argwhere(inside)[0][0]))
    # the union is the convex hull: the boundary edges are one cycle through every hull point, the areas agree, T = 2n - 2 - h
    hull = hull_with_collinear(coords)
    h, n = len(hull), len(distinct)
    assert len(boundary) == h, "%d boundary edges, the hull has %d points" % (len(boundary), h)
    nxt = {coords[u]: coords[v] for u, v in boundary}
    assert len(nxt) == h
    walk, cur = [], hull[0]
    for _ in range(h):
        walk.append(cur)
        cur = nxt[cur]
    assert cur == hull[0] and walk == hull, "the boundary is not the convex hull"
    hull_area2 = sum(hull[i][0] * hull[(i + 1) % h][1] - hull[(i + 1) % h][0] * hull[i][1] for i in range(h))
    assert int(orient.sum()) == hull_area2, "the triangles do not tile the hull"
    assert T == 2 * n - 2 - h, "%d triangles for %d points with %d on the hull" % (T, n, h)


def triangle_set(simplices):
    """the triangles as a set of sorted corner triples"""
    return set(tuple(sorted(int(v) for v in s)) for s in np.asarray(simplices).reshape(-1, 3))


def same_cycle(a, b):
    """two rings (sequences of points or indices, the first not repeated at the end) equal up to rotation and reversal"""
    a = [tuple(np.atleast_1d(v).tolist()) for v in a]
    b = [tuple(np.atleast_1d(v).tolist()) for v in b]
    if len(a) != len(b):
        return False
    if not a:
        return True
    for seq in (b, b[::-1]):
        for k in (i for i, v in enumerate(seq) if v == a[0]):
            if seq[k:] + seq[:k] == a:
                return True
    return False


def canonical_ring(ring):
    """textblock.canonical_ring restated: from the smallest (y, x) vertex, in the direction of positive shoelace area"""
    ring = [(int(x), int(y)) for x, y in ring]
    n = len(ring)
    area2 = sum(ring[i][0] * ring[(i + 1) % n][1] - ring[(i + 1) % n][0] * ring[i][1] for i in range(n))
    if area2 < 0:
        ring = ring[::-1]
    k = min(range(n), key=lambda i: (ring[i][1], ring[i][0]))
    return ring[k:] + ring[:k]


def flip_cocircular(points, simplices, neighbors, rng=None):
    """Another valid Delaunay triangulation of the same points: every pair of neighbouring triangles whose four corners lie on one
    circle has its diagonal flipped, each triangle at most once.  Returns (simplices, neighbors, number of flips); the neighbour table
    is rebuilt from the edges."""
    pts = _exact(points)
    simp = np.array(simplices, np.int64).reshape(-1, 3)
    neigh = np.asarray(neighbors, np.int64).reshape(-1, 3)
    order = list(range(len(simp)))
    if rng is not None:
        rng.shuffle(order)
    done, flips = set(), 0
    for t in order:
        if t in done:
            continue
        for j in range(3):
            o = int(neigh[t, j])
            if o < 0 or o in done or t in done:
                continue
            a, b, c = (int(simp[t, (j + k) % 3]) for k in range(3))          # a faces the shared edge (b, c)
            d = next(int(v) for v in simp[o] if v != b and v != c)
            if int(_incircle(pts[a], pts[b], pts[c], pts[d])) != 0:
                continue
            # a, b, d, c is the quadrilateral, counter-clockwise; it is strictly convex because the four lie on one circle
            simp[t] = (a, b, d)
            simp[o] = (a, d, c)
            done.update((t, o))
            flips += 1
    owner = {}
    for t in range(len(simp)):
        for j in range(3):
            owner[(int(simp[t, (j + 1) % 3]), int(simp[t, (j + 2) % 3]))] = t
    out = np.full(simp.shape, -1, np.int32)
    for (u, v), t in owner.items():
        j = next(j for j in range(3) if int(simp[t, (j + 1) % 3]) == u and int(simp[t, (j + 2) % 3]) == v)
        out[t, j] = owner.get((v, u), -1)
    return simp.astype(np.int32), out, flips
