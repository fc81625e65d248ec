"""Pages aimed at the seams of the two text block kernels (csrc/textblock_kernels.h), and counters that say, on the
reference side alone, that a page really reaches the seam it was built for.  No GPU and no reference import: the
yardsticks are slow_interline_distances / slow_neighbours of textblock_cases.py.

A page is a list of baselines (xs, ys) as in textblock_cases.py.  Interline cases are raw pages that the tests norm
(des_dist 5) before use; neighbour cases are given directly as what the kernel reads: boxes, distances and avg.

What the distance kernel's structure asks for:
  * it walks the scan "points of poly_a outer, polygons of the page inner" 64 positions per round and advances its lanes
    by (64 / Nb, 64 % Nb) with one wrap: pages of Nb = 1, 2, 3, 5 (many points of poly_a per round), 63, 64, 65, 127, 128,
    129, with point counts Pa such that the scan length Pa * Nb is 63, 64, 65, 128 or no multiple of 64;
  * within a round it applies the lowest passing lane and ballots again, and a pair is skipped when its box distance
    exceeds the RUNNING minimum: dense columns on which that order changes the result (counters of
    instrumented_interline_distances);
  * the comparisons bd <= dist, m < dist, |in_dist| <= 2 * des_dist and dist < max_d at equality: tie pages.

Exact equalities need exact arithmetic.  Only a normed polygon of one point (angle 0.0) or of two points on one row
(slope 0 from two points) has the orientation (1, 0) exactly; a longer horizontal line gets a regression slope of the order 1e-16 and
a vertical one cos(pi / 2) = 6e-17.  So the polygons whose distance is pinned on a tie page are such one- and two-point
lines; their neighbours may be any line, since only poly_a's orientation enters its distance.
"""
import math
import random

import textblock_cases as tc

DES_DIST = 5
MAX_DS = (500, 100)                   # dbscan_baselines / textregion_generation


def length_for_points(k):
    """pixel length of a straight two-point baseline that norms (des_dist 5) to k points: blow_up gives length + 1
    pixels, thin_out keeps up to 20 of them as they are and max(20, int(length / 5) + 1) of a longer run"""
    return k - 1 if k <= 20 else 5 * (k - 1)


def normed_points(length):
    """the inverse of length_for_points for any length"""
    return length + 1 if length + 1 <= 20 else max(20, int(length / DES_DIST) + 1)


def hline(x0, y, k, dy=0, reverse=False):
    """a baseline of k normed points from (x0, y), rising by dy over its length (|dy| <= length keeps the count)"""
    length = length_for_points(k)
    xs, ys = [x0, x0 + length], [y, y + (dy if abs(dy) <= length else 0)]
    return (xs[::-1], ys[::-1]) if reverse else (xs, ys)


def vline(x, y0, k, reverse=False):
    length = length_for_points(k)
    ys = [y0, y0 + length]
    return ([x, x], ys[::-1] if reverse else ys)


def lane_page(seed, nb, pa_cycle, pitch=14, per_col=24):
    """nb baselines in columns; baseline i norms to pa_cycle[i % len] points.  Left edges jitter by a few pixels so that
    neighbours pass the end-point test, rows are `pitch` apart, so every line has neighbours well below max_d."""
    rng = random.Random(seed)
    col_w = max(length_for_points(k) for k in pa_cycle) + 30
    page = []
    for i in range(nb):
        k = pa_cycle[i % len(pa_cycle)]
        col, row = divmod(i, per_col)
        x0 = 40 + col * col_w + rng.randint(0, 8)
        y = 60 + row * pitch + rng.randint(-2, 2)
        page.append(hline(x0, y, k, dy=rng.randint(-2, 2), reverse=rng.random() < 0.15))
    return page


def dense_page(seed, n_cols=4, n_lines=16, length=34, pitch=30, stagger=14, slope=0.35):
    """short skewed lines whose pitch is about their length, staggered along x: neighbouring boxes overlap, a line's
    nearest neighbour in off-distance is often NOT the nearest in box distance, and many pairs lie within a few pixels
    of the running minimum -- the order of the scan decides the result"""
    rng = random.Random(seed)
    page = []
    for c in range(n_cols):
        for r in range(n_lines):
            x0 = 50 + c * (length + 6) + rng.randint(-stagger, stagger)
            y0 = 50 + r * pitch + rng.randint(-pitch // 3, pitch // 3)
            ln = length + rng.randint(-10, 10)
            dy = int(round(ln * rng.uniform(-slope, slope)))
            n_pts = rng.choice([2, 2, 3])
            xs = [x0 + round(k * ln / (n_pts - 1)) for k in range(n_pts)]
            ys = [y0 + round(k * dy / (n_pts - 1)) + (rng.randint(-3, 3) if 0 < k < n_pts - 1 else 0) for k in range(n_pts)]
            page.append((xs[::-1], ys[::-1]) if rng.random() < 0.2 else (xs, ys))
    rng.shuffle(page)
    return page


def _dot(x, y):
    return ([x, x], [y, y])                    # norms to the single point (x, y): orientation (1, 0)


def _pair(x, y):
    return ([x, x + 1], [y, y])                # norms to two points on one row: orientation (1, 0)


def tie_same_off_page():
    """a one-point line with a neighbour 30 above and one 30 below.  The upper one comes first in the page and sets
    dist = 30; at the lower one the box distance is 30 == dist (evaluated: bd <= dist) and its minimum is 30 == dist (no
    change: m < dist is strict).  The same with a two-point line, and with the neighbours in the other order."""
    page = []
    for k, (x, mk) in enumerate(((100, _dot), (400, _pair), (700, _dot), (1000, _pair))):
        up, down = hline(x - 10, 200 - 30, 20), hline(x - 10, 200 + 30, 20)         # x - 10 .. x + 9: they span x
        page += [up, mk(x, 200), down] if k < 2 else [down, mk(x, 200), up]
    return page


def tie_in_dist_page():
    """|in_dist| <= 2 * des_dist at 10 and at 11.  A one-point line at (x, 300); below it a 20-pixel diagonal that comes
    nearer as it runs right, (x - 9 + t, 329 - t): its off-distance 29 - t is smallest at the last point.  With the last
    point at in-distance exactly 10 it counts (result 10); shifted right by one, the last point is at 11 and the point
    before it, at exactly 10 again, gives 11.  Shifted by two the last counted point gives 12."""
    page = []
    for k, shift in enumerate((0, 1, 2)):
        x = 100 + 300 * k
        page.append(_dot(x, 300))
        page.append(([x - 9 + shift, x + 10 + shift], [329, 310]))
    return page


def tie_max_d_page(max_d):
    """pairs of exactly oriented lines max_d - 1, max_d and max_d + 1 apart (dist < max_d, m < dist and bd <= dist at
    max_d itself), each pair 40 pixels right of the last so that the end-point test keeps the pairs apart.  From above
    the box distance of the lower line is the pitch, from below it is pitch - 1 (the box is one pixel higher than the
    line), so at pitch max_d + 1 the lower line still evaluates the upper one (bd == max_d) and finds m = max_d + 1."""
    page = []
    for k, pitch in enumerate((max_d - 1, max_d, max_d + 1)):
        for j, mk in enumerate((_dot, _pair)):
            x = 50 + 80 * k + 40 * j
            page += [mk(x, 20), mk(x, 20 + pitch)]
        x = 50 + 80 * k + 300
        page += [hline(x, 20, 7), _dot(x + 3, 20 + pitch)]          # a longer partner: only poly_a's orientation is pinned
    return page


def misc_page():
    """vertical, reversed and duplicated lines and lines at y in 0..fac*d, on top of a columns page that has some"""
    page = tc.columns_page(51, n_cols=2, n_lines=7, col_w=200)
    page += [vline(700, 100, 40), vline(712, 100, 40, reverse=True), vline(724, 130, 12), vline(724, 130, 12)]
    page += [hline(60, 0, 30), hline(60, 1, 30, reverse=True), hline(60, 9, 25), hline(64, 17, 3), hline(64, 17, 3)]
    return page


def interline_cases():
    """[(name, page)] in the order the batched test lists them"""
    mixed = [1, 2, 3, 7, 20, 33, 12, 5]
    cases = [
        ("nb1_pa64", lane_page(101, 1, [64])),                      # Pa * Nb = 64, every position is b == a
        ("nb2_pa32", lane_page(102, 2, [32])),                      # 64
        ("nb2_pa64", lane_page(103, 2, [64])),                      # 128
        ("nb2_pa1", lane_page(104, 2, [1, 5])),
        ("nb3_pa21", lane_page(105, 3, [21, 21, 7])),               # 63 and 21
        ("nb5_pa13", lane_page(106, 5, [13, 13, 64, 1, 26])),       # 65, 320, 5, 130
        ("nb63", lane_page(107, 63, mixed)),                        # Pa 1: 63
        ("nb64", lane_page(108, 64, mixed)),                        # step_b == 0; Pa 1: 64, Pa 2: 128
        ("nb65", lane_page(109, 65, mixed)),                        # Pa 1: 65
        ("nb127", lane_page(110, 127, mixed)),
        ("nb128", lane_page(111, 128, mixed)),                      # Pa 1: 128
        ("nb129", lane_page(112, 129, mixed)),
        ("dense_a", dense_page(201)),
        ("dense_b", dense_page(202, n_cols=3, n_lines=22, length=26, pitch=22, stagger=18, slope=0.5)),
        ("tie_same_off", tie_same_off_page()),
        ("tie_in_dist", tie_in_dist_page()),
        ("tie_max_d_500", tie_max_d_page(500)),
        ("tie_max_d_100", tie_max_d_page(100)),
        ("misc", misc_page()),
    ]
    return cases


LANE_COUNTS = {"nb1_pa64": 1, "nb2_pa32": 2, "nb2_pa64": 2, "nb2_pa1": 2, "nb3_pa21": 3, "nb5_pa13": 5, "nb63": 63,
               "nb64": 64, "nb65": 65, "nb127": 127, "nb128": 128, "nb129": 129}
SCAN_LENGTHS = {63, 64, 65, 128}      # Pa * Nb that some polygon of the lane pages must have, besides a non-multiple of 64
DENSE = ("dense_a", "dense_b")
TIES = ("tie_same_off", "tie_in_dist", "tie_max_d_500", "tie_max_d_100")
EMPTY_PAGE, ONE_LINE_PAGE = [], [hline(30, 40, 9)]


def prepared(pg):
    """(normed, orient) as the slow loops take them, from a NormedPage-like object (polys, angles)"""
    normed = [([int(v) for v in xs], [int(v) for v in ys]) for xs, ys in pg.polys]
    return normed, [(math.cos(a), math.sin(a)) for a in pg.angles]


def instrumented_interline_distances(normed, orient, des_dist=5, max_d=500):
    """slow_interline_distances (the same statements in the same order for `dist`) with counters for the page:
      skipped_would_lower   pairs (p_a, poly_b) skipped because the box distance exceeded the running dist, although the
                            box distance was within max_d and the pair's own minimum m was below the running dist: a box
                            test against max_d alone would have let them lower dist
      skipped_below_result  those of them whose m is below the polygon's final dist: a scan that evaluated them would
                            return another distance
      rounds_reordered      rounds of 64 consecutive scan positions (b == a included, as the kernel's lanes count them) in
                            which a pair passes both tests against the dist at the start of the round but fails against
                            the dist an earlier pair of the same round left
      eq_bd, eq_m, eq_in    bd == dist at the box test; m == dist at an evaluated pair; |in_dist| == 2 * des_dist at a
                            point of an evaluated pair
      eq_max_d              polygons whose dist ends at exactly max_d after at least one evaluated pair gave m == max_d
    Returns (distances, counters)."""
    boxes = []
    for xs, ys in normed:
        boxes.append((min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1))
    cnt = dict(skipped_would_lower=0, skipped_below_result=0, rounds_reordered=0, eq_bd=0, eq_m=0, eq_in=0, eq_max_d=0)
    inf = float("inf")
    out = []
    for a, (xa, ya) in enumerate(normed):
        ox, oy = orient[a]
        dist = max_d
        a1, a2 = (xa[0], ya[0]), (xa[-1], ya[-1])
        skipped, t, round_start, round_hit, m_at_max_d = [], 0, dist, False, False
        for px, py in zip(xa, ya):
            for b, (xb, yb) in enumerate(normed):
                if t % 64 == 0:
                    cnt["rounds_reordered"] += round_hit
                    round_start, round_hit = dist, False
                t += 1
                if b == a:
                    continue
                bx, by, bw, bh = boxes[b]
                bd = 0.0
                if px < bx:
                    bd += bx - px
                if px > bx + bw:
                    bd += px - bx - bw
                if py < by:
                    bd += by - py
                if py > by + bh:
                    bd += py - by - bh
                # the pair's own minimum, which does not read dist
                b1, b2 = (xb[0], yb[0]), (xb[-1], yb[-1])
                ins = [(p[0] - q[0]) * ox + (-p[1] + q[1]) * oy for p in (a1, a2) for q in (b1, b2)]
                end_skip = all(v < 0 for v in ins) or all(v > 0 for v in ins)
                m, n_eq_in = inf, 0
                if not end_skip:
                    for qx, qy in zip(xb, yb):
                        dx, dy = px - qx, -py + qy
                        in_d = abs(dx * ox + dy * oy)
                        n_eq_in += in_d == 2 * des_dist
                        if in_d <= 2 * des_dist:
                            m = min(m, abs(dx * oy - dy * ox))
                passes_start = bd <= round_start and m < round_start
                cnt["eq_bd"] += bd == dist
                if bd > dist:
                    if bd <= max_d and m < dist:
                        cnt["skipped_would_lower"] += 1
                        skipped.append(m)
                    round_hit = round_hit or passes_start
                    continue
                if end_skip:
                    continue
                cnt["eq_m"] += m == dist
                cnt["eq_in"] += n_eq_in
                m_at_max_d = m_at_max_d or m == max_d
                if passes_start and not m < dist:
                    round_hit = True
                for qx, qy in zip(xb, yb):
                    dx, dy = px - qx, -py + qy
                    if abs(dx * ox + dy * oy) <= 2 * des_dist:
                        dist = min(dist, abs(dx * oy - dy * ox))
        cnt["rounds_reordered"] += round_hit
        cnt["skipped_below_result"] += sum(1 for m in skipped if m < dist)
        cnt["eq_max_d"] += dist == max_d and m_at_max_d
        out.append(dist if dist < max_d else max_d)
    return out, cnt


# ---- neighbour cases ----------------------------------------------------------------------------------------------------

FAC = 1.25


def boxes_of(normed):
    return [(min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1) for xs, ys in normed]


def _row(x0, y, length):
    """an already normed horizontal line of length + 1 points (length <= 19: norming would keep it as it is)"""
    return (list(range(x0, x0 + length + 1)), [y] * (length + 1))


def column_neighbour_case(n, seed):
    """n short lines in columns, 6 pixels apart, distances 8 / 10 / 12.5 / out of range around avg 10: a handful of
    neighbours per row; the order is shuffled so that a row's bits spread over its words"""
    rng = random.Random(seed)
    normed = [_row(30 + 40 * (i // 12) + rng.randint(0, 3), 20 + 6 * (i % 12), rng.randint(8, 15)) for i in range(n)]
    rng.shuffle(normed)
    dists = [rng.choice([8.0, 10.0, 12.5, 3.0, 500.0, 7.3]) for _ in range(n)]
    return normed, dists, 10.0


def surface_tie_case():
    """>= 0.95 * surface at equality.  Line j is 18 long (box w 19, h 1: surface 20 * 2 = 40, and 0.95 * 40 == 38.0 as
    Python evaluates it) and lies 5 below the end of the long line i, sticking out by k pixels: the expanded box of i
    covers (20 - k) * 2 of it, 38 at k = 1 (a neighbour by equality), 36 at k = 2 (not), 40 at k = 0.  The long line is
    far too large to be covered by j's box, so the other half of the `or` is false.  One triple per k, 200 apart."""
    normed, dists = [], []
    for n, k in enumerate((1, 2, 0)):
        y = 100 + 200 * n
        normed += [(list(range(50, 251, 5)), [y] * 41), _row(250 - 18 + k, y + 5, 18)]       # i ends at x = 250
        dists += [10.0, 10.0]
    return normed, dists, 10.0


def top_edge_case():
    """int() truncates y - fac * d toward zero.  Line i at y = 4 with d = 7.3: y - 9.125 = -5.125 -> -5 (floor: -6), and
    h + 18.25 -> 19, so its expanded box reaches down to y = 14 (floor: 13).  Line j at y = 13 (box 13..14) is covered
    entirely under truncation and only by half under floor; j's own expanded box (d = 4: 8..19) does not reach i.  More
    lines at y = 0..9 with fractional distances, and a pair deep in the page for contrast."""
    normed = [_row(40, 4, 15), _row(42, 13, 10), _row(100, 0, 12), _row(100, 9, 12), _row(160, 2, 12), _row(161, 11, 9),
              _row(40, 300, 15), _row(42, 309, 10)]
    dists = [7.3, 4.0, 6.9, 6.9, 7.3, 4.1, 7.3, 4.0]
    return normed, dists, 7.3


def grid_neighbour_case(n=2049, seed=7):
    """n lines of 9 points on a regular grid (63 rows 6 pixels apart per column), in shuffled order: with distances
    around avg 10 the expanded boxes reach two rows up and down, so most rows have four neighbours, anywhere in the
    row's 65 words (the page has more lines than 64 threads * 32 bits)"""
    rng = random.Random(seed)
    normed = [_row(20 + 30 * (i // 63), 10 + 6 * (i % 63), 8) for i in range(n)]
    rng.shuffle(normed)
    dists = [(8.0, 10.0, 12.5, 7.3, 500.0)[rng.randrange(5)] for _ in range(n)]
    return normed, dists, 10.0


def neighbour_cases():
    """[(name, normed polygons, distances, avg)] small enough for slow_neighbours"""
    cases = [("n%d" % n, *column_neighbour_case(n, 300 + n)) for n in (31, 32, 33, 64, 65)]
    cases += [("surface_tie", *surface_tie_case()), ("top_edge", *top_edge_case())]
    return cases


def slow_neighbours_floor(boxes, dists, avg, fac=FAC):
    """slow_neighbours with math.floor in place of int(): what a kernel that rounded toward minus infinity would give"""
    def exp(i):
        d = dists[i]
        if not 0.5 * avg <= d <= 1.5 * avg:
            d = avg
        x, y, w, h = boxes[i]
        return int(x), math.floor(y - fac * d), int(w), math.floor(h + 2 * fac * d)

    def inter(r, s):
        tx1, ty1 = max(r[0], s[0]), max(r[1], s[1])
        w, h = min(r[0] + r[2], s[0] + s[2]) - tx1, min(r[1] + r[3], s[1] + s[3]) - ty1
        return (w + 1) * (h + 1) if w >= 0 and h >= 0 else 0
    out = []
    for i in range(len(boxes)):
        s1 = (boxes[i][3] + 1) * (boxes[i][2] + 1)
        out.append([j for j in range(len(boxes)) if j != i and (
            inter(exp(i), boxes[j]) >= 0.95 * (boxes[j][3] + 1) * (boxes[j][2] + 1) or inter(exp(j), boxes[i]) >= 0.95 * s1)])
    return out


def surface_equalities(boxes, dists, avg, fac=FAC):
    """ordered pairs (i, j) with intersection(expanded i, box j) == 0.95 * surface(j) as Python evaluates it"""
    def exp(i):
        d = dists[i]
        if not 0.5 * avg <= d <= 1.5 * avg:
            d = avg
        x, y, w, h = boxes[i]
        return int(x), int(y - fac * d), int(w), int(h + 2 * fac * d)
    hits = []
    for i in range(len(boxes)):
        r = exp(i)
        for j, s in enumerate(boxes):
            if j == i:
                continue
            tx1, ty1 = max(r[0], s[0]), max(r[1], s[1])
            w, h = min(r[0] + r[2], s[0] + s[2]) - tx1, min(r[1] + r[3], s[1] + s[3]) - ty1
            s12 = (w + 1) * (h + 1) if w >= 0 and h >= 0 else 0
            if s12 and s12 == 0.95 * ((s[3] + 1) * (s[2] + 1)):
                hits.append((i, j))
    return hits


def fast_neighbours(boxes, dists, avg, fac=FAC):
    """slow_neighbours restated with numpy over all ordered pairs at once: the same float64 operations in the same
    order (y - fac * d, h + 2 * fac * d truncated toward zero; 0.95 * surface), integers in int64"""
    import numpy as np
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    d = np.asarray(dists, np.float64).copy()
    d[~((0.5 * avg <= d) & (d <= 1.5 * avg))] = avg
    x, y, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    ey = np.trunc(y - fac * d).astype(np.int64)
    eh = np.trunc(h + 2 * fac * d).astype(np.int64)
    surf = (h + 1) * (w + 1)
    # inter[i, j] = intersection(expanded i, box j)
    tx1 = np.maximum(x[:, None], x[None, :])
    ty1 = np.maximum(ey[:, None], y[None, :])
    iw = np.minimum((x + w)[:, None], (x + w)[None, :]) - tx1
    ih = np.minimum((ey + eh)[:, None], (y + h)[None, :]) - ty1
    inter = np.where((iw >= 0) & (ih >= 0), (iw + 1) * (ih + 1), 0)
    want = 0.95 * surf.astype(np.float64)
    m = (inter >= want[None, :]) | (inter.T >= want[:, None])
    np.fill_diagonal(m, False)
    return [np.flatnonzero(r).tolist() for r in m]
