"""Seeded synthetic baseline-only pages for the text block detection goldens (make_textblock_golden.py) and benchmarks.

A page is a list of baselines, each a pair (xs, ys) of int lists.  The generator covers what the reference's
distance / neighbourhood code branches on: columns of lines, headings across columns, skewed, reversed and vertical
lines, 2-point and short (<= 20 blown-up points) baselines, duplicated baselines and lines at the top edge of the page.
"""
import random


def _line(rng, x0, y0, width, n_pts, slope=0.0, jitter=2, reverse=False):
    xs = sorted({x0 + round(k * width / (n_pts - 1)) for k in range(n_pts)})
    ys = [int(round(y0 + slope * (x - x0))) + rng.randint(-jitter, jitter) for x in xs]
    if reverse:
        xs, ys = xs[::-1], ys[::-1]
    return xs, ys


def columns_page(seed, n_cols=3, n_lines=12, col_w=300, gap=40, pitch=36, x_off=30, y_off=60, heading=True,
                 extras=True):
    rng = random.Random(seed)
    page = []
    y_start = y_off
    if heading:                                      # a heading across all columns
        page.append(_line(rng, x_off, y_off, n_cols * col_w + (n_cols - 1) * gap - 20, 6, jitter=1))
        y_start += 2 * pitch
    for c in range(n_cols):
        x0 = x_off + c * (col_w + gap)
        y = y_start + rng.randint(0, 8)
        for k in range(n_lines):
            w = col_w - rng.randint(0, 60) if k % 7 != 6 else rng.randint(40, 120)      # short paragraph ends
            n_pts = rng.choice([2, 3, 5, 8])
            slope = rng.uniform(-0.03, 0.03)
            page.append(_line(rng, x0 + rng.randint(0, 6), y, w, n_pts, slope))
            y += pitch + rng.randint(-3, 3) + (pitch if k % 7 == 6 else 0)
    if extras:
        page.append(_line(rng, x_off + 10, 4, 200, 4, jitter=1))                   # at the top edge: y - fac*d < 0
        page.append(_line(rng, x_off + 5, y_start + 40, 250, 5, slope=0.35))        # skewed
        page.append(_line(rng, x_off + 400, y_start + 90, 220, 4, slope=-0.2, reverse=True))   # reversed, skewed
        vx = x_off + n_cols * (col_w + gap) + 10                                   # vertical lines
        page.append(([vx, vx, vx + 1], [y_start, y_start + 150, y_start + 300]))
        page.append(([vx + 30, vx + 30], [y_start + 300, y_start]))
        page.append(([x_off + 20, x_off + 33], [y_start + 500, y_start + 501]))     # <= 20 blown-up points
        page.append(([x_off + 60, x_off + 64, x_off + 75], [y_start + 520, y_start + 520, y_start + 522]))
        page.append(page[3])                                                       # a duplicate baseline
        page.append(([x_off + 100, x_off + 100], [y_start + 600, y_start + 600]))  # two identical points
    return page


def random_page(seed, n_lines, width=3000, height=4500, max_w=400):
    """Lines scattered over a page (the fuzz inputs)."""
    rng = random.Random(seed)
    page = []
    for _ in range(n_lines):
        x0, y0 = rng.randint(0, width - 50), rng.randint(0, height)
        w = rng.randint(2, max_w)
        kind = rng.random()
        if kind < 0.08:
            page.append(([x0, x0 + rng.randint(-2, 2)], [y0, y0 + rng.randint(20, 200)]))
        else:
            page.append(_line(rng, x0, y0, w, rng.randint(2, 6), rng.uniform(-0.5, 0.5), 3, rng.random() < 0.2))
    return page


def golden_pages():
    pages = [
        ("empty", []),
        ("one", [([100, 400], [200, 205])]),
        ("two", [([100, 400], [200, 205]), ([100, 380], [240, 243])]),
        ("two_duplicate", [([100, 400], [200, 205]), ([100, 400], [200, 205])]),
        ("cols2", columns_page(1, n_cols=2, n_lines=8, col_w=260)),
        ("cols3", columns_page(2, n_cols=3, n_lines=10, col_w=220)),
        ("cols3_tight", columns_page(3, n_cols=3, n_lines=9, col_w=180, gap=15, pitch=22)),
        ("cols4_noextras", columns_page(4, n_cols=4, n_lines=8, col_w=160, heading=False, extras=False)),
        ("scatter", random_page(5, 40, 1500, 2000, 200)),
    ]
    return pages


def slow_interline_distances(normed, orient, des_dist=5, max_d=500):
    """dbscan_baselines.py:35-110 restated loop for loop (the reference's Python path) on normed polygons given as
    (xs, ys) lists with their (cos, sin): the slow yardstick of the fuzz tests."""
    boxes = []
    for xs, ys in normed:
        boxes.append((min(xs), min(ys), max(xs) - min(xs) + 1, max(ys) - min(ys) + 1))
    out = []
    for a, (xa, ya) in enumerate(normed):
        ox, oy = orient[a]
        dist = max_d
        a1, a2 = (xa[0], ya[0]), (xa[-1], ya[-1])
        for px, py in zip(xa, ya):
            for b, (xb, yb) in enumerate(normed):
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
                if bd > dist:
                    continue
                b1, b2 = (xb[0], yb[0]), (xb[-1], yb[-1])
                ins = [(p[0] - q[0]) * ox + (-p[1] + q[1]) * oy for p in (a1, a2) for q in (b1, b2)]
                if all(v < 0 for v in ins) or all(v > 0 for v in ins):
                    continue
                for qx, qy in zip(xb, yb):
                    dx, dy = px - qx, -py + qy
                    if abs(dx * ox + dy * oy) <= 2 * des_dist:
                        dist = min(dist, abs(dx * oy - dy * ox))
        out.append(dist if dist < max_d else max_d)
    return out


def slow_neighbours(boxes, dists, avg, fac=1.25):
    """dbscan_baselines.py:253-307 region_query for every row, restated (boxes (x, y, w, h) with w = max-min+1)."""
    def exp(i):
        d = dists[i]
        if not 0.5 * avg <= d <= 1.5 * avg:
            d = avg
        x, y, w, h = boxes[i]
        return int(x), int(y - fac * d), int(w), int(h + 2 * fac * d)

    def inter(r, s):
        tx1, ty1, tx2, ty2 = r[0], r[1], r[0] + r[2], r[1] + r[3]
        tx1, ty1, tx2, ty2 = max(tx1, s[0]), max(ty1, s[1]), min(tx2, s[0] + s[2]), min(ty2, s[1] + s[3])
        w, h = tx2 - tx1, ty2 - ty1
        return (w + 1) * (h + 1) if w >= 0 and h >= 0 else 0

    out = []
    for i in range(len(boxes)):
        r1 = exp(i)
        s1 = (boxes[i][3] + 1) * (boxes[i][2] + 1)
        row = []
        for j in range(len(boxes)):
            if j == i:
                continue
            s2 = (boxes[j][3] + 1) * (boxes[j][2] + 1)
            if inter(r1, boxes[j]) >= 0.95 * s2 or inter(exp(j), boxes[i]) >= 0.95 * s1:
                row.append(j)
        out.append(row)
    return out
