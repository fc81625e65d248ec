"""Pages and settings of the heading evaluation golden (make_heading_eval_golden.py) and its tests.

A page is GT text regions (lists of line ids, a heading label each) with recorded per-line measurements: stroke width
(integers and halves), text height (integers) and net confidence (tenths), so that the fusion rule's comparisons meet
ties.  Lines without an outline measure (0, 0, 0.0), as the product's line_values gives them.  Edge pages: no regions, a
region without lines, lines without outlines, all lines equal (max == min), all-heading and no-heading GT."""
import numpy as np

N_RANDOM_PAGES = 24
N_SAMPLED_SETTINGS = 190
LOG_SETTINGS = 5           # settings of which the exact log text is recorded


def _page(name, regions, gt, meas, outline=None):
    lines = []
    for reg in regions:
        for lid in reg:
            has = True if outline is None else outline.get(lid, True)
            sw, th, net = meas[lid] if has else (0, 0, 0.0)
            lines.append({"id": lid, "outline": has, "sw": sw, "th": th, "net": net})
    return {"name": name, "regions": [list(r) for r in regions], "gt": [bool(g) for g in gt], "lines": lines}


def pages(seed=2020):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(N_RANDOM_PAGES):
        n_reg = int(rng.integers(1, 9))
        regions, meas, outline = [], {}, {}
        for r in range(n_reg):
            ids = [f"p{k}r{r}l{i}" for i in range(int(rng.integers(0 if rng.random() < 0.1 else 1, 6)))]
            regions.append(ids)
            big = rng.random() < 0.3
            for lid in ids:
                sw = float(rng.integers(2, 12)) / 2 + (2.0 if big else 0.0)
                th = int(rng.integers(18, 26)) + (int(rng.integers(8, 20)) if big else 0)
                net = int(rng.integers(0, 11)) / 10 if big else int(rng.integers(0, 6)) / 10
                meas[lid] = (sw, th, net)
                outline[lid] = rng.random() > 0.05
        gt = [bool(rng.random() < 0.35) for _ in regions]
        out.append(_page(f"page{k:02d}", regions, gt, meas, outline))
    # edge pages
    out.append(_page("no_regions", [], [], {}))
    out.append(_page("empty_region", [["e0", "e1"], [], ["e2"]], [True, True, False],
                     {"e0": (4.0, 30, 0.9), "e1": (2.0, 20, 0.1), "e2": (2.5, 22, 0.3)}))
    out.append(_page("no_outlines", [["o0", "o1"], ["o2"]], [False, True], {"o0": (3.0, 20, 0.5), "o1": (3.0, 20, 0.5),
                                                                            "o2": (6.0, 40, 1.0)}, {"o0": False, "o1": False}))
    out.append(_page("all_equal", [["q0", "q1"], ["q2", "q3"]], [True, False], {q: (3.5, 24, 0.6) for q in ("q0", "q1", "q2", "q3")}))
    out.append(_page("all_heading_gt", [["h0"], ["h1", "h2"], ["h3"]], [True, True, True],
                     {"h0": (5.0, 40, 0.8), "h1": (2.0, 20, 0.2), "h2": (6.0, 44, 0.9), "h3": (3.0, 21, 0.4)}))
    out.append(_page("no_heading_gt", [["n0", "n1"], ["n2"]], [False, False],
                     {"n0": (2.0, 20, 0.1), "n1": (2.5, 21, 0.2), "n2": (6.0, 40, 0.9)}))
    return out


def settings(seed=7):
    """tenths rows (threshold, net_w, sw_w, th_w, net_thresh, sw_thresh, th_thresh, sw_th_thresh, tlp) from the grid:
    the edge settings first, then a seeded sample"""
    edges = [(4, 0, 0, 10, 8, 8, 8, 7, 8), (9, 10, 0, 0, 10, 10, 10, 10, 10), (5, 0, 10, 0, 9, 8, 10, 8, 10),
             (4, 10, 0, 0, 8, 10, 9, 8, 9), (6, 5, 5, 0, 10, 9, 8, 7, 8), (7, 3, 3, 4, 8, 9, 10, 9, 10),
             (4, 0, 5, 5, 10, 10, 8, 7, 9), (9, 0, 0, 10, 8, 10, 10, 9, 8), (5, 8, 0, 2, 10, 10, 9, 9, 8),
             (8, 1, 9, 0, 9, 8, 9, 7, 10)]
    grid = []
    for t in range(4, 10):
        for nw in range(0, 11):
            for nt in range(8, 11):
                for swt in range(8, 11):
                    for tht in range(8, 11):
                        for tlp in range(8, 11):
                            ub = min(swt, tht)
                            for swth in range(ub - 1, ub + 1):
                                for sww in range(0, 10 - nw + 1):
                                    grid.append((t, nw, sww, 10 - nw - sww, nt, swt, tht, swth, tlp))
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(grid), N_SAMPLED_SETTINGS, replace=False)
    return edges + [grid[i] for i in sorted(pick.tolist())]
