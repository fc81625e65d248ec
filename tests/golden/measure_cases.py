"""Seeded synthetic ground-truth / hypothesis pairs for the article separation measure goldens (make_measure_golden.py),
tests and benchmarks, built on the pages of textblock_cases.py.

A side is a list of [article id or None, [[xs, ys], ...]] entries in dictionary order (the order in which
``Page.get_article_dict`` meets the ids); ``as_dict`` turns it into the {id: [(xs, ys), ...]} form run_eval works on.
The hypotheses are jittered and shifted copies of the ground truth with lines missing and extra, split and merged
articles, lines without an article id on either side, duplicated baselines and one line far from everything.
"""
import random

import textblock_cases as tc

MODES = {"dyn": (-1, -1), "fix": (10, 14), "fix_wide": (10, 30)}


def as_dict(side):
    return {k: [(list(xs), list(ys)) for xs, ys in polys] for k, polys in side}


def _group(lines, ids):
    out = {}
    for line, k in zip(lines, ids):
        out.setdefault(k, []).append([list(line[0]), list(line[1])])
    return [[k, v] for k, v in out.items()]


def make_pair(page, seed, per_article=9, drop=0.08, extra=2, none_every=11, jitter=(4, 9), regroup=7, far=True, dup=True):
    """GT: consecutive runs of ``per_article`` lines form an article, every ``none_every``-th line has no id.  HY: each
    line shifted by up to ``jitter`` px (x, y), dropped with probability ``drop``; articles regrouped in runs of
    ``regroup`` lines (splits and merges), some lines without id, ``extra`` invented lines, one far away, one duplicate."""
    rng = random.Random(seed)
    gt_ids = [None if none_every and i % none_every == none_every - 1 else "a%d" % (i // per_article) for i in range(len(page))]
    hy_lines, hy_ids = [], []
    for i, (xs, ys) in enumerate(page):
        if rng.random() < drop:
            continue
        dx, dy = rng.randint(-jitter[0], jitter[0]), rng.randint(-jitter[1], jitter[1])
        hy_lines.append(([x + dx for x in xs], [y + dy + rng.randint(-1, 1) for y in ys]))
        hy_ids.append(None if i % 13 == 5 else "h%d" % ((i + 3) // regroup))
    for _ in range(extra):
        x0, y0 = rng.randint(0, 900), rng.randint(0, 900)
        hy_lines.append(([x0, x0 + rng.randint(30, 200)], [y0, y0 + rng.randint(-4, 4)]))
        hy_ids.append("h0")
    if far:
        hy_lines.append(([20000, 20300], [30000, 30004]))
        hy_ids.append("hfar")
    if dup and hy_lines:
        hy_lines.append(hy_lines[1])
        hy_ids.append(hy_ids[1])
    return _group(page, gt_ids), _group(hy_lines, hy_ids)


def golden_cases(shift=0):
    """[(name, gt side, hy side, modes, record normed polygons?)].  ``shift`` is added to the jitter seeds: the generator
    takes, per case, the smallest shift whose alignments have no near ties (its docstring) and records it."""
    cases = []
    p = tc.columns_page(11, n_cols=2, n_lines=8, col_w=260)
    cases.append(("cols2", *make_pair(p, 1 + 100 * shift), ("dyn", "fix", "fix_wide"), False))
    p = tc.columns_page(12, n_cols=3, n_lines=10, col_w=220)
    cases.append(("cols3", *make_pair(p, 2 + 100 * shift, per_article=6, regroup=11), ("dyn", "fix"), False))
    p = tc.columns_page(13, n_cols=3, n_lines=9, col_w=180, gap=15, pitch=22)
    cases.append(("cols3_tight", *make_pair(p, 3 + 100 * shift, jitter=(3, 4)), ("dyn", "fix"), False))
    p = tc.random_page(14, 40, 1500, 2000, 200)
    cases.append(("scatter", *make_pair(p, 4 + 100 * shift, per_article=5, regroup=4), ("dyn", "fix"), False))
    p = tc.columns_page(15, n_cols=2, n_lines=6, col_w=200, extras=False)
    gt, hy = make_pair(p, 5 + 100 * shift)
    cases.append(("identical", gt, [[k, [list(map(list, q)) for q in v]] for k, v in gt], ("dyn", "fix"), False))
    cases.append(("gt_no_ids", [[None, [q for _, v in gt for q in v]]], hy, ("dyn", "fix"), False))
    cases.append(("hy_no_ids", gt, [[None, [q for _, v in hy for q in v]]], ("dyn", "fix"), False))
    cases.append(("hy_ids_only_none_gt", [[None, gt[0][1]], ["a0", gt[-1][1]]], hy, ("dyn",), False))
    cases.append(("empty_hy", gt, [], ("dyn", "fix"), False))
    cases.append(("empty_gt", [], hy, ("dyn", "fix"), False))
    cases.append(("one_each", [["a0", [[[100, 400], [200, 205]]]]], [["h0", [[[104, 390], [203, 207]]]]], ("dyn", "fix"), True))
    cases.append(("two_point_vertical", [["a0", [[[100, 100], [200, 500]], [[300, 301], [200, 500]]]], [None, [[[500, 700], [90, 90]]]]],
                  [["h0", [[[171, 173], [213, 480]]]], ["h1", [[[296, 300], [190, 505]], [[500, 690], [97, 95]]]]], ("dyn", "fix"), True))
    p = tc.columns_page(16, n_cols=4, n_lines=24, col_w=240, extras=False)
    cases.append(("cols4_100", *make_pair(p, 6 + 100 * shift, per_article=12, regroup=10), ("dyn",), False))
    p = tc.columns_page(17, n_cols=5, n_lines=40, col_w=240, extras=False)
    cases.append(("cols5_200", *make_pair(p, 7 + 100 * shift, per_article=20, regroup=17), ("dyn",), False))
    return cases


TIMED_ONLY = ("cols5_200",)       # run for profiles/measure/reference_cpu.json, not recorded in the golden

# name -> (cases in base-name order, as run_measure sorts them; (mode, verbose) runs whose stdout is recorded)
FILE_LISTS = {
    "mixed": (["cols2", "empty_gt", "empty_hy", "gt_no_ids", "hy_no_ids", "one_each"], [("dyn", True), ("dyn", False), ("fix", True)]),
    "plain": (["cols3", "two_point_vertical"], [("fix", False)]),
    "none_valid": (["empty_gt"], [("dyn", True)]),
}


def bench_pair(n_cols, n_lines, seed=7):
    """the benchmark pairs: n_cols * n_lines baselines in columns (200 = 5 x 40, 360 = 6 x 60, 1500 = 10 x 150)"""
    p = tc.columns_page(seed, n_cols=n_cols, n_lines=n_lines, col_w=240, extras=False)
    return make_pair(p, seed, per_article=20, regroup=17)
