"""The seam pages of tests/golden/textblock_seam_cases.py, checked on the reference side alone (no GPU): the
instrumented loop returns what slow_interline_distances returns, and every page reaches the seam it was built for -- the
lane pages have the scan lengths, the dense pages make the scan order matter, the tie pages meet each equality, the
neighbour cases hold an exact 0.95 * surface tie and a top-edge box on which int() and floor differ.  These are
conditions on the inputs: a case that misses one is mended, not the condition."""
import math
import os
import sys
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import textblock_cases as tc  # noqa: E402
import textblock_seam_cases as sc  # noqa: E402

CASES = sc.interline_cases()
NAMES = [n for n, _ in CASES]
_cache = {}


def _prepared(name):
    if name not in _cache:
        from citlab_article_separation_new_amd import textblock_geometry as geo
        page = dict(CASES)[name]
        polys = geo.norm_poly_dists(page, sc.DES_DIST)
        angles = [geo.calc_reg_line_angle(xs, ys) for xs, ys in polys]
        _cache[name] = sc.prepared(types.SimpleNamespace(polys=polys, angles=angles))
    return _cache[name]


def _counted(name, max_d):
    key = (name, max_d)
    if key not in _cache:
        normed, orient = _prepared(name)
        _cache[key] = sc.instrumented_interline_distances(normed, orient, sc.DES_DIST, max_d)
    return _cache[key]


@pytest.mark.parametrize("max_d", sc.MAX_DS)
@pytest.mark.parametrize("name", NAMES)
def test_instrumented_loop_equals_slow_loop(name, max_d):
    normed, orient = _prepared(name)
    assert _counted(name, max_d)[0] == tc.slow_interline_distances(normed, orient, sc.DES_DIST, max_d)


def test_norming_gives_the_point_counts_asked_for():
    from citlab_article_separation_new_amd import textblock_geometry as geo
    for k in (1, 2, 3, 13, 19, 20, 21, 32, 33, 64, 65):
        for line in (sc.hline(10, 20, k), sc.hline(10, 20, k, reverse=True), sc.vline(10, 20, k)):
            (xs, ys), = geo.norm_poly_dists([line], sc.DES_DIST)
            assert len(xs) == k == sc.normed_points(sc.length_for_points(k))
    # one point is the smallest polygon the norming gives (two identical points); an empty one is refused upstream
    assert min(len(xs) for name in NAMES for xs, _ in _prepared(name)[0]) == 1


def test_lane_pages_have_the_scan_lengths():
    lengths = {}
    for name, nb in sc.LANE_COUNTS.items():
        normed, _ = _prepared(name)
        assert len(normed) == nb, name
        lengths[name] = {len(xs) * nb for xs, _ in normed}
    assert sorted(set(sc.LANE_COUNTS.values())) == [1, 2, 3, 5, 63, 64, 65, 127, 128, 129]
    every = set().union(*lengths.values())
    assert sc.SCAN_LENGTHS <= every and any(t % 64 for t in every)
    # Nb = 64: the lanes never change polygon (64 % Nb == 0); Pa * Nb ends on a round for Pa = 1 and 2
    assert {64, 128} <= lengths["nb64"] and 63 in lengths["nb63"] and 65 in lengths["nb65"] and 128 in lengths["nb128"]
    assert 63 in lengths["nb3_pa21"] and 65 in lengths["nb5_pa13"] and lengths["nb2_pa32"] == {64}
    # and the lines see each other: nearly every line of the large pages has a neighbour below max_d
    for name in ("nb63", "nb64", "nb65", "nb127", "nb128", "nb129"):
        for max_d in sc.MAX_DS:
            d = _counted(name, max_d)[0]
            assert sum(v < max_d for v in d) >= 0.9 * len(d), (name, max_d)


@pytest.mark.parametrize("max_d", sc.MAX_DS)
@pytest.mark.parametrize("name", sc.DENSE)
def test_dense_pages_depend_on_the_scan_order(name, max_d):
    cnt = _counted(name, max_d)[1]
    assert cnt["skipped_would_lower"] >= 1 and cnt["rounds_reordered"] >= 1, cnt
    # stronger still: some skipped pair lies below the distance that is returned, so a scan that tested the box
    # against max_d alone returns another result
    assert cnt["skipped_below_result"] >= 1, cnt


def test_tie_pages_meet_the_equalities():
    for max_d in sc.MAX_DS:
        d, cnt = _counted("tie_same_off", max_d)
        assert cnt["eq_bd"] >= 1 and cnt["eq_m"] >= 1, cnt
        normed = _prepared("tie_same_off")[0]
        assert [v for (xs, _), v in zip(normed, d) if len(xs) <= 2] == [30.0] * 4      # exact: orientation (1, 0)
        d, cnt = _counted("tie_in_dist", max_d)
        assert cnt["eq_in"] >= 3, cnt
        assert d[0::2] == [10.0, 11.0, 12.0]            # the point at exactly 10 counts, the one at 11 does not
    for max_d in sc.MAX_DS:
        d, cnt = _counted("tie_max_d_%d" % max_d, max_d)
        assert cnt["eq_bd"] >= 1 and cnt["eq_m"] >= 1 and cnt["eq_max_d"] >= 1, cnt
        normed = _prepared("tie_max_d_%d" % max_d)[0]
        exact = [v for (xs, _), v in zip(normed, d) if len(xs) <= 2]
        assert exact == [max_d - 1.0] * 5 + [max_d] * 10 and all(type(v) is int for v in exact[5:])
    every = [_counted(n, m)[1] for n in sc.TIES for m in sc.MAX_DS]
    assert all(sum(c[k] for c in every) >= 1 for k in ("eq_bd", "eq_m", "eq_in", "eq_max_d"))


NEIGHBOUR_CASES = sc.neighbour_cases()


@pytest.mark.parametrize("case", NEIGHBOUR_CASES, ids=[c[0] for c in NEIGHBOUR_CASES])
def test_vectorised_neighbours_equal_slow_neighbours(case):
    _, normed, dists, avg = case
    boxes = sc.boxes_of(normed)
    assert sc.fast_neighbours(boxes, dists, avg, sc.FAC) == tc.slow_neighbours(boxes, dists, avg, sc.FAC)


def test_neighbour_cases_hold_the_edges():
    by_name = {c[0]: c[1:] for c in NEIGHBOUR_CASES}
    assert sorted(len(by_name["n%d" % n][0]) for n in (31, 32, 33, 64, 65)) == [31, 32, 33, 64, 65]
    # s12 == 0.95 * s2 as Python evaluates it: the pair is a neighbour by equality, one pixel further it is not
    normed, dists, avg = by_name["surface_tie"]
    boxes = sc.boxes_of(normed)
    assert 0.95 * 40 == 38.0 and sc.surface_equalities(boxes, dists, avg) == [(0, 1)]
    assert tc.slow_neighbours(boxes, dists, avg, sc.FAC) == [[1], [0], [], [], [5], [4]]
    # a box with y - fac * d negative and fractional: int() and floor differ, and so do the neighbour lists
    normed, dists, avg = by_name["top_edge"]
    boxes = sc.boxes_of(normed)
    v = boxes[0][1] - sc.FAC * dists[0]
    assert v < 0 and v != int(v) and int(v) == math.floor(v) + 1
    slow = tc.slow_neighbours(boxes, dists, avg, sc.FAC)
    assert slow != sc.slow_neighbours_floor(boxes, dists, avg, sc.FAC) and slow[0] == [1] and slow[6] == []
    # the other cases do not depend on the rounding direction (nothing there is negative)
    normed, dists, avg = by_name["n33"]
    boxes = sc.boxes_of(normed)
    assert tc.slow_neighbours(boxes, dists, avg, sc.FAC) == sc.slow_neighbours_floor(boxes, dists, avg, sc.FAC)


def test_grid_page_has_a_handful_of_neighbours_per_row():
    normed, dists, avg = sc.grid_neighbour_case()
    assert len(normed) == 2049 and (len(normed) + 31) // 32 > 64          # more words per row than threads per block
    rows = sc.fast_neighbours(sc.boxes_of(normed), dists, avg, sc.FAC)
    sizes = [len(r) for r in rows]
    assert min(sizes) >= 1 and max(sizes) <= 6 and sum(s >= 3 for s in sizes) > len(sizes) // 2
    assert any(j >= 2048 for r in rows for j in r) and rows[2048]           # the 65th word is used, and so is the last row
    assert len({j // 32 for r in rows for j in r}) == 65                    # every word of a row holds a bit somewhere
