"""The two text block kernels at their seams (tests/golden/textblock_seam_cases.py): pages whose line and point counts put
the ends of the distance kernel's 64-lane rounds everywhere (Nb 1..129, scan lengths 63, 64, 65, 128), dense columns on
which the order of the scan decides the result, exact ties of every comparison, pages of very different sizes in one
launch; neighbour rows of 31..65 and of 2049 lines (more words than threads), an exact 0.95 * surface tie and boxes at
the top edge.  Every result is compared with == against the loop-for-loop restatement in textblock_cases.py; that the
pages reach these seams is checked without a GPU in test_textblock_seams_host.py.  Every GPU step runs in a child process
(this file, run as a script) under a time limit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _child(check, *args, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), check, *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, f"{check} failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


@pytest.mark.parametrize("max_d", (500, 100))
def test_interline_page_by_page(max_d):
    assert "ok" in _child("single", str(max_d))


@pytest.mark.parametrize("max_d", (500, 100))
def test_interline_pages_of_mixed_sizes_in_one_launch(max_d):
    assert "ok" in _child("batched", str(max_d))


def test_neighbours_small_pages_and_edges():
    assert "ok" in _child("neighbours")


def test_neighbours_page_of_2049_lines():
    assert "ok" in _child("neighbours_grid")


# ---- the checks, run in the child -------------------------------------------------------------------------------------

def _normed_and_slow(max_d, extra=()):
    """[(name, NormedPage, the slow loop's distances)] for the seam cases and the `extra` (name, page) entries"""
    import textblock_cases as tc
    import textblock_seam_cases as sc
    from citlab_article_separation_new_amd import textblock
    named = sc.interline_cases() + list(extra)
    pages = textblock.normed_pages([p for _, p in named], sc.DES_DIST)
    return [(name, pg, tc.slow_interline_distances(*sc.prepared(pg), sc.DES_DIST, max_d)) for (name, _), pg in zip(named, pages)]


def check_single(max_d):
    import textblock_seam_cases as sc
    from citlab_article_separation_new_amd import textblock
    n = 0
    for name, pg, want in _normed_and_slow(max_d):
        got = textblock.interline_distances([pg], sc.DES_DIST, max_d)[0].tolist()
        assert got == want, (name, max_d, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
        assert textblock.last_kernel_us(0) > 0
        n += len(want)
    print("ok", n, "lines")


def check_batched(max_d):
    import textblock_seam_cases as sc
    from citlab_article_separation_new_amd import textblock
    cases = _normed_and_slow(max_d, [("empty", sc.EMPTY_PAGE), ("one_line", sc.ONE_LINE_PAGE)])
    by_name = {name: (name, pg, want) for name, pg, want in cases}
    listed = cases[:-2]
    # reversed, with the empty and the one-line page between the large ones
    mixed = []
    for c in reversed(listed):
        mixed.append(c)
        if c[0] == "nb129":
            mixed.append(by_name["empty"])
        if c[0] == "nb128":
            mixed.append(by_name["one_line"])
    assert [c[0] for c in mixed][-14:-9] == ["nb129", "empty", "nb128", "one_line", "nb127"], [c[0] for c in mixed]
    single = {name: textblock.interline_distances([pg], sc.DES_DIST, max_d)[0].tolist() for name, pg, _ in cases}
    assert single["empty"] == [] and single["one_line"] == [max_d]
    for order in (listed, mixed):
        got = [d.tolist() for d in textblock.interline_distances([pg for _, pg, _ in order], sc.DES_DIST, max_d)]
        for (name, _, want), g in zip(order, got):
            assert g == want, (name, max_d, "batched != slow loop")
            assert g == single[name], (name, max_d, "batched != page by page")
    print("ok", len(listed), len(mixed))


def _neighbour_inputs(case):
    from citlab_article_separation_new_amd import textblock
    _, normed, dists, avg = case
    return textblock.NormedPage(normed), dists, avg


def check_neighbours():
    import textblock_cases as tc
    import textblock_seam_cases as sc
    from citlab_article_separation_new_amd import textblock
    cases = sc.neighbour_cases()
    assert [c[0] for c in cases] == ["n31", "n32", "n33", "n64", "n65", "surface_tie", "top_edge"]
    inputs = [_neighbour_inputs(c) for c in cases]
    want = []
    for (name, normed, dists, avg), (pg, _, _) in zip(cases, inputs):
        boxes = [tuple(int(v) for v in b) for b in pg.boxes]
        assert boxes == sc.boxes_of(normed)
        want.append(tc.slow_neighbours(boxes, dists, avg, sc.FAC))
        assert textblock.neighbour_lists([pg], [dists], [avg], sc.FAC)[0] == want[-1], name
        assert textblock.last_kernel_us(1) > 0
    for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
        got = textblock.neighbour_lists([inputs[k][0] for k in order], [inputs[k][1] for k in order],
                                        [inputs[k][2] for k in order], sc.FAC)
        assert got == [want[k] for k in order], order
    print("ok")


def check_neighbours_grid():
    import textblock_cases as tc
    import textblock_seam_cases as sc
    from citlab_article_separation_new_amd import textblock
    small = sc.neighbour_cases()
    for name, normed, dists, avg in small:                # the vectorised yardstick is the slow one on the small cases
        boxes = sc.boxes_of(normed)
        assert sc.fast_neighbours(boxes, dists, avg, sc.FAC) == tc.slow_neighbours(boxes, dists, avg, sc.FAC), name
    grid = ("grid", *sc.grid_neighbour_case())
    assert len(grid[1]) == 2049
    pg, dists, avg = _neighbour_inputs(grid)
    want = sc.fast_neighbours([tuple(int(v) for v in b) for b in pg.boxes], dists, avg, sc.FAC)
    got = textblock.neighbour_lists([pg], [dists], [avg], sc.FAC)[0]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    # between two small pages: the large page's rows start at a word offset (bits_off) and a row index that are not 0
    by_name = {c[0]: c for c in small}
    trio = [by_name["n33"], grid, by_name["top_edge"]]
    inputs = [_neighbour_inputs(c) for c in trio]
    got = textblock.neighbour_lists([i[0] for i in inputs], [i[1] for i in inputs], [i[2] for i in inputs], sc.FAC)
    assert got[1] == want, "the 2049-line page differs inside a batch"
    for k in (0, 2):
        _, normed, d, a = trio[k]
        assert got[k] == tc.slow_neighbours(sc.boxes_of(normed), d, a, sc.FAC), trio[k][0]
    print("ok", sum(len(r) for r in want), "neighbours")


if __name__ == "__main__":
    name = sys.argv[1]
    {"single": lambda: check_single(int(sys.argv[2])), "batched": lambda: check_batched(int(sys.argv[2])),
     "neighbours": check_neighbours, "neighbours_grid": check_neighbours_grid}[name]()
