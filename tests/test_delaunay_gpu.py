"""The Delaunay triangulation on the GPU (asep_delaunay, asep_alpha_shapes_points, --device_triangulation).  Every table that comes
back goes through tests/delaunay_check.py::check_triangulation, exactly in integers: the named shapes of
tests/golden/delaunay_cases.py (3 points, cocircular squares and lattices, collinear hull edges, one baseline, 2 points, duplicates, a
box at the coordinate bound and one pixel over it, the LDS point bound and one point over it), random sets against scipy's set of
triangles, 200 articles in one call against one per call, the refusals; the alpha shapes from points against asep_alpha_shapes fed
with scipy's tables on the golden pages' articles and the fuzz of tests/test_delaunay_host.py (same cycle, retries, failed); the
regions of create_text_regions and of the command line against the host function's, as cycles.  What scipy does with the degenerate
inputs is recorded in tests/test_delaunay_host.py.  Every GPU step runs in a child process (this file, run as a script) under a time
limit."""
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(HERE, "golden"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _child(check, *args, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), check, *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, f"{check} failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def test_named_shapes_random_sets_and_refusals():
    assert "ok" in _child("tables")


def test_batch_equals_one_per_call():
    assert "ok" in _child("batch")


def test_alpha_shapes_from_points():
    assert "ok" in _child("alpha")


def test_create_text_regions():
    assert "ok" in _child("regions")


def test_command_line_same_polygons(tmp_path):
    assert "ok" in _child("cli", str(tmp_path), timeout=600)


# ---- the checks, run in the child -------------------------------------------------------------------------------------

def _checked(pts, got, want_status, name):
    """one article's result: the status, and tables that are a Delaunay triangulation of the points (or none)"""
    import delaunay_check as dc
    simp, neigh, status = got
    assert status == want_status, (name, status, want_status)
    if status != 0:
        assert len(simp) == 0 and len(neigh) == 0, name
        return
    try:
        dc.check_triangulation(pts, simp, neigh)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (name, e))


def check_tables():
    import numpy as np
    from scipy.spatial import Delaunay
    import delaunay_cases as dcases
    import delaunay_check as dc
    from citlab_article_separation_new_amd import _lib, textblock
    lds, ext = textblock.delaunay_lds_points(), textblock.delaunay_max_extent()
    assert 256 <= lds <= 4096 and ext == 2 ** 14 - 1
    shapes = dcases.shapes(lds, ext)
    assert [len(p) for n, p, _ in shapes if n.startswith("lds_points")] == [lds, lds + 1]
    for name, pts, status in shapes:                       # one article per call ..
        _checked(pts, textblock.delaunay_device([pts])[0], status, name)
    got = textblock.delaunay_device([p for _, p, _ in shapes])      # .. and all in one
    for (name, pts, status), g in zip(shapes, got):
        _checked(pts, g, status, name + " (in one call)")
    assert textblock.last_delaunay_kernel_us() > 0
    by_name = {n: g for (n, _, _), g in zip(shapes, got)}
    assert len(by_name["three_points"][0]) == 1 and len(by_name["square"][0]) == 2 and len(by_name["one_inside"][0]) == 3
    assert len(by_name["lattice_5x5"][0]) == 32 and len(by_name["lattice_3x40"][0]) == 156 and len(by_name["two_baselines"][0]) == 78
    dup = next(p for n, p, _ in shapes if n == "duplicates")
    assert sorted(set(by_name["duplicates"][0].ravel().tolist())) == [0, 1, 2, 3, 5]          # the first of equal points, as scipy
    assert sorted(set(Delaunay(dup).simplices.ravel().tolist())) == [0, 1, 2, 3, 5]
    # general position: the triangulation is unique, so the set of triangles is scipy's
    rng = np.random.RandomState(21)
    for n in (50, 300):
        while True:
            pts = rng.randint(0, ext + 1, (n, 2))
            if len(np.unique(pts, axis=0)) == n:
                break
        simp, neigh, status = textblock.delaunay_device([pts])[0]
        _checked(pts, (simp, neigh, status), 0, "random %d" % n)
        tri = Delaunay(pts)
        dc.check_triangulation(pts, tri.simplices, tri.neighbors)
        assert dc.triangle_set(simp) == dc.triangle_set(tri.simplices), n
    # empty calls and refusals
    assert textblock.delaunay_device([]) == []
    assert [g[2] for g in textblock.delaunay_device([np.zeros((0, 2), int), np.array([(1, 1)])])] == [1, 1]
    lib, h = textblock._handle(0)
    pt_off, cap_off = np.array([0, 4, 8], np.int32), np.array([0, 8, 10], np.int32)
    pts = np.zeros((8, 2), np.int32)
    out = np.zeros((10, 3), np.int32)
    res = np.zeros((2, 2), np.int32)
    P = textblock._ptr
    rc = lib.asep_delaunay(h, 2, P(pt_off), P(pts), P(cap_off), P(out), P(out.copy()), P(res[0]), P(res[1]))
    assert rc == -1 and "asep_delaunay: article 1 has room for 2 triangles, its 4 points can give 3" in _lib.last_error()
    rc = lib.asep_delaunay(h, 2, P(np.array([0, 4, 3], np.int32)), P(pts), P(cap_off), P(out), P(out.copy()), P(res[0]), P(res[1]))
    assert rc == -1 and "pt_off 1 (4 -> 3) is decreasing" in _lib.last_error()
    rc = lib.asep_delaunay(h, 2, P(pt_off), P(pts), P(np.array([0, 8, 16], np.int32)), None, None, P(res[0]), P(res[1]))
    assert rc == -1 and "null argument" in _lib.last_error()
    _checked(shapes[2][1], textblock.delaunay_device([shapes[2][1]])[0], 0, "after the refusals")
    print("ok")


def _mixed_articles(count, seed):
    import numpy as np
    import delaunay_cases as dcases
    rng = np.random.RandomState(seed)
    arts = []
    for k in range(count):
        n = int(rng.randint(3, 121))
        kind = k % 5
        if kind == 0:
            pts = rng.randint(0, 2000, (n, 2))
        elif kind == 1:
            pts = rng.randint(0, 7, (n, 2)) * 9                                # a lattice with duplicates
        elif kind == 2:
            pts = dcases.lattice(int(rng.randint(2, 12)), int(rng.randint(2, 6)), 5, int(rng.randint(-99, 99)), 3)
        elif kind == 3:
            pts = np.array([(4 * i, 7) for i in range(n)])                     # one line: status 2
        else:
            pts = np.concatenate([rng.randint(0, 50, (n, 2)), [(0, 0), (17000, 3)]])      # too wide: status 3
        arts.append(np.asarray(pts, np.int64))
    return arts


def check_batch():
    import numpy as np
    from citlab_article_separation_new_amd import textblock
    arts = _mixed_articles(200, 33)
    lds = textblock.delaunay_lds_points()
    arts[57] = np.random.RandomState(1).randint(0, 3000, (lds + 40, 2))        # one article in global scratch among them
    together = textblock.delaunay_device(arts)
    statuses = [g[2] for g in together]
    assert statuses.count(0) >= 100 and statuses.count(2) >= 30 and statuses.count(3) >= 30
    for k, (pts, g) in enumerate(zip(arts, together)):
        _checked(pts, g, g[2], "article %d" % k)
        alone = textblock.delaunay_device([pts])[0]
        assert alone[2] == g[2] and np.array_equal(alone[0], g[0]) and np.array_equal(alone[1], g[1]), k
    again = textblock.delaunay_device(arts[::-1])[::-1]                         # and in another order
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(again, together))
    print("ok")


def check_alpha():
    import numpy as np
    import alpha_shape_cases as ac
    import delaunay_cases as dcases
    import delaunay_check as dc
    from test_delaunay_host import MAX_RETRIES
    from citlab_article_separation_new_amd import textblock
    cases = [c for c in ac.golden_articles() if len(c[1]) > 3] + dcases.fuzz_articles() + ac.named_cases()
    arts, aside = [], 0
    for name, pts, alpha in cases:
        p, simp, neigh = textblock.triangulate(np.asarray(pts))
        circ = ac.circum_r(p, simp)
        arts.append((name, p, simp, neigh, float(alpha), circ))
    pages = lambda rows: [rows[i:i + 31] for i in range(0, len(rows), 31)] + [[]]      # noqa: E731
    want = [g for pg in textblock.alpha_shapes_device(pages([a[1:5] for a in arts]), MAX_RETRIES + 1) for g in pg]
    got = [g for pg in textblock.alpha_shapes_points_device(pages([(a[1], a[4]) for a in arts]), MAX_RETRIES + 1) for g in pg]
    assert len(want) == len(got) == len(arts)
    for (name, p, _, _, alpha, circ), w, g in zip(arts, want, got):
        assert g[3] == 0, (name, g[3])
        if dcases.near_tried_alpha(circ, alpha, w[1]):
            aside += 1
            continue
        assert g[1] == w[1] and g[2] == w[2], (name, g[1:3], w[1:3])
        assert dc.same_cycle(p[w[0]], p[g[0]]), name
    assert aside <= 1, aside                                # the one article tests/test_delaunay_host.py records
    assert max(w[1] for w in want) >= 14 and not any(w[2] for w in want)
    assert textblock.last_delaunay_kernel_us() > 0 and textblock.last_alpha_shape_kernel_us(1) > 0
    # a failing article between others: five retries allowed, the sliver never closes; and the statuses of what is not triangulated
    sliver = np.array(ac.sliver_points())
    line = np.array([(3 * i, 2 * i) for i in range(9)])
    wide = np.array([(0, 0), (20000, 5), (7, 9), (100, 300)])
    quad = np.asarray(ac.named_cases()[0][1])
    got = textblock.alpha_shapes_points_device([[(quad, 75.0), (sliver, 75.0)], [(line, 75.0), (wide, 75.0), (quad, 75.0)], []], 5)
    assert [g[3] for pg in got for g in pg] == [0, 3, 2, 3, 0]              # (the sliver's box is over the bound too)
    assert [g[2] for pg in got for g in pg] == [False, True, True, True, False]
    assert all(len(g[0]) == 0 and g[1] == 5 for pg in got for g in pg if g[2])
    assert dc.same_cycle(quad[got[0][0][0]], quad) and dc.same_cycle(quad[got[1][2][0]], quad)
    assert textblock.alpha_shapes_points_device([]) == [] and textblock.alpha_shapes_points_device([[], []]) == [[], []]
    print("ok")


def _page_inputs(page):
    """what create_text_regions reads for a page of baselines, as run_textregion_generation builds it"""
    from citlab_article_separation_new_amd import textblock, textblock_geometry as geo
    labels, _ = textblock.cluster_baselines([page])[0]
    art = {}
    for i, lab in enumerate(labels):
        art.setdefault("a%d" % lab, []).append("l%d" % i)
    n50 = geo.norm_poly_dists(page, 50)
    d_tr = textblock.interline_distances(textblock.normed_pages([page], 5), 5, 100)[0]
    return art, {"l%d" % i: (p, v) for i, (p, v) in enumerate(zip(n50, d_tr.tolist()))}


def _same_regions(got, want):
    import delaunay_check as dc
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g[0], g[2], g[3]) == (w[0], w[2], w[3])
        assert g[1][0] == g[1][-1] and w[1][0] == w[1][-1]
        assert dc.same_cycle(g[1][:-1], w[1][:-1]), g[0]
        if len(g[1]) > 4:                                   # an alpha shape: in the canonical form
            assert [tuple(p) for p in g[1][:-1]] == dc.canonical_ring(w[1][:-1]), g[0]


def check_regions():
    import numpy as np
    from scipy.spatial import QhullError
    import alpha_shape_cases as ac
    import delaunay_cases as dcases
    import textblock_cases as tc
    from citlab_article_separation_new_amd import textblock
    for seed in (61, 62):
        art, geom = _page_inputs(tc.columns_page(seed, n_cols=2, n_lines=8, col_w=300, pitch=40))
        h_log, d_log = [], []
        want = textblock.create_text_regions(art, geom, 30, h_log.append)
        got = textblock.create_text_regions(art, geom, 30, d_log.append, device_regions=True, device_triangulation=True)
        assert len(want) >= 2 and h_log == d_log
        _same_regions(got, want)
    # hand-made jobs: what the device flags takes the host function and still appears; an article Qhull refuses ends its page
    wide = dcases.lattice(6, 3, 3300)                       # 16,500 px wide: over the bound
    jobs = [[(np.array([(0, 0), (9, 0), (4, 4)]), ["l0"]), (dcases.lattice(6, 4), ["l1"]), (wide, ["l2"]),
             (np.asarray(ac.named_cases()[3][1]), ["l3", "l4"]), (np.array([(0, 0), (10, 0), (0, 10), (10, 10), (10, 0), (5, 4)]), ["l5"])],
            [(dcases.lattice(3, 3), ["l0"]), (np.array([(2 * i, 3 * i) for i in range(6)]), ["l1"]), (dcases.lattice(2, 2), ["l2"])],
            [(np.array([(1, 1), (5, 5), (1, 1), (5, 5)]), ["l0"])]]
    textblock._region_jobs = lambda art_lines, geom, alpha: (art_lines, None)
    logs = [[], [], []]
    got = textblock.create_text_regions_pages([(j, {}) for j in jobs], 10.0, [lg.append for lg in logs], device_triangulation=True)
    want_log = []
    want = [("tr_%d" % i, textblock.alpha_shape_int(p, 10.0, want_log.append), m, i) for i, (p, m) in enumerate(jobs[0])]
    _same_regions(got[0], want)
    assert logs[0] == want_log and len(want_log) > 5 and got[0][2][1] == textblock.canonical_ring(want[2][1])
    assert isinstance(got[1], QhullError) and isinstance(got[2], QhullError)
    # an article over DEVICE_TRIANGULATION_MAX_POINTS takes the host function too; one of exactly that size stays on the device
    assert textblock.DEVICE_TRIANGULATION_MAX_POINTS == 4096
    textblock.DEVICE_TRIANGULATION_MAX_POINTS = 18
    sent = []
    inner = textblock.alpha_shapes_points_device
    textblock.alpha_shapes_points_device = lambda pages, *a: sent.append([len(p) for pg in pages for p, _ in pg]) or inner(pages, *a)
    got = textblock.create_text_regions_pages([(jobs[0], {})], 10.0, [lambda s: None], device_triangulation=True)
    assert sent == [[18, 18, 6]]                            # the 24 points of the lattice stay on the host, 18 points do not
    _same_regions(got[0], want)
    with pytest.raises(QhullError):
        textblock.alpha_shape_int(jobs[1][1][0], 10.0)
    print("ok")


def _regions_of(path):
    """{region id: [(x, y), ...]} of a PAGE-XML file, the closing point dropped"""
    import xml.etree.ElementTree as ET
    out = {}
    for el in ET.parse(path).getroot().iter():
        if el.tag.endswith("}TextRegion") or el.tag == "TextRegion":
            coords = next(c for c in el if c.tag.endswith("Coords"))
            pts = [tuple(int(v) for v in p.split(",")) for p in coords.get("points").split()]
            out[el.get("id")] = pts[:-1] if len(pts) > 1 and pts[0] == pts[-1] else pts
    return out


def check_cli(tmp):
    import delaunay_check as dc
    import textblock_cases as tc
    from test_textblock_gpu import _baseline_page
    data = os.path.join(tmp, "page")
    os.makedirs(data)
    paths = []
    for k, seed in enumerate((51, 52)):
        p = os.path.join(data, "p%d.xml" % k)
        _baseline_page(p, "p%d.png" % k, 1400, 1300, tc.columns_page(seed, n_cols=3, n_lines=10, col_w=300, pitch=40))
        paths.append(p)
    lst = os.path.join(tmp, "pages.lst")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(mod, *args, rc=0):
        r = subprocess.run([sys.executable, "-m", "citlab_article_separation_new_amd." + mod, *args], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == rc, f"{mod}: {r.stdout[-3000:]}\n{r.stderr[-3000:]}"
        return r.stdout
    run("run_baseline_clustering", "--path_to_xml_lst", lst)
    keep = os.path.join(tmp, "clustered")
    shutil.copytree(data, keep)
    out, regions = {}, {}
    for name, extra in (("host", []), ("device", ["--device_regions", "True", "--device_triangulation", "True"])):
        for p in paths:
            shutil.copyfile(os.path.join(keep, os.path.basename(p)), p)
        out[name] = run("run_textregion_generation", "--path_to_xml_lst", lst, "--alpha", "30", *extra)
        regions[name] = [_regions_of(p) for p in paths]
    assert out["host"] == out["device"] and "saving errors:" in out["host"]
    for h, d in zip(regions["host"], regions["device"]):
        assert sorted(h) == sorted(d) and "tr_1" in h
        for rid in h:
            assert dc.same_cycle(h[rid], d[rid]), rid
            if len(d[rid]) > 3:
                assert d[rid] == dc.canonical_ring(h[rid]), rid
    run("run_textregion_generation", "--path_to_xml_lst", lst, "--device_triangulation", "True", rc=2)
    print("ok", out["host"].count("alpha value not suitable"))


if __name__ == "__main__":
    {"tables": check_tables, "batch": check_batch, "alpha": check_alpha, "regions": check_regions,
     "cli": lambda: check_cli(sys.argv[2])}[sys.argv[1]]()
