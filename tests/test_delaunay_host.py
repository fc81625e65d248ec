"""The device triangulation's contract pinned on the CPU before any kernel runs (csrc/delaunay_kernels.h, --device_triangulation).

What scipy.spatial.Delaunay (Qhull, scipy 1.15) returns for the degenerate inputs, looked at before the kernel was written; the
kernel's rules mirror these and tests/test_delaunay_gpu.py holds it to them through check_triangulation:
  * exact duplicates: the later copies are in no simplex (they are listed in ``coplanar``), the first copy is a corner;
  * collinear points on the hull (two parallel baselines, a lattice's sides): every one is a corner of proper triangles, all
    simplices are strictly counter-clockwise (positive cross product in (x, y)), T = 2n - 2 - h with h counting them;
  * lattices (5 x 5, 3 x 40): every cell is split by one of its two diagonals, 32 and 156 triangles, no point left out;
  * all points on one line, or fewer than 3 distinct points among more than 3: QhullError ("initial simplex is flat").

The contract of --device_triangulation: the boundary of the alpha shape does not depend on how cocircular cells are split, unless a
circumradius lies within rounding of an alpha that is tried.  Here the existing numpy restatement of the boundary step
(tests/golden/alpha_shape_cases.py) runs on scipy's triangulation and on a second valid one made by flipping the diagonals of
cocircular quadrilaterals: same cycle, same retries.  Also the checker itself, the Python-side argument checks, the flag's
dependency on --device_regions, and the engine's table check in a stand-alone program under the sanitizers."""
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc")
for _p in (os.path.join(HERE, "golden"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import alpha_shape_cases as ac  # noqa: E402
import delaunay_cases as dcases  # noqa: E402
import delaunay_check as dc  # noqa: E402

MAX_RETRIES = 200
# articles of delaunay_cases.fuzz_articles() (480) that scipy's triangulation alone sets aside: a circumradius within 1e-9 relative
# of a tried alpha.  Counted on the CPU when the seeds were chosen; the cap is 5 % = 24.
FUZZ_SET_ASIDE = 1


def _scipy(points):
    from scipy.spatial import Delaunay
    tri = Delaunay(np.asarray(points))
    return np.ascontiguousarray(tri.simplices, np.int32), np.ascontiguousarray(tri.neighbors, np.int32)


# ---- what scipy does (the docstring's findings) ---------------------------------------------------------------------------

def test_scipy_on_degenerate_input():
    from scipy.spatial import Delaunay, QhullError
    dup = np.array([(0, 0), (10, 0), (0, 10), (10, 10), (10, 0), (5, 4), (5, 4)])
    tri = Delaunay(dup)
    assert sorted(set(tri.simplices.ravel().tolist())) == [0, 1, 2, 3, 5] and sorted(tri.coplanar[:, 0].tolist()) == [4, 6]
    dc.check_triangulation(dup, tri.simplices, tri.neighbors)
    for pts, n_tri in ((dcases.lattice(5, 5), 32), (dcases.lattice(40, 3), 156), (dcases.lattice(2, 40, 7)[:, ::-1], 78)):
        tri = Delaunay(pts)
        assert len(tri.simplices) == n_tri and len(tri.coplanar) == 0
        dc.check_triangulation(pts, tri.simplices, tri.neighbors)
    for pts in ([(0, 0), (5, 5), (10, 10), (20, 20)], [(0, 0), (5, 5), (0, 0), (5, 5)]):
        with pytest.raises(QhullError):
            Delaunay(np.array(pts))


# ---- the checker ----------------------------------------------------------------------------------------------------------

def test_checker_accepts_scipy():
    rng = np.random.RandomState(2)
    for n in (3, 4, 7, 50, 300):
        pts = rng.randint(0, 16000, (n, 2))
        dc.check_triangulation(pts, *_scipy(pts))
    pts = rng.randint(0, 10 ** 6, (40, 2))                # beyond the int64 range of the determinant: Python ints
    dc.check_triangulation(pts, *_scipy(pts))


def _quad():
    """(points, simplices, neighbors) of a convex quadrilateral split along 0-2, which is the Delaunay diagonal"""
    pts = np.array([(0, 0), (10, -4), (11, 0), (10, 4)])
    simp = np.array([(0, 1, 2), (0, 2, 3)])
    neigh = np.array([(-1, 1, -1), (-1, -1, 0)])
    return pts, simp, neigh


def test_checker_rejects_what_is_wrong():
    pts, simp, neigh = _quad()
    dc.check_triangulation(pts, simp, neigh)
    with pytest.raises(AssertionError, match="inside the circumcircle"):      # the other diagonal
        dc.check_triangulation(pts, np.array([(0, 1, 3), (1, 2, 3)]), np.array([(1, -1, -1), (-1, 0, -1)]))
    with pytest.raises(AssertionError, match="not counter-clockwise"):
        dc.check_triangulation(pts, np.array([(0, 2, 1), (0, 2, 3)]), neigh)
    for t, j, v in ((0, 1, -1), (0, 0, 1), (1, 2, 1)):
        bad = neigh.copy()
        bad[t, j] = v
        with pytest.raises(AssertionError, match="neighbors says"):
            dc.check_triangulation(pts, simp, bad)
    with pytest.raises(AssertionError):                                       # a triangle missing: the hull is not covered
        dc.check_triangulation(pts, simp[:1], np.array([(-1, -1, -1)]))
    far = np.concatenate([pts, [(30, 30)]])
    with pytest.raises(AssertionError, match="in no triangle"):
        dc.check_triangulation(far, simp, neigh)
    dup = np.concatenate([pts, pts[:1]])                                      # a duplicate may stay out ..
    dc.check_triangulation(dup, simp, neigh)
    with pytest.raises(AssertionError, match="same point"):                   # .. but not be a second corner
        dc.check_triangulation(dup, np.array([(0, 1, 2), (4, 2, 3)]), neigh)


def test_same_cycle_and_canonical_ring():
    from citlab_article_separation_new_amd import textblock
    a = [(0, 0), (4, 0), (4, 3), (0, 3)]
    assert dc.same_cycle(a, a[2:] + a[:2]) and dc.same_cycle(a, a[::-1]) and dc.same_cycle(a, (a[1:] + a[:1])[::-1])
    assert not dc.same_cycle(a, [a[0], a[2], a[1], a[3]]) and not dc.same_cycle(a, a[:3]) and dc.same_cycle([], [])
    assert not dc.same_cycle(a, a[:3] + [(0, 4)])
    for ring in (a, a[::-1], a[1:] + a[:1], [(5, 2), (1, 2), (3, 9)], [(5, 2), (3, 9), (1, 2)]):
        want = dc.canonical_ring(ring)
        assert dc.same_cycle(ring, want) and want[0] == min(ring, key=lambda p: (p[1], p[0]))
        n = len(want)
        assert sum(want[i][0] * want[(i + 1) % n][1] - want[(i + 1) % n][0] * want[i][1] for i in range(n)) > 0
        closed = [list(p) for p in ring] + [list(ring[0])]
        assert textblock.canonical_ring(closed) == [list(p) for p in want] + [list(want[0])]


def test_flip_gives_another_valid_triangulation():
    pts = dcases.lattice(5, 5)
    simp, neigh = _scipy(pts)
    s2, n2, flips = dc.flip_cocircular(pts, simp, neigh)
    assert flips >= 8 and dc.triangle_set(s2) != dc.triangle_set(simp)
    dc.check_triangulation(pts, s2, n2)
    rng = np.random.RandomState(4)
    gp = rng.randint(0, 16000, (60, 2))                   # general position: nothing to flip
    simp, neigh = _scipy(gp)
    s2, n2, flips = dc.flip_cocircular(gp, simp, neigh)
    assert flips == 0 and np.array_equal(s2, simp) and np.array_equal(n2, neigh)


# ---- the contract ---------------------------------------------------------------------------------------------------------

def _contract(cases, check_tables):
    """per case: scipy's triangulation and a flipped one through the restated boundary step.  Returns (articles compared, articles
    set aside, articles where a diagonal was flipped)."""
    compared = aside = flipped = 0
    for k, (name, pts, alpha) in enumerate(cases):
        pts = np.asarray(pts)
        if len(pts) <= 3:
            continue
        simp, neigh = _scipy(pts)
        ring, retries, failed, circ, _ = ac.restated(pts, simp, neigh, alpha, MAX_RETRIES)
        assert not failed, name
        if dcases.near_tried_alpha(circ, alpha, retries):
            aside += 1
            continue
        s2, n2, flips = dc.flip_cocircular(pts, simp, neigh, np.random.RandomState(k))
        if check_tables:
            dc.check_triangulation(pts, s2, n2)
        ring2, retries2, failed2, circ2, _ = ac.restated(pts, s2, n2, alpha, MAX_RETRIES)
        assert not dcases.near_tried_alpha(circ2, alpha, retries2), name      # the flipped cells have the same circumcircles
        assert not failed2 and retries2 == retries, (name, retries, retries2)
        assert dc.same_cycle(pts[ring], pts[ring2]), name
        compared += 1
        flipped += flips > 0
    return compared, aside, flipped


def test_contract_on_fuzz():
    cases = dcases.fuzz_articles()
    assert len(cases) == 480
    compared, aside, flipped = _contract(cases, True)
    print("fuzz: compared %d, set aside %d, with flips %d" % (compared, aside, flipped))
    assert aside == FUZZ_SET_ASIDE and aside <= 0.05 * len(cases)
    assert compared + aside == len(cases) and flipped >= 150


def test_contract_on_golden_pages():
    cases = [c for c in ac.golden_articles() if len(c[1]) > 3]
    compared, aside, flipped = _contract(cases, False)
    print("golden: compared %d, set aside %d, with flips %d" % (compared, aside, flipped))
    assert compared >= 40 and aside == 0


# ---- Python-side validation and the flag ------------------------------------------------------------------------------------

def test_flag_needs_device_regions(capsys):
    from citlab_article_separation_new_amd import run_textregion_generation as rtg, textblock
    assert rtg.build_parser().parse_known_args([])[0].device_triangulation is False
    flags = rtg.parse_flags(["--device_regions", "True", "--device_triangulation", "True"])
    assert flags.device_regions is True and flags.device_triangulation is True
    assert rtg.parse_flags(["--device_regions", "True"]).device_triangulation is False
    for argv in (["--device_triangulation", "True"], ["--device_regions", "False", "--device_triangulation", "True"]):
        with pytest.raises(SystemExit) as e:
            rtg.parse_flags(argv)
        assert e.value.code == 2
        assert "--device_triangulation True needs --device_regions True" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        rtg.main(["--path_to_xml_lst", "nowhere.lst", "--device_triangulation", "True"])
    assert inspect.signature(textblock.create_text_regions).parameters["device_triangulation"].default is False
    assert inspect.signature(textblock.create_text_regions_pages).parameters["device_triangulation"].default is False
    with pytest.raises(ValueError, match="device_triangulation needs device_regions"):
        textblock.create_text_regions({}, {}, 75, device_triangulation=True)


def test_python_argument_checks():
    from citlab_article_separation_new_amd import textblock
    off, pts = textblock._packed_points("f", [np.array([(1, 2), (3, 4)]), np.zeros((0, 2), int), np.array([(-5, 6)])])
    assert off.tolist() == [0, 2, 2, 3] and off.dtype == np.int32 and pts.tolist() == [[1, 2], [3, 4], [-5, 6]]
    assert textblock._packed_points("f", [])[1].shape == (1, 2)
    for bad in (np.zeros((4, 3), int), np.zeros(4, int), np.array([(0, 2 ** 31)]), np.array([(-2 ** 31 - 1, 0)]), np.zeros((4, 2))):
        with pytest.raises(ValueError, match="f: article 1 needs"):
            textblock._packed_points("f", [np.zeros((3, 2), int), bad])


def test_abi_entries():
    from citlab_article_separation_new_amd import _lib
    header = open(os.path.join(ROOT, "include", "asep_hip.h")).read()
    for name in ("asep_delaunay", "asep_alpha_shapes_points", "asep_delaunay_last_kernel_us", "asep_delaunay_lds_points",
                 "asep_delaunay_max_extent"):
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["asep_delaunay"][1]) == 9 and len(_lib.SIGNATURES["asep_alpha_shapes_points"][1]) == 12


# ---- the engine's table check, stand-alone under the sanitizers -------------------------------------------------------------

def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_table_check_accepts_and_refuses(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++, c++ or clang++) on PATH")
    exe = str(tmp_path / "delaunay_tables_check")
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover",
           *([] if is_clang else ["-static-libasan", "-static-libubsan"]), "-I", CSRC,
           os.path.join(HERE, "delaunay_tables_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert ran.stdout.startswith("delaunay tables ok:"), ran.stdout
