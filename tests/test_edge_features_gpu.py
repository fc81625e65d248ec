"""The edge feature engine (asep_edge_features_run, edge_features.py) against the host functions of feature_generation.py: separator
flags under both rules, edge hulls, pair bits and the masked confidences.  Every comparison is exact equality.

The `bb` rule, the pair rules, the hulls and the masked matrices are pinned to the REFERENCE through tests/golden/host_goldens.json (read
only).  The `line` rule is pinned by this repository's restatement alone (feature_generation.get_edge_separator_feature_line): the reference's
own needs shapely, which the build image lacks, so there is no reference run of it."""
import ctypes as C
import itertools
import json
import os
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(ROOT, "tests", "golden", "host_goldens.json")))


class _Region:
    def __init__(self, points, region_type=None, rid="r"):
        self.id, self.points, self.region_type = rid, [tuple(p) for p in points], region_type


class _Sep:
    def __init__(self, points, orientation=None):
        self.points, self._o = [tuple(p) for p in points], orientation

    def get_orientation(self):
        return self._o


def _golden_page(rec):
    return ([_Region(s["points"], s["type"], s["id"]) for s in rec["regions"]],
            [_Sep(s["points"], s["orientation"]) for s in rec["separators"]])


def _fully(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]


def _host(fg, regions, seps, edges, rule):
    fn = fg.get_edge_separator_feature_line if rule == "line" else fg.get_edge_separator_feature_bb
    return np.array([fn(regions[a], regions[b], seps) if seps else [0.0, 0.0] for a, b in edges], np.float64).reshape(-1, 2)


def _host_hulls(fg, regions, edges):
    return [[list(p) for p in fg.get_edge_visual_region(regions[a], regions[b])] for a, b in edges]


def _device_hulls(res):
    assert not res["hull"][np.arange(res["hull"].shape[1])[None, :] >= res["hull_n"][:, None]].any()      # zero behind the count
    return [res["hull"][e, :n].tolist() for e, n in enumerate(res["hull_n"])]


def _host_pair_bits(fg, regions, seps):
    n = len(regions)
    bits = np.zeros((n, n), np.uint8)
    for i in range(n):
        for j in range(i + 1, n):
            b = (1 if fg.is_aligned_heading_separated(regions[i], regions[j]) else 0) | \
                (2 if fg.is_aligned_horizontally_separated(regions[i], regions[j], seps) else 0)
            bits[i, j] = bits[j, i] = b
    return bits


def _check_pages(fg, ef, pages, rule, results=None, hulls=True, pair_bits=True):
    """every page of one call against the host functions -> the results"""
    if results is None:
        results = ef.edge_features_device(pages, rule=rule, hulls=hulls, pair_bits=pair_bits)
    assert len(results) == len(pages)
    for k, (page, res) in enumerate(zip(pages, results)):
        edges = page.edges.tolist()
        assert res["flags"].dtype == np.uint8 and res["flags"].shape == (len(edges), 2)
        assert np.array_equal(res["flags"].astype(np.float64), _host(fg, page.text_regions, page.separator_regions, edges, rule)), (k, rule)
        if hulls:
            assert _device_hulls(res) == _host_hulls(fg, page.text_regions, edges), k
        if pair_bits:
            assert np.array_equal(res["pair_bits"], _host_pair_bits(fg, page.text_regions, page.separator_regions)), k
    return results


def test_reference_fixture_in_one_call(monkeypatch):
    """the six pages of the reference fixture (one without separators, one of three regions) in ONE call"""
    from citlab_article_separation_new_amd import edge_features as ef, feature_generation as fg
    assert len(G["pages"]) == 6
    built = [_golden_page(rec) for rec in G["pages"]]
    assert any(not seps for _, seps in built) and any(len(regions) == 3 for regions, _ in built)
    pages = [ef.EdgePage(regions, seps, [(pr["i"], pr["j"]) for pr in rec["pairs"]]) for rec, (regions, seps) in zip(G["pages"], built)]
    results = ef.edge_features_device(pages, rule="bb", hulls=True, pair_bits=True)
    assert ef.last_kernel_us > 0
    for rec, res in zip(G["pages"], results):
        assert res["flags"].astype(np.float64).tolist() == [pr["separator_bb"] for pr in rec["pairs"]]
        assert _device_hulls(res) == [pr["edge_visual_region"] for pr in rec["pairs"]]
        bits = res["pair_bits"]
        assert not np.diag(bits).any() and np.array_equal(bits, bits.T)
        for pr in rec["pairs"]:
            want = (1 if pr["aligned_heading_separated"] else 0) | (2 if pr["aligned_horizontally_separated"] else 0)
            assert bits[pr["i"], pr["j"]] == want and bits[pr["j"], pr["i"]] == want, (pr["i"], pr["j"])
    # the masked matrices, values and dtype, through the public switch (Page patched the way tests/test_host_goldens.py does)
    for rec, (regions, seps) in zip(G["pages"], built):
        confs = np.asarray(rec["confs"], np.float64).astype(np.float32)

        class FakePage:
            def __init__(self, path):
                pass

            def get_regions(self, regions=regions, seps=seps):
                d = {"TextRegion": regions}
                if seps:
                    d["SeparatorRegion"] = seps
                return d
        monkeypatch.setattr(fg, "Page", FakePage)
        for key, want in rec["masked"].items():
            mh, ms = (int(t.split("=")[1]) for t in key.split(","))
            got = fg.mask_horizontally_separated_confs(confs.copy(), "unused", mask_heading=bool(mh), mask_horizontal=bool(ms), device_edges=True)
            host = fg.mask_horizontally_separated_confs(confs.copy(), "unused", mask_heading=bool(mh), mask_horizontal=bool(ms))
            assert got.dtype == host.dtype and np.array_equal(got, host), key
            if "raises" in want:      # the reference fails there; the product masks the headings (tests/test_host_goldens.py)
                exp = confs.astype(np.float64).copy()
                for pr in rec["pairs"]:
                    if pr["aligned_heading_separated"]:
                        exp[pr["i"], pr["j"]] = exp[pr["j"], pr["i"]] = 0.0
                assert np.array_equal(np.asarray(got, np.float64), exp)
                continue
            assert str(got.dtype) == want["dtype"], key
            assert np.array_equal(np.asarray(got, np.float64), np.asarray(want["values"], np.float64)), key


def _rect(box):
    min_x, max_x, min_y, max_y = box
    return [(min_x, min_y), (max_x, min_y), (max_x, max_y), (min_x, max_y)]


def test_touching_and_equal_coordinates_as_400_pages():
    """the 400 raw triples of the reference fixture, each a page of two regions and one untagged separator, in one call: touching and equal
    coordinates for the flags, collinear and all-equal point sets for the hulls"""
    from citlab_article_separation_new_amd import edge_features as ef, feature_generation as fg
    assert len(G["bbox_rules"]) == 400
    pages = [ef.EdgePage([_Region(_rect(c["a"])), _Region(_rect(c["b"]))], [_Sep(_rect(c["s"]))], [(0, 1)]) for c in G["bbox_rules"]]
    results = ef.edge_features_device(pages, rule="bb", hulls=True)
    for c, page, res in zip(G["bbox_rules"], pages, results):
        min_x, max_x, min_y, max_y = c["s"]
        vertical = not (max(max_y - min_y, 1) < 5 * max(max_x - min_x, 1))          # _sep_orientation without a tag
        want = [0.0, float(c["vertical"])] if vertical else [float(c["horizontal"]), 0.0]
        assert res["flags"][0].astype(np.float64).tolist() == want, c
        assert want == fg.get_edge_separator_feature_bb(page.text_regions[0], page.text_regions[1], page.separator_regions), c
        hull = _device_hulls(res)[0]
        assert hull == [list(p) for p in fg.get_edge_visual_region(*page.text_regions)], c
    # the fixture's boxes need not be degenerate: lines and points of their own for the hull's collinear and all-equal cases
    line = [(3, 3), (1, 1), (2, 2), (1, 1)]
    extra = [ef.EdgePage([_Region(line), _Region([(5, 5), (4, 4)])], [], [(0, 1), (1, 0)]),
             ef.EdgePage([_Region([(7, -2)] * 3), _Region([(7, -2)])], [], [(0, 1)]),
             ef.EdgePage([_Region([(0, 0), (0, 5), (0, 2)]), _Region([(0, 9)])], [], [(0, 1)])]
    got = [_device_hulls(r) for r in ef.edge_features_device(extra, hulls=True)]
    assert got == [[[[1, 1], [5, 5]]] * 2, [[[7, -2], [7, -2]]], [[[0, 0], [0, 9]]]]
    assert got == [_host_hulls(fg, p.text_regions, p.edges.tolist()) for p in extra]


# ---- rule `line`: pinned by the repository's restatement only (no reference run: the image lacks shapely) -----------------------------------
def _line_pages(ef):
    from citlab_article_separation_new_amd import synth
    # box sums even (integer centres: (5, 5), (25, 5)) and odd (half-integer centres: (5.5, 5.5), (25.5, 5.5), (15.5, 30.5))
    regions = [_Region(_rect((0, 10, 0, 10))), _Region(_rect((20, 30, 0, 10))), _Region(_rect((0, 11, 0, 11))),
               _Region(_rect((20, 31, 0, 11))), _Region([(10, 25), (21, 28), (15, 36), (12, 31)]), _Region(_rect((40, 50, 40, 51)))]
    shapes = [
        [(5, 5), (8, 20), (2, 20)],                                  # a vertex on the end of the segment (5, 5) - (25, 5)
        [(25, 5), (25, 30), (24, 30)],                               # ... and on its other end
        [(12, 5), (18, 5), (18, 9), (12, 9)],                        # an edge collinear with the segment y = 5 (and not with y = 5.5)
        [(12, 6), (18, 5), (18, 9)],                                 # a slanted triangle across y = 5.5
        # concave: a U around the lower regions whose box holds the segments between them, its boundary apart from them
        [(-50, -50), (100, -50), (100, 100), (-50, 100), (-50, 90), (90, 90), (90, -40), (-50, -40)],
        # concave zigzag of 12 points between the columns
        [(14, -5), (17, 0), (14, 5), (17, 10), (14, 15), (17, 20), (19, 20), (16, 15), (19, 10), (16, 5), (19, 0), (16, -5)],
        [(15, -3), (15, 40)],                                        # two points: a segment, closed there and back
        [(15, 5), (15, 5), (15, 5)],                                 # a point on the segment y = 5: its box is one point
        [(0, 20), (60, 20), (60, 22), (0, 22), (0, 20)],             # closed already, flat, below the upper row
        [(33, 0), (34, 0), (34, 60), (33, 60)],                      # tall and thin: ratio >= 5
    ]
    pages = [ef.EdgePage(regions, [_Sep(s, tag)], _fully(len(regions))) for s in shapes for tag in (None, "horizontal", "vertical", "diagonal")]
    for k in range(4):                                               # slanted and concave polygons of 3 to 12 points, tagged and untagged
        r, s = synth.synth_regions_and_separators(k, 8, 20, W=900, H=700)
        pages.append(ef.EdgePage(r, s, _fully(8)))
    sizes = {len(x.points) for p in pages[-4:] for x in p.separator_regions}
    assert min(sizes) == 3 and max(sizes) == 12 and {x.get_orientation() for x in pages[-1].separator_regions} == {None, "horizontal", "vertical"}
    return pages


def test_rule_line_against_the_restatement():
    from citlab_article_separation_new_amd import edge_features as ef, feature_generation as fg
    pages = _line_pages(ef)
    results = _check_pages(fg, ef, pages, "line", hulls=False, pair_bits=False)
    flags = np.concatenate([r["flags"] for r in results])
    assert flags[:, 0].any() and flags[:, 1].any() and not flags.all()
    # the same pages under `bb` (the tags none / horizontal / vertical / other take their branches there as well)
    _check_pages(fg, ef, pages, "bb", hulls=False, pair_bits=False)


# ---- sizes around the kernels' seams ---------------------------------------------------------------------------------------------------
def _ring(rng, n, cx, cy, radius):
    """n points, most of them on a circle (a hull of many points), some inside, some repeated"""
    ang = rng.random(n) * 2 * np.pi
    rad = np.where(rng.random(n) < 0.7, radius, rng.random(n) * radius)
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).astype(np.int32)
    pts[n // 2] = pts[0]
    return [tuple(int(v) for v in p) for p in pts]


def _seam_pages(ef):
    from citlab_article_separation_new_amd import synth
    rng = np.random.default_rng(99)
    pages = []
    for s_count in (0, 1, 63, 64, 65, 257):                         # around the 64 separators of one LDS chunk
        regions, seps = synth.synth_regions_and_separators(100 + s_count, 6, s_count, W=800, H=400)
        pages.append(ef.EdgePage(regions, seps, _fully(6)))
    regions, seps = synth.synth_regions_and_separators(7, 6, 5, W=800, H=400)
    regions[0] = _Region([(5, 5), (90, 17), (33, 80)], "heading")                        # 3 points
    regions[2] = _Region(_ring(rng, 65, 400, 200, 120), "paragraph")                   # 65 points: more than a wavefront
    regions[4] = _Region(_ring(rng, 300, 300, 250, 200), "heading")                    # 300 points
    pages.append(ef.EdgePage(regions, seps, _fully(6)))
    pages.insert(3, ef.EdgePage(*synth.synth_regions_and_separators(8, 6, 3, W=800, H=400), []))      # E = 0 between pages with edges
    regions, seps = synth.synth_regions_and_separators(9, 40, 20, W=1500, H=1200)
    pages.append(ef.EdgePage(regions, seps, _fully(40)))                                 # 1560 edges: seven blocks of the flag kernel
    return pages


@pytest.fixture(scope="module")
def seam_results():
    from citlab_article_separation_new_amd import edge_features as ef
    pages = _seam_pages(ef)
    return pages, {rule: ef.edge_features_device(pages, rule=rule, hulls=True, pair_bits=True) for rule in ("bb", "line")}


@pytest.mark.parametrize("rule", ["bb", "line"])
def test_seams_against_the_host(seam_results, rule):
    from citlab_article_separation_new_amd import edge_features as ef, feature_generation as fg
    pages, results = seam_results
    assert [len(p.separator_regions) for p in pages[:3] + pages[4:7]] == [0, 1, 63, 64, 65, 257] and len(pages[3].edges) == 0
    _check_pages(fg, ef, pages, rule, results[rule], hulls=rule == "bb", pair_bits=rule == "bb")
    assert max(int(r["hull_n"].max()) for r in results[rule] if len(r["hull_n"])) > 20      # the large regions give large hulls


def test_batch_equals_page_by_page_calls(seam_results):
    from citlab_article_separation_new_amd import edge_features as ef
    pages, results = seam_results
    for rule in ("bb", "line"):
        for page, batch in zip(pages, results[rule]):
            single = ef.edge_features_device([page], rule=rule, hulls=True, pair_bits=True)[0]
            assert sorted(single) == sorted(batch)
            for key in batch:
                assert single[key].dtype == batch[key].dtype and np.array_equal(single[key], batch[key]), (rule, key)


def test_hull_budget_splits_calls_and_refuses_a_single_edge(seam_results, monkeypatch):
    from citlab_article_separation_new_amd import _lib, edge_features as ef
    pages, results = seam_results
    monkeypatch.setattr(ef, "HULL_BYTE_BUDGET", 100 * 1024)           # the 1560 + 210 edges need about 1.3 MB in one call
    split = ef.edge_features_device(pages, rule="bb", hulls=True, pair_bits=True)
    assert sum(1 for name, _ in ef.last_launches if name == "edge_hull_kernel") > 3
    for a, b in zip(split, results["bb"]):
        for key in b:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    monkeypatch.setattr(ef, "HULL_BYTE_BUDGET", 2000)                 # the first edge into the 300 point region needs 303 x 8 bytes
    with pytest.raises(_lib.AsepError, match=r"joins regions of 303 points: its hull row of 2424 bytes alone exceeds the budget of 2000 bytes, "
                                             r"no split of the edges helps"):
        ef.edge_features_device([pages[7]], rule="bb", hulls=True)
    assert ef.launches() == []


def test_refusals_through_the_abi():
    """each returns ASEP_ERR_ARG with its reason and launches nothing"""
    from citlab_article_separation_new_amd import _lib, edge_features as ef, feature_generation as fg
    good = ef.EdgePage([_Region(_rect((0, 10, 0, 10))), _Region(_rect((20, 30, 0, 10)))], [_Sep(_rect((14, 16, -5, 40)))], [(0, 1)])

    def refused(match, rule=0, **change):
        t = ef.pack_pages([good])
        t.update(change)
        with pytest.raises(_lib.AsepError, match=match) as e:
            ef.run_tables(t, rule, hulls=True, pair_bits=True, hull_cap=8)
        assert "(-1)" in str(e.value)                                 # ASEP_ERR_ARG
        assert ef.launches() == [] and _lib.load_library().asep_edge_features_last_kernel_us() == 0.0

    ef.run_tables(ef.pack_pages([good]), 0, hulls=True, pair_bits=True)
    assert ef.launches()
    refused(r"edge 0 of page 0 names region 2, the page has 2 regions", edges=np.array([[0, 2]], np.int32))
    refused(r"edge 0 of page 0 names region -1, the page has 2 regions", edges=np.array([[-1, 1]], np.int32))
    pts = ef.pack_pages([good])["node_pts"]
    pts[5, 1] = (1 << 20) + 1
    refused(r"point 1 of region 1 of page 0 has the coordinate 1048577, outside \[-1048576, 1048576\]", node_pts=pts)
    refused(r"region 0 of page 0 has no points \(node_pt_off 0 -> 0\)", node_pt_off=np.array([0, 0, 8], np.int32))
    refused(r"separator 0 of page 0 has no points", sep_pt_off=np.array([0, 0], np.int32))
    refused(r"unknown rule 2", rule=2)
    refused(r"node_off 0 \(0 -> -2\) is decreasing", node_off=np.array([0, -2], np.int32))
    # the bound itself is accepted
    pts = ef.pack_pages([good])["node_pts"]
    pts[5, 1] = 1 << 20
    pts[0, 0] = -(1 << 20)
    t = ef.pack_pages([good])
    t["node_pts"] = pts
    flags, hull, hull_n, pairs = ef.run_tables(t, 1, hulls=True, pair_bits=True)
    moved = [_Region(pts[:4].tolist()), _Region(pts[4:].tolist())]
    assert hull[0, :hull_n[0]].tolist() == _host_hulls(fg, moved, [(0, 1)])[0]
    assert flags.astype(np.float64).tolist() == [fg.get_edge_separator_feature_line(moved[0], moved[1], good.separator_regions)]
    # nothing to do is valid: no pages, no edges, no separators
    assert ef.edge_features_device([], hulls=True, pair_bits=True) == []
    res = ef.edge_features_device([ef.EdgePage(good.text_regions, [], [])], hulls=True, pair_bits=True)[0]
    assert res["flags"].shape == (0, 2) and res["hull_n"].shape == (0,) and not res["pair_bits"].any()


def test_launch_record_names_the_engines_kernels():
    """the device path did the work: the engine's own record of its last call lists its kernels, with their grids"""
    from citlab_article_separation_new_amd import edge_features as ef, synth
    regions, seps = synth.synth_regions_and_separators(3, 30, 70, W=1500, H=1200)
    ef.edge_features_device([ef.EdgePage(regions, seps, _fully(30))] * 2, rule="line", hulls=True, pair_bits=True)
    assert ef.last_launches == ef.launches()
    assert ef.last_launches == [("edge_boxes_kernel", 1), ("edge_boxes_kernel", 1), ("edge_flags_kernel<line>", 8), ("edge_pair_bits_kernel", 8),
                                ("edge_sort_points_kernel", 60), ("edge_hull_kernel", 7)]
    assert ef.last_kernel_us > 0
    ef.edge_features_device([ef.EdgePage(regions, seps, _fully(30))], rule="bb")
    assert ef.last_launches == [("edge_boxes_kernel", 1), ("edge_boxes_kernel", 1), ("edge_flags_kernel<bb>", 4)]


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_feature_jsons_are_byte_identical(tmp_path):
    """18 small pages (two engine calls of 16 and 2), visual regions, both separator rules, both edge sets"""
    from PIL import Image
    from citlab_article_separation_new_amd import feature_generation as fg, synth
    data = tmp_path / "data"
    (data / "page").mkdir(parents=True)
    paths = []
    for k in range(18):
        Image.fromarray(synth.synth_page(k, W=600, H=900)).save(data / f"p{k:02d}.png")
        synth.synth_region_page_xml(str(data / "page" / f"p{k:02d}.xml"), k, n_regions=3 if k == 5 else 12, n_separators=0 if k == 7 else 6,
                                    W=600, H=900, image_filename=f"p{k:02d}.png")
        paths.append(str(data / "page" / f"p{k:02d}.xml"))
    assert fg.EDGE_PAGE_GROUP == 16 < len(paths)
    for separators, interaction in itertools.product(("bb", "line"), ("fully", "delaunay")):
        host = fg.generate_feature_jsons(paths, str(tmp_path / f"host_{separators}_{interaction}"), interaction, True, separators=separators)
        dev = fg.generate_feature_jsons(paths, str(tmp_path / f"dev_{separators}_{interaction}"), interaction, True, separators=separators,
                                        device_edges=True)
        assert len(host) == len(dev) == 18
        for a, b in zip(host, dev):
            assert os.path.basename(a) == os.path.basename(b) and open(a, "rb").read() == open(b, "rb").read(), (separators, interaction, a)
        made = [json.load(open(path)) for path in dev]
        assert any(np.asarray(m["edge_features"])[:, 0].any() for m in made) and any(np.asarray(m["edge_features"])[:, 1].any() for m in made)
        assert max(max(m["num_points_visual_regions_edges"]) for m in made) > 4


def _write_chain_page(path, W, H, blocks):
    regs = []
    for i, (x0, y0, x1, y1, nl) in enumerate(blocks):
        lines = []
        lh = (y1 - y0) // nl
        for k in range(nl):
            ya, yb = y0 + k * lh, y0 + (k + 1) * lh - 4
            lines.append(f'<TextLine id="r{i}l{k}"><Coords points="{x0},{ya} {x1},{ya} {x1},{yb} {x0},{yb}"/>'
                         f'<Baseline points="{x0},{yb - 3} {x1},{yb - 3}"/><TextEquiv><Unicode>t{k}</Unicode>'
                         f'</TextEquiv></TextLine>')
        regs.append(f'<TextRegion id="r{i}"><Coords points="{x0},{y0} {x1},{y0} {x1},{y1} {x0},{y1}"/>'
                    + "".join(lines) + '</TextRegion>')
    path.write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/'
                    'pagecontent/2013-07-15"><Metadata><Creator>t</Creator><Created>2020-01-01T00:00:00</Created>'
                    '<LastChange>2020-01-01T00:00:00</LastChange></Metadata>'
                    f'<Page imageFilename="p0.png" imageWidth="{W}" imageHeight="{H}">' + "".join(regs)
                    + '</Page></PcGts>')


def test_gnn_clustering_gives_the_same_article_ids(tmp_path):
    """the page set of tests/test_full_chain_gpu.py, built afresh (scan + PAGE-XML -> separators -> headings -> graph json -> relation net):
    run_gnn_clustering with both masks writes the same article ids with and without --device_edges True"""
    from PIL import Image
    from citlab_article_separation_new_amd import (feature_generation as fg, pb_import, run_feature_generation, run_gnn_clustering,
                                                   run_net_post_processing, synth)
    from citlab_article_separation_new_amd.config import AruConfig, GnnConfig
    from citlab_article_separation_new_amd.page_xml import Page
    from citlab_article_separation_new_amd.weights import init_aru_weights, init_gnn_weights
    from oracle import classical_oracle as co, gnn_cases
    sys.path.insert(0, os.path.dirname(__file__))
    import tf_aru_graph
    mask = [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1]
    W, H = 600, 900
    data = tmp_path / "data"
    (data / "page").mkdir(parents=True)
    gray = synth.synth_page(9, W=W, H=H)
    Image.fromarray(gray).save(data / "p0.png")
    _write_chain_page(data / "page" / "p0.xml", W, H, [(40 + 190 * c, 60 + 140 * r, 200 + 190 * c, 180 + 140 * r, 3) for r in range(5) for c in range(3)])
    lst = tmp_path / "images.lst"
    lst.write_text(str(data / "p0.png") + "\n")
    acfg = AruConfig()
    for name, seed in (("sep.pb", 21), ("head.pb", 22)):
        (tmp_path / name).write_bytes(tf_aru_graph.build_aru_pb(init_aru_weights(acfg, seed, bias_jitter=0.05, logit_scale=0.05), acfg))
    for name, extra in (("sep.pb", ["--mode", "separator", "--fixed_height", "450", "--threshold", "0.5"]),
                        ("head.pb", ["--mode", "heading", "--fixed_height", "300"])):
        assert run_net_post_processing.main(["--path_to_image_list", str(lst), "--path_to_pb", str(tmp_path / name), *extra, "--num_processes", "1"]) == 0
        shutil.move(str(data / "page" / "p0.xml.xml"), str(data / "page" / "p0.xml"))
    page_path = str(data / "page" / "p0.xml")
    regions = Page(page_path).get_regions()
    plist = tmp_path / "pages.lst"
    plist.write_text(page_path + "\n")
    # the graph json both ways as well, through the command line
    assert run_feature_generation.main(["--pagexml_list", str(plist), "--separators", "bb", "--out_dir", str(tmp_path / "json_host")]) == 0
    assert run_feature_generation.main(["--pagexml_list", str(plist), "--separators", "bb", "--out_dir", str(tmp_path / "json_dev"),
                                        "--device_edges", "True"]) == 0
    assert (tmp_path / "json_host" / "p0.json").read_bytes() == (tmp_path / "json_dev" / "p0.json").read_bytes()
    assert run_feature_generation.main(["--pagexml_list", str(plist), "--separators", "bb"]) == 0
    jpath = data / "json15d2bb" / "p0.json"
    ref = fg.build_input_and_target(page_path, separators="bb", swt_img=co.swt_distance_transform(gray))
    gcfg = GnnConfig()
    keep = [i for i, m in enumerate(mask) if m]
    column = np.array([i % 3 for i in range(15)])
    gw = gnn_cases.calibrate_l1_classifier(init_gnn_weights(gcfg, 23, bias_jitter=0.05), gcfg, 15, ref[1], ref[3][:, keep], ref[4],
                                           column[:, None] == column[None, :], wrong_side=0.2, seed=5)
    (tmp_path / "gnn.pb").write_bytes(pb_import.weights_to_graphdef(gw, "graph/", meta={"num_transition_steps": 3}))
    jl = tmp_path / "eval.lst"
    jl.write_text(str(jpath) + "\n")
    ids = {}
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        for name, extra in (("host", []), ("dev", ["--device_edges", "True"])):
            outs = run_gnn_clustering.main([
                "--model_dir", str(tmp_path / "gnn.pb"), "--eval_list", str(jl), "--out_dir", "out_" + name, "--input_params", "node_feature_dim=15",
                "edge_feature_dim=2", "node_input_feature_mask=" + str(mask).replace(" ", ""), "--clustering_method", "dbscan",
                "--mask_horizontally_separated_confs", "True", "--mask_heading_separated_confs", "True", *extra])
            assert len(outs) == 1
            out = outs[0] if os.path.isabs(outs[0]) else os.path.join(tmp_path, outs[0])
            ids[name] = [r.text_lines[0].get_article_id() for r in Page(out).get_regions()["TextRegion"]]
    finally:
        os.chdir(cwd)
    assert ids["host"] == ids["dev"] and len(ids["dev"]) == 15
    # and the masks of this page themselves, whatever the separator net found on it
    confs = np.random.default_rng(4).random((15, 15)).astype(np.float32)
    for mh, ms in ((True, True), (True, False), (False, True)):
        if ms and "SeparatorRegion" not in regions:
            continue
        assert np.array_equal(fg.mask_horizontally_separated_confs(confs.copy(), page_path, mh, ms, device_edges=True),
                              fg.mask_horizontally_separated_confs(confs.copy(), page_path, mh, ms))
