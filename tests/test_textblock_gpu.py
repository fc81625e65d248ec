"""Text block detection on the GPU: the two kernels against the reference's Python path (tests/golden/textblock_golden.json)
bit for bit, one page per launch and all pages in one launch; labels and regions of the whole stage; a seeded fuzz
against the loop-for-loop restatement in textblock_cases.py; and the command lines end to end (baseline-only PAGE-XML ->
run_baseline_clustering -> run_textregion_generation -> run_feature_generation).  Every GPU step runs in a child
process (this file, run as a script) under a time limit."""
import json
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


def _child(check, *args, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), check, *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, f"{check} failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def test_interline_distances_golden():
    assert "ok" in _child("distances")


def test_neighbours_golden():
    assert "ok" in _child("neighbours")


def test_labels_and_regions_golden():
    assert "ok" in _child("labels_regions")


def test_fuzz_against_restatement():
    assert "ok" in _child("fuzz", timeout=1200)


def test_command_lines_report_bad_files(tmp_path):
    assert "ok" in _child("bad_files", str(tmp_path), timeout=600)


def test_command_line_chain(tmp_path):
    out = _child("chain", str(tmp_path), timeout=900)
    assert "ok" in out


# ---- the checks, run in the child -------------------------------------------------------------------------------------

def _gold():
    return json.load(open(os.path.join(HERE, "golden", "textblock_golden.json")))["cases"]


def _pages(polys_per_page, des_dist):
    from citlab_article_separation_new_amd import textblock
    return textblock.normed_pages(polys_per_page, des_dist)


def check_distances():
    from citlab_article_separation_new_amd import textblock, textblock_geometry as geo
    gold = _gold()
    polys = [[tuple(p) for p in c["polygons"]] for c in gold]
    first = _pages(polys, 5)
    for c, pg in zip(gold, first):                                       # one page per launch
        assert textblock.interline_distances([pg], 5, 500)[0].tolist() == c["dists1"], c["name"]
    batched = textblock.interline_distances(first, 5, 500)              # all pages in one launch
    assert [d.tolist() for d in batched] == [c["dists1"] for c in gold]
    resc = [c for c in gold if c["avg1"] is not None]
    second = _pages([geo.scale_polygons([tuple(p) for p in c["polygons"]], 50 / c["avg1"]) for c in resc], 5)
    assert [d.tolist() for d in textblock.interline_distances(second, 5, 500)] == [c["dists2"] for c in resc]
    tr = textblock.interline_distances(first, 5, 100)                    # text region generation: max_d 100
    assert [d.tolist() for d in tr] == [c["dists_tr"] for c in gold]
    print("ok", textblock.last_kernel_us(0))


def check_neighbours():
    from citlab_article_separation_new_amd import textblock
    gold = _gold()
    pages = [textblock.NormedPage([tuple(p) for p in c["normed2"]]) for c in gold]
    for c, pg in zip(gold, pages):
        assert textblock.neighbour_lists([pg], [c["dists2"]], [c["avg"]], 1.25)[0] == c["neighbours"], c["name"]
    got = textblock.neighbour_lists(pages, [c["dists2"] for c in gold], [c["avg"] for c in gold], 1.25)
    assert got == [c["neighbours"] for c in gold]
    print("ok")


def check_labels_regions():
    from citlab_article_separation_new_amd import textblock, textblock_geometry as geo
    gold = _gold()
    polys = [[tuple(p) for p in c["polygons"]] for c in gold]
    for min_art in (1, 3):
        res = textblock.cluster_baselines(polys, 2, min_art, 1.25, 5, 500, 50)
        for c, r in zip(gold, res):
            want = c["labels"][str(min_art)]
            if want == "ValueError":
                assert isinstance(r, ValueError), c["name"]
            else:
                assert r[0] == want, (c["name"], min_art)
    dists = textblock.interline_distances(_pages(polys, 5), 5, 100)
    for c, d in zip(gold, dists):
        art = {(None if k == "" else k): v for k, v in c["articles"].items()}
        n50 = geo.norm_poly_dists([tuple(p) for p in c["polygons"]], 50)
        geom = {"l%d" % i: (p, v) for i, (p, v) in enumerate(zip(n50, d.tolist()))}
        regions = textblock.create_text_regions(art, geom, 75, log=lambda s: None)
        assert [(r[0], r[1], r[2], r[3]) for r in regions] == \
            [(g["id"], g["points"], g["lines"], g["reading_order"]) for g in c["regions"]], c["name"]
    print("ok")


def check_fuzz():
    import math
    import textblock_cases as tc
    from citlab_article_separation_new_amd import textblock
    n_checked = 0
    for seed, n_lines, max_w in ((11, 300, 120), (12, 200, 300), (13, 120, 600)):
        polys = tc.random_page(seed, n_lines, 2000, 2600, max_w)
        pg = _pages([polys], 5)[0]
        normed = [([int(v) for v in xs], [int(v) for v in ys]) for xs, ys in pg.polys]
        orient = [(math.cos(a), math.sin(a)) for a in pg.angles]
        d = textblock.interline_distances([pg], 5, 500)[0].tolist()
        assert d == tc.slow_interline_distances(normed, orient, 5, 500), seed
        avg = textblock.average_positive(d, 1e-8)
        boxes = [tuple(int(v) for v in b) for b in pg.boxes]
        assert textblock.neighbour_lists([pg], [d], [avg], 1.25)[0] == tc.slow_neighbours(boxes, d, avg, 1.25), seed
        n_checked += n_lines
    print("ok", n_checked)


NS = "http://schema.primaresearch.org/PAGE/gts/pagecontent/2013-07-15"


def _baseline_page(path, img_name, W, H, page):
    lines = "".join('<TextLine id="tl_%d"><Baseline points="%s"/><TextEquiv><Unicode>w%d</Unicode></TextEquiv></TextLine>'
                    % (i, " ".join("%d,%d" % (x, y) for x, y in zip(xs, ys)), i) for i, (xs, ys) in enumerate(page))
    with open(path, "w") as f:
        f.write('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="%s"><Metadata><Creator>htr</Creator>'
                '<Created>2020-01-01T00:00:00</Created><LastChange>2020-01-01T00:00:00</LastChange></Metadata>'
                '<Page imageFilename="%s" imageWidth="%d" imageHeight="%d"><TextRegion id="r0" type="paragraph">'
                '<Coords points="0,0 %d,0 %d,%d 0,%d"/>%s</TextRegion></Page></PcGts>'
                % (NS, img_name, W, H, W - 1, W - 1, H - 1, H - 1, lines))


def check_chain(tmp):
    import numpy as np
    from PIL import Image
    import textblock_cases as tc
    from citlab_article_separation_new_amd import synth
    from citlab_article_separation_new_amd.page_xml import Page
    W, H = 1400, 1300
    data = os.path.join(tmp, "data")
    os.makedirs(os.path.join(data, "page"), exist_ok=True)
    paths = []
    for k, seed in enumerate((31, 32)):
        page = tc.columns_page(seed, n_cols=3, n_lines=10, col_w=300, pitch=40)
        Image.fromarray(synth.synth_page(k, W=W, H=H)).save(os.path.join(data, "p%d.png" % k))
        p = os.path.join(data, "page", "p%d.xml" % k)
        _baseline_page(p, "p%d.png" % k, W, H, page)
        paths.append(p)
    lst = os.path.join(tmp, "pages.lst")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(mod, *args):
        r = subprocess.run([sys.executable, "-m", "citlab_article_separation_new_amd." + mod, *args], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{mod}: {r.stdout[-3000:]}\n{r.stderr[-3000:]}"
        return r.stdout
    out = run("run_baseline_clustering", "--path_to_xml_lst", lst, "--num_threads", "2")
    assert out.count("Number of detected articles (inclusive the \"noise\" class): ") == 2
    arts = []
    for p in paths:
        tls = Page(p).get_textlines()
        assert all(tl.get_article_id() for tl in tls)           # min_polygons_for_article 1: every line has an article
        arts.append({tl.id: tl.get_article_id() for tl in tls})
    run("run_textregion_generation", "--path_to_xml_lst", lst)
    regions = []
    for p, art in zip(paths, arts):
        regs = Page(p).get_text_regions()
        assert [r.id for r in regs] == ["tr_%d" % i for i in range(len(regs))] and len(regs) >= 2
        seen = []
        for r in regs:
            ids = {art[tl.id] for tl in r.text_lines}
            # (a closed outline: a line of one normed point gives two outline points, returned as they are + the first)
            assert len(ids) == 1 and r.region_type == "paragraph" and len(r.points) >= 3 and r.points[0] == r.points[-1]
            assert all(tl.surr_p for tl in r.text_lines)          # synthetic Coords
            seen += [tl.id for tl in r.text_lines]
        assert sorted(seen) == sorted(art)
        regions.append(regs)
    out_dir = os.path.join(tmp, "json")
    run("run_feature_generation", "--pagexml_list", lst, "--out_dir", out_dir)
    for p, regs in zip(paths, regions):
        g = json.load(open(os.path.join(out_dir, os.path.splitext(os.path.basename(p))[0] + ".json")))
        assert g["num_nodes"] == len(regs)                       # one graph node per generated region
        assert np.asarray(g["node_features"]).shape[0] == len(regs)
    print("ok")


def check_bad_files(tmp):
    """a malformed file and a page whose baseline box exceeds 100000 px fail alone: both command lines list them under
    "saving errors", leave them as they were and process the good page of the same group"""
    import textblock_cases as tc
    from citlab_article_separation_new_amd import run_baseline_clustering as rbc, run_textregion_generation as rtg
    from citlab_article_separation_new_amd.page_xml import Page
    good, broken, huge = (os.path.join(tmp, n) for n in ("good.xml", "broken.xml", "huge.xml"))
    _baseline_page(good, "g.png", 1400, 1300, tc.columns_page(41, n_cols=2, n_lines=6, col_w=300))
    with open(broken, "w") as f:
        f.write("<PcGts><Page>")
    _baseline_page(huge, "h.png", 1400, 1300, [([10, 400], [50, 50]), ([10, 200010], [90, 95])])
    before = {p: open(p).read() for p in (broken, huge)}
    paths = [broken, good, huge]
    errs = rbc.process(paths, rbc.build_parser().parse_args([]), log=lambda s: None)
    assert [e.split(":")[0] for e in errs] == [broken, huge], errs
    assert all(tl.get_article_id() for tl in Page(good).get_textlines())
    errs = rtg.process(paths, rtg.build_parser().parse_args([]), log=lambda s: None)
    assert [e.split(":")[0] for e in errs] == [broken, huge], errs
    assert [r.id for r in Page(good).get_text_regions()][:1] == ["tr_0"]
    assert all(open(p).read() == before[p] for p in (broken, huge))
    print("ok")


if __name__ == "__main__":
    name = sys.argv[1]
    {"distances": check_distances, "neighbours": check_neighbours, "labels_regions": check_labels_regions,
     "fuzz": check_fuzz, "chain": lambda: check_chain(sys.argv[2]),
     "bad_files": lambda: check_bad_files(sys.argv[2])}[name]()
