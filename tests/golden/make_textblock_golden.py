"""Generates textblock_golden.json from the REFERENCE's text block detection code (use_java_code=False):
dbscan_baselines.py (interline distances, DBSCANBaselines, region_query, labels) and textregion_generation.py
(create_text_regions, txtlines_set_reading_order) on the seeded pages of textblock_cases.py.

Run in the build container only (the reference imports TensorFlow, lxml, jpype ... at module level: ref_import stubs
them).  scipy here has no Delaunay.vertices: it is aliased to .simplices for this generator only.

    python tests/golden/make_textblock_golden.py
"""
import contextlib
import io
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

ref_import.install_stubs()

import scipy.spatial  # noqa: E402

if not hasattr(scipy.spatial.Delaunay, "vertices"):
    scipy.spatial.Delaunay.vertices = property(lambda self: self.simplices)

from python_util.geometry.polygon import Polygon, norm_poly_dists, calc_reg_line_stats  # noqa: E402
from article_separation.baseline_clustering import dbscan_baselines as db  # noqa: E402
from article_separation.textregion_generation import textregion_generation as trg  # noqa: E402

import textblock_cases  # noqa: E402


class _Baseline:
    def __init__(self, xs, ys):
        self.xs, self.ys = xs, ys

    def to_polygon(self):
        return Polygon(list(self.xs), list(self.ys), len(self.xs))


class _Line:
    """duck-typed TextLine: id, baseline.to_polygon(), custom"""

    def __init__(self, lid, xs, ys):
        self.id = lid
        self.baseline = _Baseline(xs, ys)
        self.custom = {}


def _polys(page):
    return [Polygon(list(xs), list(ys), len(xs)) for xs, ys in page]


def _normed(ps):
    return [[list(p.x_points), list(p.y_points)] for p in ps]


def _angles(ps):
    out = []
    for p in ps:
        a = calc_reg_line_stats(p)[0]
        out.append([a, math.cos(a), math.sin(a)])
    return out


def _f(v):
    return [float(x) for x in v]


def run_page(name, page):
    rec = {"name": name, "polygons": [[list(xs), list(ys)] for xs, ys in page]}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        n1 = norm_poly_dists(_polys(page), 5)
        rec["normed1"], rec["angles1"] = _normed(n1), _angles(n1)
        d1 = db.get_list_of_interline_distances(_polys(page), des_dist=5, max_d=500, use_java_code=False)
        rec["dists1"] = _f(d1)
        al = [d for d in d1 if d > 0]
        rec["avg1"] = 1 / len(al) * sum(al) if al else None
        obj = db.DBSCANBaselines(_polys(page), min_polygons_for_cluster=2, min_polygons_for_article=1,
                                 rectangle_interline_factor=1.25, des_dist=5, max_d=500, use_java_code=False,
                                 target_average_interline_distance=50)
        rec["normed2"], rec["angles2"] = _normed(obj.list_of_normed_polygons), _angles(obj.list_of_normed_polygons)
        rec["dists2"] = _f(obj.list_of_interline_distances)
        rec["avg"] = float(obj.avg)
        n = len(page)
        rec["neighbours"] = [obj.region_query(i) for i in range(n)]
        labels = {}
        for min_art in (1, 3):
            obj.list_of_labels = [0] * n
            obj.list_if_center = [False] * n
            obj.min_polygons_for_article = min_art
            obj.clustering_polygons()
            try:
                labels[str(min_art)] = list(obj.get_cluster_of_polygons())
            except ValueError as e:
                labels[str(min_art)] = "ValueError"
        rec["labels"] = labels

        # text regions: article ids of the min_polygons_for_article = 3 labels (noise -> no id), des_dist 50, max_d 100
        lab3 = labels["3"]
        lines = [_Line("l%d" % i, xs, ys) for i, (xs, ys) in enumerate(page)]
        art = {}
        for ln, lab in zip(lines, lab3 if isinstance(lab3, list) else []):
            art.setdefault(None if lab == -1 else "a%d" % lab, []).append(ln)
        n50 = norm_poly_dists(_polys(page), 50)
        d_tr = db.get_list_of_interline_distances(_polys(page), max_d=100, use_java_code=False)
        rec["normed50"] = _normed(n50)
        rec["dists_tr"] = _f(d_tr)
        txt = {ln.id: (n50[i], d_tr[i]) for i, ln in enumerate(lines)}
    buf_tr = io.StringIO()
    with contextlib.redirect_stdout(buf_tr):
        regions = trg.create_text_regions(art, txt, alpha=75)
    rec["alpha_retries"] = buf_tr.getvalue().count("alpha value not suitable -> is increased")
    out = []
    for rid, (bp, tls, ro) in regions.items():
        trg.txtlines_set_reading_order(tls)
        out.append({"id": rid, "points": bp, "lines": [t.id for t in tls], "reading_order": ro,
                    "line_reading_orders": [t.custom["readingOrder"]["index"] for t in tls]})
    rec["regions"] = out
    rec["articles"] = {("" if k is None else k): [ln.id for ln in v] for k, v in art.items()}
    return rec


def main():
    cases = []
    for name, page in textblock_cases.golden_pages():
        cases.append(run_page(name, page))
        print(name, len(page), "baselines")
    path = os.path.join(HERE, "textblock_golden.json")
    with open(path, "w") as f:
        json.dump({"generator": "make_textblock_golden.py", "cases": cases}, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
