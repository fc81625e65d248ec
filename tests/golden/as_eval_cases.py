"""Page pairs for the split / merge comparison (as_eval.py), shared by the golden generator and the tests: each side of a pair
is a table of (line id, article id or None) in document order.  ``write_page`` turns such a table into a PAGE-XML file with
``page_xml.Page``."""
import xml.etree.ElementTree as ET

import numpy as np


def _t(spec):
    """'a1:l1 l2|a2:l3|-:l4' -> [(l1, a1), (l2, a1), (l3, a2), (l4, None)]"""
    out = []
    for part in spec.split("|"):
        art, lines = part.split(":")
        out.extend((l, None if art == "-" else art) for l in lines.split())
    return out


HAND = [
    ("identical", "a1:l1 l2|a2:l3 l4", "x:l1 l2|y:l3 l4"),
    ("identical_one_article", "a1:l1 l2 l3", "b:l1 l2 l3"),
    ("pure_split", "a1:l1 l2 l3 l4", "x:l1 l2|y:l3 l4"),
    ("pure_split_three", "a1:l1 l2 l3|a2:l4", "x:l1|y:l2|z:l3|w:l4"),
    ("pure_merge", "a1:l1 l2|a2:l3 l4", "x:l1 l2 l3 l4"),
    ("pure_merge_three", "a1:l1|a2:l2|a3:l3 l4", "x:l1 l2 l3 l4"),
    ("split_and_merge", "a1:l1 l2|a2:l3 l4", "x:l1|y:l2 l3 l4"),
    ("split_and_merge_crossed", "a1:l1 l2 l3|a2:l4 l5 l6", "x:l1 l4|y:l2 l5|z:l3 l6"),
    ("interleaved_document_order", "a1:l1|a2:l2|a1:l3|a2:l4", "x:l1 l3|y:l2 l4"),
    ("hyp_lacks_lines", "a1:l1 l2 l3|a2:l4 l5", "x:l1 l2|y:l4 l5"),
    ("hyp_lacks_lines_split", "a1:l1 l2 l3|a2:l4 l5", "x:l1|y:l2|z:l4 l5"),
    ("hyp_lacks_whole_article", "a1:l1 l2|a2:l3", "x:l1 l2"),
    ("gt_lacks_lines_strict_subset", "a1:l1 l2|a2:l3", "x:l1 l2|y:l3 l4"),
    ("gt_lacks_lines_strict_subset_same_article", "a1:l1 l2", "x:l1 l2 l3"),
    ("both_lack_lines", "a1:l1 l2 l3|a2:l4", "x:l1 l2 l9|y:l4"),
    ("both_lack_lines_merge", "a1:l1 l2 l3|a2:l4", "x:l1 l2 l4 l9"),
    ("both_lack_lines_extra_own_article", "a1:l1 l2 l3|a2:l4", "x:l1 l2|y:l4|z:l9"),
    ("article_emptied_by_removal", "a1:l1 l2|a2:l3|a3:l4", "x:l1 l2|y:l4"),
    ("article_emptied_and_split", "a1:l1 l2|a2:l3", "x:l1|y:l2"),
    ("gt_lines_without_article", "a1:l1 l2|-:l3 l4", "x:l1 l2|y:l3 l4"),
    ("gt_lines_without_article_split", "a1:l1 l2|-:l3 l4", "x:l1 l2|y:l3|z:l4"),
    ("hyp_lines_without_article", "a1:l1 l2|a2:l3 l4", "x:l1 l2|-:l3 l4"),
    ("both_without_article", "-:l1 l2", "-:l1 l2"),
    ("one_line_page", "a1:l1", "x:l1"),
    ("one_line_page_no_article", "-:l1", "x:l1"),
    ("one_line_hyp_lacks_it_other_line", "a1:l1", "x:l2"),
    ("disjoint_lines", "a1:l1 l2", "x:l3 l4"),
    ("gt_articles_outnumber_hyp_lines", "a1:l1|a2:l2|a3:l3", "x:l3"),
]


def _seeded(seed, n_lines, n_gt, n_hyp, drop_hyp, drop_gt):
    rng = np.random.default_rng(seed)
    ids = [f"tl_{i}" for i in range(n_lines)]
    gt = [(l, f"a{int(rng.integers(n_gt))}") for l in ids]
    hyp = [(l, f"h{int(rng.integers(n_hyp))}") for l in ids]
    hyp = [e for e in hyp if rng.random() >= drop_hyp] or hyp[:1]
    gt = [e for e in gt if rng.random() >= drop_gt] or gt[:1]
    return gt, hyp


def cases():
    """-> [(name, ground truth table, hypothesis table)]"""
    out = [(name, _t(gt), _t(hyp)) for name, gt, hyp in HAND]
    for k, args in enumerate([(12, 3, 3, 0.0, 0.0), (20, 4, 6, 0.0, 0.0), (20, 6, 3, 0.15, 0.0), (30, 5, 5, 0.1, 0.1),
                              (40, 8, 8, 0.05, 0.0), (15, 2, 7, 0.2, 0.2)]):
        out.append((f"seeded_{k}", *_seeded(500 + k, *args)))
    return out


# countWinnerStat / calcWinnerDict: 3 pages x 4 methods as (dist, corrects), ties included.  The hypothesis path of method m on
# page p is WINNER_HYP.format(m=m, p=p): path2method reads parts[-5] and parts[-1] of its folder.
WINNER_METHODS = ["dbscan_conf0.5_cluster0.5", "dbscan_conf0.6_cluster0.4", "greedy_iter1000", "linkage_centroid_distance_t-1.0"]
WINNER_HYP = "/data/run1/set/sub/clustering/{m}/page{p}_clustering.xml"
WINNER_GT = "/data/gt/page/page{p}.xml"
WINNER_TABLE = [                      # [page][method] = (dist, corrects)
    [(0, 5), (0, 5), (2, 3), (-1, 4)],
    [(1, 2), (1, 3), (1, 3), (3, 0)],
    [(-2, 1), (0, 4), (-2, 2), (-2, 1)],
]


def write_page(path, regions, page_cls):
    """PAGE-XML with one TextRegion per entry of ``regions`` ([(line id, article id or None)] each), written with ``page_cls``
    (page_xml.Page)"""
    from citlab_article_separation_new_amd.page_xml import TextLine
    page = page_cls(None, img_filename="scan.png", img_w=1000, img_h=1000)
    q = page._q
    for r, lines in enumerate(regions):
        reg = ET.SubElement(page.page_node, q("TextRegion"), {"id": f"r{r}"})
        ET.SubElement(reg, q("Coords"), {"points": "0,0 10,0 10,10 0,10"})
        for line_id, article in lines:
            nd = ET.SubElement(reg, q("TextLine"), {"id": line_id})
            ET.SubElement(nd, q("Coords"), {"points": "0,0 10,0 10,10 0,10"})
            ET.SubElement(nd, q("Baseline"), {"points": "0,5 10,5"})
            tl = TextLine(nd, page)
            tl.set_article_id(article)
            tl.flush()
    page.write_page_xml(str(path))
    return str(path)
