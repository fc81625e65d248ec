"""Host side of the heading evaluation (no GPU), against tests/golden/heading_eval_golden.json (the imported reference:
its grid script's enumeration, its heading_evaluation.py __main__ with sklearn): the grid, the confidence helper with a
numpy restatement of the fusion rule, the metrics and their averages, the log text and file names, the flags."""
import hashlib
import json
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from citlab_article_separation_new_amd import heading_evaluation as he  # noqa: E402
import heading_eval_cases as hc  # noqa: E402

def canonical(rows):
    """make_heading_eval_golden.canonical: rows of (fixed_height, 9 floats) -> the text the SHA-256 is taken of"""
    return "\n".join(",".join([str(int(r[0]))] + [repr(float(x)) for x in r[1:]]) for r in rows)


GOLD = json.load(open(os.path.join(HERE, "golden", "heading_eval_golden.json")))


def _lines(page):
    return [types.SimpleNamespace(id=d["id"]) for d in page["lines"]]


def _values(page):
    return ({d["id"]: d["sw"] for d in page["lines"]}, {d["id"]: d["th"] for d in page["lines"]},
            {d["id"]: d["net"] for d in page["lines"]})


def fuse_regions(sw, th, net, use_swt, tagged, region_lines, tenths):
    """numpy restatement of heading_net_post_processor.py:154-195 for one setting -> region heading labels"""
    thr, nw, sww, thw, nt, swt, tht, swth, tlp = (k / 10 for k in tenths)
    net = np.zeros_like(net) if tenths[1] == 0 else net
    if use_swt:
        orc = (sw >= swt) | (th >= tht) | ((sw + th) / 2 >= swth) | (net >= nt)
        conf = np.where(orc, 1.0, nw * net + sww * sw + thw * th)
    else:
        conf = net
    head = (conf > thr) | tagged
    return [bool(len(r) > 0 and int(head[r].sum()) / len(r) >= tlp) for r in region_lines]


def _page_inputs(page):
    sw, th, net, use = he.heading_confidences(_values(page), _lines(page))
    index = {d["id"]: i for i, d in enumerate(page["lines"])}
    regions = [np.array([index[i] for i in r], np.int64) for r in page["regions"]]
    return sw, th, net, use, regions


def test_grid_enumeration_matches_the_reference():
    g = GOLD["grid"]
    heights, tenths = he.grid_settings()
    assert len(tenths) == g["n_settings"] == 449064
    assert len(he.grid_outer()) == g["n_outer"] == 37422
    rows = [(int(h),) + he.setting_floats(t) for h, t in zip(heights, tenths)]
    assert hashlib.sha256(canonical(rows).encode()).hexdigest() == g["sha256"]
    for s in g["samples"]:
        mine = he.grid_inner(*s["outer"])
        assert [list(r) for r in mine] == s["settings"]
    assert any(s["outer"][2] == 0 for s in g["samples"]) and any(s["outer"][2] == 10 for s in g["samples"])
    assert any(s["outer"][4] != s["outer"][5] for s in g["samples"])


def test_confidences_and_fusion_restatement_give_the_reference_labels():
    pages = GOLD["pages"]
    assert pages == hc.pages()
    inputs = [_page_inputs(p) for p in pages]
    n_head = 0
    for st in GOLD["settings"]:
        for p, (sw, th, net, use, regions), lab in zip(pages, inputs, st["labels"]):
            got = "".join("1" if x else "0" for x in fuse_regions(sw, th, net, use, np.zeros(len(sw), bool), regions, st["tenths"]))
            assert got == lab, (p["name"], st["tenths"])
            n_head += got.count("1")
    assert n_head > 0


def _case_page(tmp_path, case):
    """a PAGE-XML of a host golden heading case (lines without an outline have no Coords)"""
    from citlab_article_separation_new_amd.page_xml import Page
    regs = []
    for r, reg in enumerate(case["regions"]):
        ls = "".join(f'<TextLine id="{i}">' + ('<Coords points="10,10 70,10 70,40 10,40"/>' if case["has_outline"][i] else "")
                     + '</TextLine>' for i in reg)
        regs.append(f'<TextRegion id="r{r}"><Coords points="0,0 90,0 90,90 0,90"/>{ls}</TextRegion>')
    p = tmp_path / "case.xml"
    p.write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2013-07-15">'
                 '<Page imageFilename="x.png" imageWidth="100" imageHeight="100">' + "".join(regs) + '</Page></PcGts>')
    return Page(str(p))


def test_confidence_helper_and_restatement_equal_apply_heading_values(tmp_path):
    """the product's apply_heading_values on the host golden's heading cases (recorded from the reference) and the
    confidence helper + the restatement of the fusion rule on the same measurements give the same lines and regions"""
    from citlab_article_separation_new_amd.heading_net_post_processor import apply_heading_values
    gold = json.load(open(os.path.join(HERE, "golden", "host_goldens.json")))["heading"]
    for case in gold:
        ids = [i for r in case["regions"] for i in r]
        meas = case["measurements"]
        values = ({i: (meas[i][0] if case["has_outline"][i] else 0) for i in ids},
                  {i: (meas[i][1] if case["has_outline"][i] else 0) for i in ids},
                  {i: meas[i][2] for i in ids})           # (the recorded net confidence of every line, as the golden fed it)
        if case["weight_dict"]["net"] == 0:
            values[2].update({i: 0 for i in ids})
        w, t = case["weight_dict"], case["thresh_dict"]

        page = _case_page(tmp_path, case)
        writer = types.SimpleNamespace(page_object=page, save_page_xml=lambda path: None)
        lines = page.get_textlines()
        apply_heading_values(writer, lines, values, w, case["threshold"], t, case["text_line_percentage"], "unused")
        product_heads = sorted(tl.id for tl in lines if tl.get_semantic_type() == "heading")
        product_types = {r.id: r.node.get("type") for r in page.get_text_regions()}
        assert product_heads == case["heading_lines"] and product_types == case["region_types"]

        sw, th, net, use = he.heading_confidences(values, lines)
        # the host golden's settings are not all tenths: the restatement with the same floats
        thr, nw, sww, thw = case["threshold"], w["net"], w["stroke_width"], w["text_height"]
        if use:
            orc = (sw >= t["stroke_width_thresh"]) | (th >= t["text_height_thresh"]) | ((sw + th) / 2 >= t["sw_th_thresh"]) | \
                  (net >= t["net_thresh"])
            conf = np.where(orc, 1.0, nw * net + sww * sw + thw * th)
        else:
            conf = net
        heads = sorted(i for i, c in zip(ids, conf) if c > thr)
        assert heads == product_heads
        types_ = {f"r{r}": "heading" if reg and sum(1 for i in reg if i in heads) / len(reg) >= case["text_line_percentage"]
                  else "paragraph" for r, reg in enumerate(case["regions"])}
        assert types_ == product_types


def _counts(gt, lab):
    return he.counts_from_labels(gt, [c == "1" for c in lab])


def test_metrics_bit_equal_to_sklearn():
    table = GOLD["metric_table"]
    counts = np.array([e["counts"] for e in table], np.int64)
    got = he.page_metrics(counts)
    for e, g in zip(table, got):
        assert json.dumps([float(x) for x in g]) == json.dumps(e["values"]), e["counts"]
    assert any(sum(e["counts"]) == 0 for e in table)                      # the page without regions (nan macro / weighted)
    assert any(e["counts"][0] + e["counts"][2] == 0 and e["counts"][1] > 0 for e in table)   # a label in one list only


def test_averages_bit_equal_to_the_reference():
    pages = GOLD["pages"]
    counts = np.array([[_counts(p["gt"], lab) for p, lab in zip(pages, st["labels"])] for st in GOLD["settings"]], np.int64)
    avg = he.average_metrics(he.page_metrics(counts))
    for st, a in zip(GOLD["settings"], avg):
        assert json.dumps([float(x) for x in a]) == json.dumps(st["averages"]), st["tenths"]


def test_log_text_and_names_byte_equal():
    pages = GOLD["pages"]
    assert len(GOLD["logs"]) >= 5
    for log in GOLD["logs"]:
        st = GOLD["settings"][log["setting"]]
        s = he.setting_floats(st["tenths"])
        counts = np.array([_counts(p["gt"], lab) for p, lab in zip(pages, st["labels"])], np.int64)
        per_page = he.page_metrics(counts)
        assert json.dumps(per_page.tolist()) == json.dumps(log["per_page"])
        assert he.log_file_name(st["fixed_height"], *s[:7], s[8]) == log["name"]
        assert he.log_text(st["fixed_height"], s, GOLD["image_paths"], per_page, he.average_metrics(per_page)) == log["text"]


def test_region_helpers(tmp_path):
    from citlab_article_separation_new_amd.page_xml import Page
    p = tmp_path / "p.xml"
    p.write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2013-07-15">'
                 '<Page imageFilename="x.png" imageWidth="10" imageHeight="10">'
                 '<TextRegion id="a" type="heading"><TextLine id="a1" custom="structure {semantic_type:heading;}"/><TextLine id="a2"/></TextRegion>'
                 '<TextRegion id="b" type="paragraph"><TextLine id="b1" custom="structure {semantic_type:heading;}"/></TextRegion>'
                 '</Page></PcGts>')
    page = Page(str(p))
    regs = he.get_heading_regions(page)
    assert [r.id for r in regs] == ["a"]
    assert [t.id for t in he.get_heading_text_lines(regs)] == ["a1", "a2"]
    assert [t.id for t in he.get_heading_text_line_by_custom_type(regs)] == ["a1"]
    pr = he.PageRegions(page)
    assert pr.region_lines == [[0, 1], [2]] and pr.gt.tolist() == [True, False] and pr.tagged.tolist() == [True, False, True]


BASE = ["--path_to_gt_list", "gt.lst", "--path_to_pb", "net.pb", "--fixed_height", "600", "--threshold", "0.5",
        "--net_weight", "0.3", "--stroke_width_weight", "0.3", "--text_height_weight", "0.4", "--net_thresh", "0.9",
        "--stroke_width_thresh", "0.9", "--text_height_thresh", "0.8", "--sw_th_thresh", "0.7", "--text_line_percentage", "0.8",
        "--log_file_folder", "logs"]


def test_flags(capsys):
    a = he.parse_args(BASE)
    assert a.fixed_height == 600 and a.threshold == 0.5 and a.gpu_devices == "0" and a.log_file_folder == "logs"
    for flag in ("--fixed_height", "--sw_th_thresh", "--net_weight"):
        i = BASE.index(flag)
        with pytest.raises(SystemExit):
            he.parse_args(BASE[:i] + BASE[i + 2:])
        assert flag in capsys.readouterr().err
    from citlab_article_separation_new_amd import heading_evaluation_grid_search as gs
    g = gs.build_parser().parse_args(["--path_to_gt_list", "a", "--path_to_pb", "b", "--log_file_folder", "c"])
    assert g.fixed_heights == list(range(600, 1300, 100)) and g.num_processes == 8 and not g.no_setting_logs and g.results is None


def test_region_count_mismatch_names_the_file(tmp_path):
    page = tmp_path / "page"
    page.mkdir()
    head = ('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2013-07-15">'
            '<Page imageFilename="x.png" imageWidth="10" imageHeight="10">')
    (page / "s0.xml").write_text(head + '<TextRegion id="a" type="heading"/><TextRegion id="b"/></Page></PcGts>')
    (page / "s0.xml.xml").write_text(head + '<TextRegion id="a" type="heading"/></Page></PcGts>')
    with pytest.raises(ValueError, match="s0.xml"):
        he.hypothesis_labels([str(tmp_path / "s0.png")])


def test_grid_pages_layout():
    gp = he.GridPages([(np.array([0.1, 0.2]), np.array([0.3, 0.4]), np.array([0.5, 0.6]), True, [[1, 0], []], [True, False], None),
                       (np.zeros(0), np.zeros(0), np.zeros(0), False, [], [], None)])
    assert gp.line_off.tolist() == [0, 2, 2] and gp.reg_off.tolist() == [0, 2, 2]
    assert gp.reg_line_off.tolist() == [0, 2, 2] and gp.reg_lines.tolist() == [1, 0]
    assert gp.gt.tolist() == [1, 0] and gp.use_swt.tolist() == [1, 0] and gp.tagged.tolist() == [0, 0]
