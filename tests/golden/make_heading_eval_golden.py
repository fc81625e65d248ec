"""Golden of the heading evaluation (tests/golden/heading_eval_golden.json), from the imported reference on the CPU.

1. The grid of heading_evaluation_grid_search.py: its __main__ run under runpy with ProcessPoolExecutor replaced by a
   recorder (the outer tuples), then run_grid_search of every tuple with os.system captured (the commands, parsed back to
   numbers).  Stored: the count, a SHA-256 of the canonical list and the full lists of some outer tuples.
2. Scoring and log text: heading_evaluation.py's __main__ under runpy for every setting of heading_eval_cases.settings(),
   with HeadingNetPostProcessor.run replaced by a driver of the reference's own to_page_xml fed the recorded per-line
   measurements of heading_eval_cases.pages() (a recording PAGE writer, as make_host_goldens.py does) and Page replaced
   by the GT pages of the cases.  sklearn computes the scores.  Stored: per setting the per-page hypothesis labels and
   the 12 averages; the per-page values of every distinct (TP, FP, FN, TN) seen; for a few settings the log text and name.

Run:  python tests/golden/make_heading_eval_golden.py
"""
import concurrent.futures
import hashlib
import json
import os
import runpy
import shlex
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install_stubs()

import heading_eval_cases as hc  # noqa: E402
from article_separation.image_segmentation.net_post_processing import heading_net_post_processor as rhead  # noqa: E402
from article_separation.image_segmentation.net_post_processing import region_net_post_processor_base as rbase  # noqa: E402
from python_util.io import file_loader  # noqa: E402
from python_util.parser.xml.page import page as rpage  # noqa: E402

NET = os.path.dirname(rhead.__file__) + os.sep          # the reference's net_post_processing scripts
FIELDS = ("fixed_height", "threshold", "net_weight", "stroke_width_weight", "text_height_weight", "net_thresh",
          "stroke_width_thresh", "text_height_thresh", "sw_th_thresh", "text_line_percentage")


def canonical(rows):
    """rows of (fixed_height int, 9 floats) -> the text the SHA-256 is taken of"""
    return "\n".join(",".join([str(int(r[0]))] + [repr(float(x)) for x in r[1:]]) for r in rows)


def grid_golden():
    class Recorder:
        calls = []

        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def submit(self, fn, *args):
            Recorder.calls.append(args)

    saved_ppe, saved_argv, saved_system = concurrent.futures.ProcessPoolExecutor, sys.argv, os.system
    concurrent.futures.ProcessPoolExecutor = Recorder
    sys.argv = ["grid", "--path_to_gt_list", "GT.lst", "--path_to_pb", "NET.pb", "--log_file_folder", "LOGS"]
    try:
        g = runpy.run_path(NET + "heading_evaluation_grid_search.py", run_name="__main__")
    finally:
        concurrent.futures.ProcessPoolExecutor, sys.argv = saved_ppe, saved_argv
    outer = list(Recorder.calls)
    commands = []
    os.system = commands.append
    rows, per_outer = [], []
    try:
        for args in outer:
            commands.clear()
            g["run_grid_search"](*args)
            parsed = []
            for cmd in commands:
                tok = shlex.split(cmd)
                kv = {tok[i][2:]: tok[i + 1] for i in range(len(tok)) if tok[i].startswith("--")}
                parsed.append([int(kv["fixed_height"])] + [float(kv[k]) for k in FIELDS[1:]])
            per_outer.append(parsed)
            rows.extend(parsed)
    finally:
        os.system = saved_system
    samples = []
    pick = [i for i, a in enumerate(outer) if a[2] == 0][:3] + [i for i, a in enumerate(outer) if a[2] == 10][:3] + \
           [i for i, a in enumerate(outer) if a[4] != a[5]][::3000][:10] + list(range(0, len(outer), 9000))
    for i in sorted(set(pick)):
        samples.append({"outer": [outer[i][0], outer[i][1]] + list(outer[i][2:]), "settings": per_outer[i]})
    return {"n_outer": len(outer), "n_settings": len(rows), "sha256": hashlib.sha256(canonical(rows).encode()).hexdigest(),
            "samples": samples}


class GTRegion:
    def __init__(self, rid, lines, region_type):
        self.id, self.text_lines, self.region_type = rid, lines, region_type


class GTPage:
    """python_util Page of a case page: what heading_evaluation's __main__ reads (get_text_regions().region_type)"""

    def __init__(self, case):
        self.regions = [GTRegion(f"r{i}", [], "heading" if g else "paragraph") for i, g in enumerate(case["gt"])]

    def get_text_regions(self):
        return self.regions


def scoring_golden():
    pages, settings = hc.pages(), hc.settings()
    by_path = {f"/data/{p['name']}.png": p for p in pages}
    image_paths = list(by_path)

    class Line:
        def __init__(self, d):
            self.id = d["id"]
            self.surr_p = [(0, 0), (1, 1)] if d["outline"] else None
            self.custom = {}

    class FakeNode:
        def __init__(self, obj):
            self.obj, self.attrs = obj, {}

        def set(self, k, v):
            self.attrs[k] = v

    def driver_run(self, gpu_devices):
        results = []
        for path in image_paths:
            case = by_path[path]
            lines = {d["id"]: Line(d) for d in case["lines"]}
            meas = {d["id"]: (d["sw"], d["th"], d["net"]) for d in case["lines"]}
            reg_lines = [[lines[i] for i in r] for r in case["regions"]]
            all_lines = [ln for r in reg_lines for ln in r]

            class FakePageObject:
                page_doc = None

                def __init__(self):
                    self.regions = [type("R", (), {"id": f"r{r}", "text_lines": ls})() for r, ls in enumerate(reg_lines)]
                    self.nodes = {}

                def get_textlines(self):
                    return all_lines

                def get_text_regions(self):
                    return self.regions

                def get_child_by_id(self, doc, cid):
                    obj = next((x for x in all_lines + self.regions if x.id == cid))
                    return [self.nodes.setdefault(cid, FakeNode(obj))]

                def set_custom_attr(self, node, key, sub, value):
                    node.obj.custom.setdefault(key, {})[sub] = value

            class FakeWriter:
                def __init__(self, *a, **k):
                    self.page_object, self.scaling_factor = FakePageObject(), 1.0

                def save_page_xml(self, path):
                    pass

            rhead.RegionToPageWriter = FakeWriter
            self.get_swt_features_image = lambda image_path: "swt"
            self.get_swt_features_textline = lambda swt, tl: meas[tl.id][:2]
            self.get_net_prob_for_text_line = lambda netp, tl, sf: meas[tl.id][2]
            po = self.to_page_xml(path + ".xml", image_path=path, net_output_post="net")
            types = [po.nodes[f"r{r}"].attrs.get("type") for r in range(len(reg_lines))]
            results.append(type("HypPage", (), {"get_text_regions": lambda s, t=types: [GTRegion("", [], x) for x in t]})())
        return results

    def base_init(self, image_list, path_to_pb, fixed_height, scaling_factor, *a, **k):
        self.fixed_height, self.scaling_factor = fixed_height, scaling_factor

    rbase.RegionNetPostProcessor.__init__ = base_init
    rhead.StrokeWidthDistanceTransform = lambda **k: None
    rhead.HeadingNetPostProcessor.run = driver_run
    file_loader.load_list_file = lambda p: list(image_paths)
    file_loader.get_page_path = lambda p: p + "_page"
    rpage.Page = lambda xml_path: GTPage(by_path[xml_path[:-len("_page")]])

    names = ("recall_scores_bin", "recall_scores_micro", "recall_scores_macro", "recall_scores_weighted",
             "precision_scores_bin", "precision_scores_micro", "precision_scores_macro", "precision_scores_weighted",
             "f1_scores_bin", "f1_scores_micro", "f1_scores_macro", "f1_scores_weighted")
    avg_names = ("avg_recall_bin", "avg_recall_micro", "avg_recall_macro", "avg_recall_weighted", "avg_precision_bin",
                 "avg_precision_micro", "avg_precision_macro", "avg_precision_weighted", "avg_f1_bin", "avg_f1_micro",
                 "avg_f1_macro", "avg_f1_weighted")
    out_settings, table, logs = [], {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for si, st in enumerate(settings):
            fl = [k / 10 for k in st]
            fixed_height = 600 + 100 * (si % 7)
            argv = ["heading_evaluation.py", "--path_to_gt_list", "GT.lst", "--path_to_pb", "NET.pb", "--fixed_height", str(fixed_height),
                    "--threshold", repr(fl[0]), "--net_weight", repr(fl[1]), "--stroke_width_weight", repr(fl[2]),
                    "--text_height_weight", repr(fl[3]), "--gpu_devices", "", "--log_file_folder", tmp, "--net_thresh", repr(fl[4]),
                    "--stroke_width_thresh", repr(fl[5]), "--text_height_thresh", repr(fl[6]), "--sw_th_thresh", repr(fl[7]),
                    "--text_line_percentage", repr(fl[8])]
            saved = sys.argv
            sys.argv = argv
            captured = {}
            orig_run = rhead.HeadingNetPostProcessor.run

            def run_and_keep(self, gpu, _o=orig_run):
                captured["hyp"] = _o(self, gpu)
                return captured["hyp"]
            rhead.HeadingNetPostProcessor.run = run_and_keep
            try:
                g = runpy.run_path(NET + "heading_evaluation.py", run_name="__main__")
            finally:
                sys.argv = saved
                rhead.HeadingNetPostProcessor.run = orig_run
            labels = ["".join("1" if tr.region_type == "heading" else "0" for tr in hp.get_text_regions()) for hp in captured["hyp"]]
            per_page = [[float(g[n][k]) for n in names] for k in range(len(pages))]
            for p, lab, vals in zip(pages, labels, per_page):
                gt = p["gt"]
                c = (sum(1 for a, b in zip(gt, lab) if a and b == "1"), sum(1 for a, b in zip(gt, lab) if not a and b == "1"),
                     sum(1 for a, b in zip(gt, lab) if a and b == "0"), sum(1 for a, b in zip(gt, lab) if not a and b == "0"))
                key = ",".join(map(str, c))
                prev = table.setdefault(key, vals)
                assert json.dumps(prev) == json.dumps(vals), (key, prev, vals)
            out_settings.append({"fixed_height": fixed_height, "tenths": list(st), "labels": labels,
                                 "averages": [float(g[n]) for n in avg_names]})
            if si < hc.LOG_SETTINGS or st[1] == 0 and len(logs) < hc.LOG_SETTINGS + 1:
                name = os.path.basename(g["log_file_name"])
                with open(g["log_file_name"]) as f:
                    logs.append({"setting": si, "name": name, "text": f.read(), "per_page": per_page})
    return {"image_paths": image_paths, "settings": out_settings,
            "metric_table": [{"counts": [int(x) for x in k.split(",")], "values": v} for k, v in sorted(table.items())],
            "logs": logs}


def main():
    out = {"grid": grid_golden()}
    out.update(scoring_golden())
    out["pages"] = hc.pages()
    path = os.path.join(HERE, "heading_eval_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes;", out["grid"]["n_outer"], "outer tuples,", out["grid"]["n_settings"], "settings,",
          len(out["settings"]), "scored settings,", len(out["metric_table"]), "count tuples")


if __name__ == "__main__":
    main()
