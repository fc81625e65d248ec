"""Generates tests/golden/as_eval_golden.json (data only) from the reference's as_eval/asQcTools/asCompTools.py.

The reference module is imported through ref_import.install_stubs() plus a placeholder for openpyxl (only its XLSX export needs
it).  ``Page.__init__`` is replaced so that a SeparatedPage is built from an in-memory table of (line id, article id) keyed by
path; everything that is recorded (the six counts or the exception, winnerStatDict / winnerDict) is computed by the reference's
own SeparatedPage / SepPageBlComper / CompDictEvaler.  Run from the repository root: python tests/golden/make_as_eval_golden.py"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import as_eval_cases  # noqa: E402
import ref_import  # noqa: E402


class _Line:
    def __init__(self, line_id, article):
        self.id = line_id
        self._article = article

    def get_article_id(self):
        return self._article


def main():
    ref_import.install_stubs()
    for name in ("openpyxl", "openpyxl.utils", "openpyxl.styles"):
        stub = types.ModuleType(name)
        for attr in ("Workbook", "get_column_letter", "Font", "Alignment", "Border", "Side"):
            setattr(stub, attr, None)
        sys.modules.setdefault(name, stub)
    from as_eval.asQcTools import asCompTools as act

    tables = {}

    def page_init(self, path_to_xml=None, *a, **k):
        self.textlines = [_Line(i, art) for i, art in tables[str(path_to_xml)]]

    act.Page.__init__ = page_init
    act.Page.get_textlines = lambda self, *a, **k: self.textlines

    out_cases = []
    for name, gt, hyp in as_eval_cases.cases():
        tables[f"{name}/gt.xml"], tables[f"{name}/hyp.xml"] = gt, hyp
        comper = act.SepPageBlComper()
        comper.loadGT(f"{name}/gt.xml")
        try:
            expect = dict(comper.compareTo(f"{name}/hyp.xml").dataDict())
        except AssertionError as e:
            expect = {"error": "AssertionError", "message": str(e)}
        out_cases.append({"name": name, "gt": [list(e) for e in gt], "hyp": [list(e) for e in hyp], "expect": expect})

    results = act.SepPageCompDict()
    for p, row in enumerate(as_eval_cases.WINNER_TABLE):
        for m, (dist, corrects) in zip(as_eval_cases.WINNER_METHODS, row):
            c = act.SepPageComparison()
            c.loadDict({"gtNIs": 5, "hypNIs": 5 - dist, "corrects": corrects, "splits": 0, "merges": -dist, "dist": dist})
            results.addItem("set", as_eval_cases.WINNER_GT.format(p=p), as_eval_cases.WINNER_HYP.format(m=m, p=p), c)
    evaler = act.CompDictEvaler(results)
    evaler.calcWinnerDict()
    golden = {"cases": out_cases, "winner": {"winnerStatDict": evaler.winnerStatDict, "winnerDict": evaler.winnerDict,
                                             "method_of_first": act.SepPageCompDict.path2method(
                                                 as_eval_cases.WINNER_HYP.format(m=as_eval_cases.WINNER_METHODS[0], p=0))}}
    with open(os.path.join(HERE, "as_eval_golden.json"), "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
    n_err = sum("error" in c["expect"] for c in out_cases)
    print(f"wrote {len(out_cases)} cases ({n_err} raise) and the winner tables")


if __name__ == "__main__":
    main()
