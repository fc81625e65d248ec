"""Split / merge comparison of article separations: host restatement of ``as_eval/asQcTools/asCompTools.py`` on ``page_xml.Page``.

``SepPageBlComper`` is the one-pair definition (pure Python): a ground truth PAGE-XML against a hypothesis, both read as
partitions of their baselines (text lines) into articles.  ``cluster_grid.ClusterGrid.run_compare`` computes the same counts
for many (page, setting) pairs on the device and is tested against this class.  ``SepPageCompDict`` collects results
(CSV, sqlite, pickle), ``CompDictEvaler`` ranks the methods.  Pinned by ``tests/golden/as_eval_golden.json``.

Quirks of the reference that are kept (the counts depend on them):
  * ``niBlDict``'s keys and ``canonicalBlPartition`` come from the page's unfiltered article dict: an article emptied by
    ``removeBlSet`` still counts in ``gtNIs``, and removed lines stay in the canonical blocks (such a block is never correct);
  * ground truth lines that are a strict subset of the hypothesis lines raise ``AssertionError``; lines the hypothesis lacks
    are dropped from the ground truth, lines the ground truth lacks stay in the hypothesis;
  * the "inf" partition (common refinement) is walked over the ground truth lines only;
  * ``path2method`` joins ``parts[-5]`` and ``parts[-1]`` of the hypothesis file's folder;
  * methods are ranked by the tuple ``(dist, -corrects)`` with ``<=`` (a method also "wins" against itself).
``winnerStat2xlsx`` is not available: it needs ``openpyxl``, which this project does not depend on.
"""
import csv
import logging
import pickle
import sqlite3
from pathlib import Path, PurePath

import numpy as np

from .page_xml import Page

logger = logging.getLogger(__name__)


class SeparatedPage(Page):
    """PAGE-XML read as a partition of its baselines into articles"""

    def __init__(self, xmlFilePath):
        super().__init__(str(xmlFilePath))
        self.xmlFilePath = xmlFilePath
        self._blIgnore = set()
        self._reInit()

    def _reInit(self):
        self.blNiDict = {}
        self.niBlDict = {ni: [] for ni in self.get_article_dict()}
        for bl in self.get_textlines():
            if bl.id in self._blIgnore:
                continue
            ni = bl.get_article_id()
            self.blNiDict[bl.id] = ni
            self.niBlDict[ni].append(bl.id)
        for ni in self.niBlDict:
            self.niBlDict[ni].sort()
        self._canBlPart = None

    def removeBlSet(self, blSet):
        """leave these baselines out of blNiDict / niBlDict (not out of the canonical partition)"""
        self._blIgnore.update(blSet)
        self._reInit()

    def canonicalBlPartition(self):
        """sorted list of the articles' sorted baseline ids, from the unfiltered article dict"""
        if self._canBlPart is None:
            self._canBlPart = sorted(sorted(bl.id for bl in lines) for lines in self.get_article_dict().values())
        return self._canBlPart


class SepPageComparison:
    """the six counters of one (ground truth, hypothesis) pair"""

    def __init__(self):
        self.gtNIs = None
        self.hypNIs = None
        self.corrects = None
        self.splits = None
        self.merges = None
        self.dist = None

    @classmethod
    def from_counts(cls, gtNIs, hypNIs, n_inf, corrects):
        """the host arithmetic behind the device counts: splits = n_inf - gtNIs, merges = hypNIs - n_inf"""
        c = cls()
        c.gtNIs, c.hypNIs, c.corrects = int(gtNIs), int(hypNIs), int(corrects)
        c.splits = int(n_inf) - c.gtNIs
        c.merges = c.hypNIs - int(n_inf)
        c.dist = c.splits - c.merges
        return c

    def __str__(self):
        return str(self.__dict__)

    def __eq__(self, other):
        return isinstance(other, SepPageComparison) and self.__dict__ == other.__dict__

    def dataDict(self):
        return self.__dict__

    def loadDict(self, dataDict):
        for member in self.__dict__:
            setattr(self, member, int(dataDict.get(member, None)))

    def checkConsistency(self):
        return self.gtNIs + self.splits + self.merges == self.hypNIs


class SepPageComper:
    """root class of the comparison engines"""

    def __init__(self):
        self._hypSepPage = None
        self._gtSepPage = None
        self._altGtDict = {}
        self.comparison = None

    def loadGT(self, xmlFilePath):
        self._gtSepPage = SeparatedPage(xmlFilePath)

    def compareTo(self, xmlFilePath):
        self._hypSepPage = SeparatedPage(xmlFilePath)
        self.comparison = self._compare()
        return self.comparison

    def _compare(self):
        raise NotImplementedError('Method not yet been implemented!')


class SepPageBlComper(SepPageComper):
    """comparison by baseline partitions"""

    def _compare(self):
        hyp = self._hypSepPage
        gt = self._gtSepPage
        hyp_lines = {tl.id for tl in hyp.get_textlines()}
        gt_lines = {tl.id for tl in gt.get_textlines()}
        if gt_lines != hyp_lines:
            if gt_lines.issubset(hyp_lines):
                raise AssertionError('cannot compare: inconsistent baselines')
            missing = gt_lines - hyp_lines
            gt_lines = gt_lines - missing
            key = ''.join(missing)
            logger.debug(f'ignoring inconsistent baselines {key}')
            gt = self._altGtDict.get(key)
            if gt is None:
                gt = SeparatedPage(self._gtSepPage.xmlFilePath)
                gt.removeBlSet(missing)
                self._altGtDict[key] = gt
        res = SepPageComparison()
        res.gtNIs = len(gt.niBlDict)
        res.hypNIs = len(hyp.niBlDict)
        hyp_blocks = hyp.canonicalBlPartition()
        res.corrects = sum(1 for block in gt.canonicalBlPartition() if block in hyp_blocks)
        n_inf = 0
        covered = set()
        for bl in gt_lines:
            if bl in covered:
                continue
            common = set(gt.niBlDict[gt.blNiDict[bl]]) & set(hyp.niBlDict[hyp.blNiDict[bl]])
            n_inf += 1
            covered |= common
        res.splits = n_inf - res.gtNIs
        res.merges = res.hypNIs - n_inf
        res.dist = res.splits - res.merges
        return res


def comparison_tables(hyp_page, gt_page):
    """What the device comparison (asep_cluster_grid_run) reads for one page, from the hypothesis' structure (any labels) and
    the ground truth: -> dict with ``line_node`` (per hypothesis line, the index of the TextRegion it hangs in), ``line_gt`` (its
    dense ground truth article or -1), ``blocks`` (the ground truth's canonical blocks as hypothesis line indices, without the
    blocks that hold a line the hypothesis lacks), ``gtNIs`` and ``inconsistent`` (SepPageBlComper raises AssertionError)."""
    hyp = hyp_page if isinstance(hyp_page, Page) else Page(str(hyp_page))
    gt = gt_page if isinstance(gt_page, Page) else Page(str(gt_page))
    line_index, line_node = {}, []
    for k, region in enumerate(hyp.get_regions().get("TextRegion", [])):
        for tl in region.text_lines:
            line_index[tl.id] = len(line_node)
            line_node.append(k)
    hyp_ids = [tl.id for tl in hyp.get_textlines()]
    if set(hyp_ids) != set(line_index) or len(hyp_ids) != len(line_node):
        raise ValueError("the hypothesis page has text lines outside its text regions, or line ids that repeat")
    articles = gt.get_article_dict()
    gt_ids = {tl.id for lines in articles.values() for tl in lines}
    line_gt = np.full(len(line_node), -1, np.int32)
    blocks = []
    n_present = 0                      # articles are numbered over those with a line in the hypothesis: an index is below the line count
    for lines in articles.values():
        ids = sorted(tl.id for tl in lines)
        present = [line_index[i] for i in ids if i in line_index]
        if present:
            line_gt[present] = n_present
            n_present += 1
        if len(present) == len(ids):
            blocks.append(present)
    return {"line_node": np.asarray(line_node, np.int32), "line_gt": line_gt, "blocks": blocks, "gtNIs": len(articles),
            "inconsistent": gt_ids != set(hyp_ids) and gt_ids.issubset(hyp_ids)}


class SepPageCompDict(dict):
    """{dataSet: {gtXML: {hypXML: SepPageComparison}}}"""
    fieldNames = ['dataSet', 'method', 'gtXML', 'hypXML', *SepPageComparison().dataDict().keys()]

    @classmethod
    def path2method(cls, path):
        parts = PurePath(path).parent.parts
        return str(parts[-5]) + "/" + str(parts[-1])

    def addItem(self, dataSet, gtXML, hypXML, spcDict):
        self.setdefault(dataSet, {}).setdefault(gtXML, {})[hypXML] = spcDict

    def loadPickle(self, dataSetLabel, pickleFilePath):
        with Path(pickleFilePath).open(mode='rb') as f:
            self[dataSetLabel] = pickle.load(f)

    def cleanup(self, inclList):
        """entries of methods outside the list become None"""
        for dataDict in self.values():
            for gtDict in dataDict.values():
                for hypXML in gtDict:
                    if self.path2method(hypXML) not in inclList:
                        gtDict[hypXML] = None

    def rows(self):
        """(dataSet, method, gtXML, hypXML, comparison) in insertion order"""
        for dataSet, dataDict in self.items():
            for gtXML, gtDict in dataDict.items():
                for hypXML, comp in gtDict.items():
                    yield dataSet, self.path2method(hypXML), gtXML, hypXML, comp

    def loadCSV(self, csvFilePath, inclList):
        with Path(csvFilePath).open(mode='rt') as f:
            for row in csv.DictReader(f):
                if row.get('method').lower() in inclList:
                    spc = SepPageComparison()
                    spc.loadDict(row)
                    self.setdefault(row.get('dataSet'), {}).setdefault(row.get('gtXML'), {})[row.get('hypXML')] = spc

    def expSqlite(self, dbFilePath, dbTableName):
        """(the rows go into the table allComps whatever dbTableName is, as in the reference)"""
        fields = ', '.join(self.fieldNames)
        con = sqlite3.connect(str(dbFilePath))
        cur = con.cursor()
        try:
            cur.execute(f'DROP TABLE {dbTableName}')
        except sqlite3.Error:
            pass
        cur.execute(f'CREATE TABLE {dbTableName} ({fields})')
        for dataSet, method, gtXML, hypXML, comp in self.rows():
            values = [f'"{dataSet}"', f'"{method}"', f'"{gtXML}"', f'"{hypXML}"'] + [str(v) for v in comp.dataDict().values()]
            cur.execute(f"INSERT INTO allComps ({fields}) VALUES ({', '.join(values)})")
        con.commit()
        con.close()

    def expCsv(self, csvFilePath):
        with Path(csvFilePath).open(mode='wt', encoding='utf8', newline='') as f:
            writer = csv.DictWriter(f, fieldnames=self.fieldNames)
            writer.writeheader()
            for dataSet, method, gtXML, hypXML, comp in self.rows():
                row = {'dataSet': dataSet, 'method': method, 'gtXML': gtXML, 'hypXML': hypXML}
                row.update(comp.dataDict())
                writer.writerow(row)


class CompDictEvaler:
    """ranks the methods of a SepPageCompDict: method0 scores a point against method1 on a page when its
    (dist, -corrects) is <= method1's"""

    def __init__(self, spcDict):
        self.spcDict = spcDict
        self.winnerStatDict = {}
        self.winnerDict = {}

    def countWinnerStat(self):
        for dataSet, dataDict in self.spcDict.items():
            stat = self.winnerStatDict[dataSet] = {}
            for gtDict in dataDict.values():
                for hyp0, c0 in gtDict.items():
                    if not c0:
                        continue
                    m0 = SepPageCompDict.path2method(hyp0)
                    stat.setdefault(m0, {'all': 0})
                    for hyp1, c1 in gtDict.items():
                        if not c1:
                            continue
                        m1 = SepPageCompDict.path2method(hyp1)
                        stat[m0].setdefault(m1, 0)
                        if (c0.dist, -c0.corrects) <= (c1.dist, -c1.corrects):
                            stat[m0][m1] += 1
                            stat[m0]['all'] += 1

    def calcWinnerDict(self):
        """knock-out table: per method its 'all' score, then the score without the points against each round's loser"""
        if len(self.winnerStatDict) == 0:
            self.countWinnerStat()
        for dataSet, stat in self.winnerStatDict.items():
            table = self.winnerDict[dataSet] = {}
            for method in stat.keys():
                table[method] = [stat[method]['all']]
            methods = sorted(stat.keys(), key=lambda m: table[m][-1])
            table['_max'] = [table[methods[-1]][-1]]
            while len(methods) > 1:
                loser = methods.pop(0)
                for m in methods:
                    table[m].append(table[m][-1] - stat[m][loser])
                methods = sorted(methods, key=lambda m: table[m][-1])
                table['_max'].append(table[methods[-1]][-1])

    def winnerStat2xlsx(self, xlsxFilePath):
        raise NotImplementedError("the XLSX export needs openpyxl, which this project does not depend on: "
                                  "use winner_csv_rows / run_compare's <name>_winner.csv")

    def winner_csv_rows(self):
        """the winner table as rows: dataSet, method, then the method's knock-out scores (longest first)"""
        if len(self.winnerDict) == 0:
            self.calcWinnerDict()
        rows = []
        for dataSet, table in self.winnerDict.items():
            methods = sorted((m for m in table if not m.startswith('_')), key=lambda m: len(table[m]), reverse=True)
            rows.extend([dataSet, m, *table[m]] for m in methods)
        return rows


def winner_all_counts(dist, corrects):
    """countWinnerStat's 'all' column with numpy.  ``dist`` / ``corrects``: int arrays [pages, methods] (every method compared
    on every page).  Per page the keys (dist, -corrects) are sorted and each method scores the number of methods whose key is
    >= its own (itself included); -> int64 [methods].  n log n per page where the double loop is quadratic."""
    dist = np.asarray(dist, np.int64)
    corrects = np.asarray(corrects, np.int64)
    span = int(corrects.max(initial=0) - corrects.min(initial=0)) + 1
    key = dist * span - corrects                       # order of the tuples (dist, -corrects)
    total = np.zeros(key.shape[1], np.int64)
    for row in key:
        ordered = np.sort(row)
        total += len(row) - np.searchsorted(ordered, row, side="left")
    return total
