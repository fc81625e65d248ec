"""Grid search over the ``dbscan`` clustering settings: every (page, setting) clustered and compared with the ground truth in
one device call (``ClusterGrid.run_compare``).  No counterpart in the reference, which runs ``run_conf_to_cluster`` once per
setting and ``run_compare`` over the folders.

    python -m citlab_article_separation_new_amd.run_cluster_grid_search --eval_list confidences.lst --gt_list gt.lst \\
        --confidence_thresholds 0:1:0.05 --cluster_agreement_thresholds 0:1:0.05 --min_neighbors 1 --out_dir eval

``--eval_list`` holds ``confidences/<name>_confidences.json`` paths, ``--gt_list`` ground truth PAGE-XMLs; they are paired by
``<name>``.  A value list is ``a,b,c`` or ``start:stop:step`` (stop included).  Outputs in ``--out_dir``:

- ``grid_comparison.csv``: one row per (page, setting) in ``SepPageCompDict.expCsv``'s format.  hypXML is the file
  ``run_conf_to_cluster`` would write for the setting, the method is ``path2method`` of it (the ``get_info`` string when the
  path is too short for that); with several ``--min_neighbors`` the info carries ``_nb<k>``, which ``get_info`` has not;
- ``grid_ranking.csv``: the settings by ``CompDictEvaler.countWinnerStat``'s ``all`` column, best first, computed with numpy;
- with ``--write_winner`` the winner's clustering PAGE-XMLs (``save_clustering_to_page``, below ``--out_dir``).
"""
import argparse
import csv
import logging
import os
import re
import sys

import numpy as np

from . import as_eval
from .path_util import get_page_from_conf_path, load_list_file

DATA_SET = "Koeln111_test"


def parse_values(text, cast=float):
    """'0.3,0.5' -> [0.3, 0.5]; '0.2:0.6:0.2' -> [0.2, 0.4, 0.6] (stop included, values rounded to 10 decimals)"""
    text = text.strip()
    if ":" in text:
        parts = text.split(":")
        if len(parts) != 3:
            raise argparse.ArgumentTypeError(f"'{text}' is not start:stop:step")
        start, stop, step = (float(p) for p in parts)
        if step <= 0 or stop < start:
            raise argparse.ArgumentTypeError(f"'{text}': step must be positive and stop >= start")
        count = int(np.floor((stop - start) / step + 1e-9)) + 1
        values = [round(start + i * step, 10) for i in range(count)]
    else:
        try:
            values = [float(v) for v in text.split(",") if v.strip() != ""]
        except ValueError:
            raise argparse.ArgumentTypeError(f"'{text}' is not a comma list of numbers")
    if cast is int and any(v != int(v) for v in values):
        raise argparse.ArgumentTypeError(f"'{text}' holds a value that is not an integer")
    return [cast(v) for v in values]


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--eval_list", type=str, required=True, help="list of confidence json files")
    p.add_argument("--gt_list", type=str, required=True, help="list of ground truth PAGE-XML files")
    p.add_argument("--confidence_thresholds", type=parse_values, default=parse_values("0:1:0.05"))
    p.add_argument("--cluster_agreement_thresholds", type=parse_values, default=parse_values("0:1:0.05"))
    p.add_argument("--min_neighbors", type=lambda s: parse_values(s, int), default=[1])
    p.add_argument("--out_dir", type=str, required=True)
    p.add_argument("--write_winner", action="store_true", help="write the winner's clustering PAGE-XMLs")
    p.add_argument("--gpu_device", type=int, default=0)
    return p


def grid_settings(conf_thrs, agree_thrs, min_nbs):
    """-> (clustering_params dicts, their info strings): min_neighbors outermost, then confidence, then agreement"""
    from .clustering import TextblockClustering

    class _F:
        clustering_params = {}
    settings, infos = [], []
    for nb in min_nbs:
        for c in conf_thrs:
            for a in agree_thrs:
                params = {"min_neighbors_for_cluster": int(nb), "confidence_threshold": c, "cluster_agreement_threshold": a}
                _F.clustering_params = params
                info = TextblockClustering(_F()).get_info("dbscan")
                settings.append(params)
                infos.append(info + (f"_nb{int(nb)}" if len(min_nbs) > 1 else ""))
    return settings, infos


def hyp_path(page_path, out_dir, info):
    """the file gnn_results.save_clustering_to_page writes for this page and info"""
    rel = os.path.relpath(page_path)
    name = re.sub(r'\.xml$', '_clustering.xml', os.path.basename(rel))
    return os.path.join(out_dir, re.sub(r'page$', 'clustering', os.path.dirname(rel)), info, name)


def method_of(path, info):
    try:
        return as_eval.SepPageCompDict.path2method(path)
    except IndexError:
        return info


def pair_lists(json_paths, gt_paths):
    """-> [(json, page, gt)] paired by <name> of <name>_confidences.json and <name>.xml"""
    by_name = {os.path.splitext(os.path.basename(p))[0]: p for p in gt_paths}
    out = []
    for j in json_paths:
        name = re.sub(r'_confidences\.json$', '', os.path.basename(j))
        if name not in by_name:
            raise ValueError(f"no ground truth PAGE-XML named {name}.xml in the gt list for {j}")
        out.append((j, get_page_from_conf_path(j), by_name[name]))
    return out


def rank(comps):
    """comps[setting][page] -> the 'all' score of every setting (int64 [settings])"""
    dist = np.array([[c.dist for c in row] for row in comps], np.int64).T
    corrects = np.array([[c.corrects for c in row] for row in comps], np.int64).T
    return as_eval.winner_all_counts(dist, corrects)


def run(json_paths, gt_paths, settings, infos, out_dir, device=0, write_winner=False):
    """-> (comparison csv path, ranking csv path, index of the winning setting, its 'all' score)"""
    from .clustering.cluster_grid import ClusterGrid
    from .run_conf_to_cluster import load_confidences
    triples = pair_lists(json_paths, gt_paths)
    grid = ClusterGrid(device)
    for j, page, _ in triples:
        grid.add_page(load_confidences(j, page)[1], symmetry_fn=None)
    comps, labels = grid.run_compare(settings, [(page, gt) for _, page, gt in triples])
    os.makedirs(out_dir, exist_ok=True)
    csv_path = os.path.join(out_dir, "grid_comparison.csv")
    with open(csv_path, "wt", encoding="utf8", newline="") as f:
        w = csv.DictWriter(f, fieldnames=as_eval.SepPageCompDict.fieldNames)
        w.writeheader()
        for k, (_, page, gt) in enumerate(triples):
            for s, info in enumerate(infos):
                hyp = hyp_path(page, out_dir, info)
                row = {"dataSet": DATA_SET, "method": method_of(hyp, info), "gtXML": str(gt), "hypXML": hyp}
                row.update(comps[s][k].dataDict())
                w.writerow(row)
    score = rank(comps) if triples else np.zeros(len(settings), np.int64)
    order = sorted(range(len(settings)), key=lambda s: -int(score[s]))      # stable: ties keep the grid's order
    rank_path = os.path.join(out_dir, "grid_ranking.csv")
    with open(rank_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["info", "min_neighbors_for_cluster", "confidence_threshold", "cluster_agreement_threshold", "all"])
        for s in order:
            p = settings[s]
            w.writerow([infos[s], p["min_neighbors_for_cluster"], repr(p["confidence_threshold"]),
                        repr(p["cluster_agreement_threshold"]), int(score[s])])
    winner = order[0] if order else None
    if write_winner and winner is not None:
        from .gnn_results import save_clustering_to_page
        for k, (_, page, _) in enumerate(triples):
            save_clustering_to_page([int(v) for v in labels[winner][k]], page, out_dir, info=infos[winner])
    logging.info(f"{len(settings)} settings on {len(triples)} pages in {grid.kernel_us:.0f} us of device time")
    return csv_path, rank_path, winner, (int(score[winner]) if winner is not None else 0)


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.getLogger().setLevel(logging.INFO)
    settings, infos = grid_settings(args.confidence_thresholds, args.cluster_agreement_thresholds, args.min_neighbors)
    json_paths = [p for p in load_list_file(args.eval_list) if p]
    gt_paths = [p for p in load_list_file(args.gt_list) if p]
    csv_path, rank_path, winner, score = run(json_paths, gt_paths, settings, infos, args.out_dir, args.gpu_device, args.write_winner)
    print(f"{len(settings)} settings on {len(json_paths)} pages -> {csv_path}, {rank_path}")
    if winner is not None:
        print(f"winner: {infos[winner]} (all = {score})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
