"""Grid search over the ``dbscan`` clustering settings and, with ``--methods``, over ``dbscan_std`` and ``greedy`` settings next
to them: every (page, setting) clustered and compared with the ground truth in one device call (``ClusterGrid.run_compare``).
No counterpart in the reference, which runs ``run_conf_to_cluster`` once per setting and ``run_compare`` over the folders.

    python -m citlab_article_separation_new_amd.run_cluster_grid_search --eval_list confidences.lst --gt_list gt.lst \\
        --confidence_thresholds 0:1:0.05 --cluster_agreement_thresholds 0:1:0.05 --min_neighbors 1 --out_dir eval

``--eval_list`` holds ``confidences/<name>_confidences.json`` paths, ``--gt_list`` ground truth PAGE-XMLs; they are paired by
``<name>``.  A value list is ``a,b,c`` or ``start:stop:step`` (stop included).  ``--methods dbscan,dbscan_std,greedy`` adds the
``--epsilons`` x ``--min_samples`` grid of ``dbscan_std`` and one ``greedy`` setting per ``--max_iterations`` value behind the
dbscan grid (``linkage`` runs on the host only: ``run_conf_to_cluster``).  Outputs in ``--out_dir``:

- ``grid_comparison.csv``: one row per (page, setting) in ``SepPageCompDict.expCsv``'s format.  hypXML is the file
  ``run_conf_to_cluster`` would write for the setting, the method is ``path2method`` of it (the ``get_info`` string when the
  path is too short for that); with several ``--min_neighbors`` the info carries ``_nb<k>``, which ``get_info`` has not;
- ``grid_ranking.csv``: the settings by ``CompDictEvaler.countWinnerStat``'s ``all`` column, best first, computed with numpy;
  with ``--methods`` it ends in the columns ``clustering_method``, ``epsilon``, ``min_samples``, ``max_iteration`` (a column that
  is not a parameter of the row's method stays empty);
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
METHODS = ("dbscan", "dbscan_std", "greedy")


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


def parse_methods(text):
    methods = [m.strip() for m in text.split(",") if m.strip()]
    for m in methods:
        if m == "linkage":
            raise argparse.ArgumentTypeError("'linkage' runs on the host only (run_conf_to_cluster --clustering_method linkage)")
        if m not in METHODS:
            raise argparse.ArgumentTypeError(f"'{m}' is not one of {', '.join(METHODS)}")
    if not methods or len(set(methods)) != len(methods):
        raise argparse.ArgumentTypeError(f"'{text}' names no method or one twice")
    return methods


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--eval_list", type=str, required=True, help="list of confidence json files")
    p.add_argument("--gt_list", type=str, required=True, help="list of ground truth PAGE-XML files")
    p.add_argument("--confidence_thresholds", type=parse_values, default=parse_values("0:1:0.05"))
    p.add_argument("--cluster_agreement_thresholds", type=parse_values, default=parse_values("0:1:0.05"))
    p.add_argument("--min_neighbors", type=lambda s: parse_values(s, int), default=[1])
    p.add_argument("--methods", type=parse_methods, default=None, help="comma list of dbscan, dbscan_std, greedy (default: dbscan)")
    p.add_argument("--epsilons", type=parse_values, default=[0.5], help="dbscan_std: epsilon values")
    p.add_argument("--min_samples", type=lambda s: parse_values(s, int), default=[1], help="dbscan_std: min_samples values")
    p.add_argument("--max_iterations", type=lambda s: parse_values(s, int), default=[1000], help="greedy: max_iteration values")
    p.add_argument("--out_dir", type=str, required=True)
    p.add_argument("--write_winner", action="store_true", help="write the winner's clustering PAGE-XMLs")
    p.add_argument("--gpu_device", type=int, default=0)
    return p


def grid_settings(conf_thrs, agree_thrs, min_nbs, methods=("dbscan",), epsilons=(0.5,), min_samples=(1,), max_iterations=(1000,)):
    """-> (clustering_params dicts, their info strings).  The dbscan grid first: min_neighbors outermost, then confidence, then
    agreement; behind it the other ``methods`` in the order given: dbscan_std with epsilon outermost, then min_samples, and
    greedy per max_iteration.  Their dicts carry "clustering_method"; the infos are ``TextblockClustering.get_info``'s."""
    from .clustering import TextblockClustering

    class _F:
        clustering_params = {}

    def info_of(method, params):
        _F.clustering_params = params
        return TextblockClustering(_F()).get_info(method)
    settings, infos = [], []
    if "dbscan" in methods:
        for nb in min_nbs:
            for c in conf_thrs:
                for a in agree_thrs:
                    params = {"min_neighbors_for_cluster": int(nb), "confidence_threshold": c, "cluster_agreement_threshold": a}
                    settings.append(params)
                    infos.append(info_of("dbscan", params) + (f"_nb{int(nb)}" if len(min_nbs) > 1 else ""))
    for method in methods:
        if method == "dbscan_std":
            grid = [{"epsilon": e, "min_samples": int(k)} for e in epsilons for k in min_samples]
        elif method == "greedy":
            grid = [{"max_iteration": int(it)} for it in max_iterations]
        else:
            continue
        for params in grid:
            settings.append(dict(params, clustering_method=method))
            infos.append(info_of(method, params))
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


METHOD_COLUMNS = ["clustering_method", "epsilon", "min_samples", "max_iteration"]


def ranking_row(info, p, score, method_columns=False):
    def value(key):
        return repr(p[key]) if isinstance(p.get(key), float) else p.get(key, "")
    row = [info, value("min_neighbors_for_cluster"), value("confidence_threshold"), value("cluster_agreement_threshold"), int(score)]
    if method_columns:
        row += [p.get("clustering_method", "dbscan")] + [value(k) for k in METHOD_COLUMNS[1:]]
    return row


def run(json_paths, gt_paths, settings, infos, out_dir, device=0, write_winner=False, method_columns=False):
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
        w.writerow(["info", "min_neighbors_for_cluster", "confidence_threshold", "cluster_agreement_threshold", "all"]
                   + (METHOD_COLUMNS if method_columns else []))
        for s in order:
            w.writerow(ranking_row(infos[s], settings[s], score[s], method_columns))
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
    settings, infos = grid_settings(args.confidence_thresholds, args.cluster_agreement_thresholds, args.min_neighbors,
                                    args.methods or ("dbscan",), args.epsilons, args.min_samples, args.max_iterations)
    json_paths = [p for p in load_list_file(args.eval_list) if p]
    gt_paths = [p for p in load_list_file(args.gt_list) if p]
    csv_path, rank_path, winner, score = run(json_paths, gt_paths, settings, infos, args.out_dir, args.gpu_device, args.write_winner,
                                             method_columns=args.methods is not None)
    print(f"{len(settings)} settings on {len(json_paths)} pages -> {csv_path}, {rank_path}")
    if winner is not None:
        print(f"winner: {infos[winner]} (all = {score})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
