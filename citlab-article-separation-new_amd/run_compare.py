"""CLI mirror of ``as_eval/run_compare.py``: ground truth PAGE-XMLs against every ``clustering/<info>/`` folder below a work dir.

    python -m citlab_article_separation_new_amd.run_compare --gt_list gt.lst --work_dir out --out_dir eval --name run1

Same arguments.  Writes ``<name>_comparison.csv`` (``SepPageCompDict.expCsv``), ``<name>_comparison.sqlite`` (``expSqlite``,
table allComps) and the winner table as ``<name>_winner.csv`` (the reference writes an XLSX workbook; that export is left
out).  This is the one-pair host path (``as_eval.SepPageBlComper``); ``run_cluster_grid_search`` compares a whole grid on
the device.
"""
import argparse
import csv
import glob
import logging
import os
import sys

from . import as_eval

DATA_SET = "Koeln111_test"      # the label the reference files every comparison under


def find_dirs(name, root='.', exclude=None):
    results = [os.path.join(path, name) for path, dirs, _ in os.walk(root) if name in dirs]
    for ex in (exclude.split(",") if exclude else []):
        results = [res for res in results if ex not in res]
    return results


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--gt_list", type=str, help="list file containing GT file paths", default=None)
    parser.add_argument("--gt_dir", type=str, help="dir path containing GT files", default=None)
    parser.add_argument("--exclude", type=str, help="comma separated strings to exclude from gt_dir", default=None)
    parser.add_argument("--work_dir", type=str, help="dir path containing clustering folders", required=True)
    parser.add_argument("--out_dir", type=str, help="dir path for the ouput files", required=True)
    parser.add_argument("--name", type=str, help="optional name for output comparison file", default=None)
    return parser


def compare(gt_files, clustering_paths, exclude=None):
    """every ground truth file against <clustering path>/<method folder>/<stem>_clustering.xml -> SepPageCompDict"""
    comper = as_eval.SepPageBlComper()
    results = as_eval.SepPageCompDict()
    for gt_file in gt_files:
        logging.info(f'comparing GT from {gt_file} ...')
        comper.loadGT(gt_file)
        for clustering_path in clustering_paths:
            folders = [os.path.join(clustering_path, f) for f in os.listdir(clustering_path)]
            for ex in (exclude.split(",") if exclude else []):
                folders = [f for f in folders if ex not in f]
            for folder in folders:
                if not os.path.isdir(folder):
                    continue
                hyp_file = os.path.join(folder, os.path.splitext(os.path.basename(gt_file))[0] + "_clustering.xml")
                res = comper.compareTo(hyp_file)
                logging.info(f'\t... with HYP in {hyp_file}:\t{res.__dict__}')
                results.addItem(dataSet=DATA_SET, gtXML=str(gt_file), hypXML=str(hyp_file), spcDict=res)
    return results


def write_outputs(results, out_dir, name=None):
    """-> (comparison csv, winner csv, sqlite) paths and the evaluator"""
    os.makedirs(out_dir, exist_ok=True)
    stem = f"{name}_" if name else ""
    csv_path = os.path.join(out_dir, f"{stem}comparison.csv")
    db_path = os.path.join(out_dir, f"{stem}comparison.sqlite")
    winner_path = os.path.join(out_dir, f"{stem}winner.csv")
    results.expCsv(as_eval.Path(csv_path))
    results.expSqlite(db_path, "allComps")
    evaler = as_eval.CompDictEvaler(results)
    evaler.calcWinnerDict()
    with open(winner_path, "w", newline="") as f:
        csv.writer(f).writerows(evaler.winner_csv_rows())
    return csv_path, winner_path, db_path, evaler


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.getLogger().setLevel(logging.INFO)
    if args.gt_dir and args.gt_list:
        logging.error("Only one GT variant can be chosen at a time!")
        return 1
    if args.gt_dir:
        gt_path = find_dirs("page", root=args.gt_dir)[0]
        gt_files = [os.path.join(gt_path, os.path.basename(p)) for p in glob.glob(os.path.join(glob.escape(gt_path), '*.xml'))]
    elif args.gt_list:
        with open(args.gt_list) as f:
            gt_files = [line.rstrip() for line in f if line.rstrip()]
    else:
        logging.error("Either --gt_list or --gt_dir is needed!")
        return 1
    clustering_paths = find_dirs("clustering", root=args.work_dir, exclude=args.exclude)
    logging.info("Using clustering paths:")
    for path in clustering_paths:
        logging.info(f"\t{path}")
    results = compare(gt_files, clustering_paths, args.exclude)
    csv_path, winner_path, db_path, _ = write_outputs(results, args.out_dir, args.name)
    logging.info(f"writing to {csv_path}, {winner_path}, {db_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
