"""CLI mirror of ``article_separation_measure/run_measure.py``.

    python -m citlab_article_separation_new_amd.run_measure --path_to_gt_xml_lst gt.lst --path_to_hy_xml_lst hy.lst \\
        [--min_tol -1] [--max_tol -1] [--rel_tol 0.25] [--poly_tick_dist 5] [--verbose True] [--num_threads N]

Scores hypothesis PAGE-XML files against ground truth: the baseline detection measure over all baselines and over the
baselines with an article id, and the article / block segmentation measure; the per-file blocks and the AVERAGE VALUES
block are the reference's stdout line for line.  This process owns the GPU: the file pairs of a group share one device
call; ``--num_threads`` host threads (at most the container's CPU quota) read the files.  No JVM is started: the
results follow the reference's Python path.
"""
import os
import sys
from multiprocessing.pool import ThreadPool

from . import cli_flags
from .host_util import effective_cpus

GROUP = 16

MODES = ("baseline detection measure - all baselines", "baseline detection measure - without none",
         "article / block segmentation measure")


def build_parser():
    p = cli_flags.LineArgumentParser(fromfile_prefix_chars="@")
    p.add_argument("--path_to_gt_xml_lst", type=str, required=True,
                   help="path to the lst file containing the file paths of the ground truth Page XML's")
    p.add_argument("--path_to_hy_xml_lst", type=str, required=True,
                   help="path to the lst file containing the file paths of the hypotheses Page XML's")
    p.add_argument("--min_tol", type=int, default=-1,
                   help="MINIMUM distance tolerance which is not penalized, -1 for dynamic calculation")
    p.add_argument("--max_tol", type=int, default=-1,
                   help="MAXIMUM distance tolerance which is not penalized, -1 for dynamic calculation")
    p.add_argument("--rel_tol", type=float, default=0.25,
                   help="fraction of estimated interline distance as tolerance values")
    p.add_argument("--poly_tick_dist", type=int, default=5,
                   help="desired distance (measured in pixels) of two adjacent pixels in the normed polygons")
    p.add_argument("--verbose", nargs="?", const=True, default=True, type=cli_flags.str2bool,
                   help="print evaluation for every single file in addition to overall summary")
    p.add_argument("--num_threads", type=int, default=1, help="number of host threads reading the files")
    return p


def filter_and_sort(gt_xml_files, hy_xml_files):
    """run_measure.py:372-379: the HY list filtered by the GT base names (substring of the HY base name), both sorted
    by base name."""
    gt_base_names = [os.path.splitext(os.path.basename(f))[0] for f in gt_xml_files]
    hy = sorted([f for f in hy_xml_files if any(gt in os.path.basename(f) for gt in gt_base_names)], key=os.path.basename)
    return sorted(gt_xml_files, key=os.path.basename), hy


def format_row(mode, values, tail=()):
    """one table row: ``{:>10f}`` values, or dashes where the tuple is None; ``tail`` = (valid files, all files)"""
    if values is not None:
        row = "{:<50s} {:>10f} {:>10f} {:>10f}".format(mode, values[0], values[1], values[2])
    else:
        row = "{:<50s} {:>10s} {:>10s} {:>10s}".format(mode, "-", "-", "-")
    return row + (" {:>25d} {:>10d}".format(*tail) if tail else "")


def run_measure(gt_files, hy_files, min_tol, max_tol, rel_tol, poly_tick_dist, verbose=True, num_threads=1, log=print,
                device=0):
    """run_measure.py:247-352.  Returns the three (average tuple or None, counter) pairs it prints."""
    from . import measure
    if len(gt_files) != len(hy_files):
        log(f"Length of GT list ({len(gt_files)}) has to match length of HY list ({len(hy_files)})!")
        raise SystemExit(1)
    measure.check_tolerances(min_tol, max_tol, rel_tol, poly_tick_dist)
    sums, counters = [[0, 0, 0] for _ in MODES], [0, 0, 0]
    pairs = list(zip(gt_files, hy_files))
    with ThreadPool(max(1, min(num_threads, effective_cpus()))) as pool:
        for g0 in range(0, len(pairs), GROUP):
            group = pairs[g0:g0 + GROUP]
            is_xml = [gt.endswith(".xml") and hy.endswith(".xml") for gt, hy in group]
            names = [f for (gt, hy), ok in zip(group, is_xml) if ok for f in (gt, hy)]
            dicts = pool.map(measure.get_data_from_pagexml, names)
            scored = iter(measure.run_eval_dicts(list(zip(dicts[0::2], dicts[1::2])), min_tol, max_tol, rel_tol,
                                                 poly_tick_dist, device))
            for (gt_file, hy_file), ok in zip(group, is_xml):
                if verbose:
                    log("-" * 125)
                    log("Ground truth file: ", gt_file)
                    log("Hypotheses file  : ", hy_file, "\n")
                if ok:
                    tuples = measure.evaluate(*next(scored), log=log)
                else:
                    log("!! Ground truth and hypotheses file have to be in Page XML format !!\n")
                    tuples = (None, None, None)
                if verbose:
                    log("{:<50s} {:>10s} {:>10s} {:>10s}".format("Mode", "R-value", "P-value", "F-value"))
                for m, tup in enumerate(tuples):
                    if verbose:
                        log(format_row(MODES[m], tup))
                    if tup is not None:
                        sums[m] = [sums[m][i] + tup[i] for i in range(3)]
                        counters[m] += 1
    log("-" * 125)
    log("-" * 125)
    log("AVERAGE VALUES")
    log("{:<50s} {:>10s} {:>10s} {:>10s} {:>25s} {:>10s}".format("Mode", "R-value", "P-value", "F-value",
                                                                 "valid evaluated files", "all files"))
    out = []
    for m, mode in enumerate(MODES):
        avg = tuple(1 / counters[m] * v for v in sums[m]) if counters[m] > 0 else None
        log(format_row(mode, avg, (counters[m], len(gt_files))))
        out.append((avg, counters[m]))
    return out


def main(argv=None):
    flags = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    gt_xml_files = [line.rstrip("\n") for line in open(flags.path_to_gt_xml_lst, "r")]
    hy_xml_files = [line.rstrip("\n") for line in open(flags.path_to_hy_xml_lst, "r")]
    gt_xml_files, hy_xml_files = filter_and_sort(gt_xml_files, hy_xml_files)
    run_measure(gt_xml_files, hy_xml_files, flags.min_tol, flags.max_tol, flags.rel_tol, flags.poly_tick_dist,
                flags.verbose, flags.num_threads)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
