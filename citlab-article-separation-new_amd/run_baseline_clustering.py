"""CLI mirror of ``article_separation/run_baseline_clustering.py`` (+ ``baseline_clustering/baseline_clustering.py``).

    python -m citlab_article_separation_new_amd.run_baseline_clustering --path_to_xml_lst pages.lst \\
        [--min_polygons_for_cluster 2] [--min_polygons_for_article 1] [--rectangle_interline_factor 1.25] \\
        [--des_dist 5] [--max_d 500] [--target_average_interline_distance 50] [--num_threads N]

DBSCAN over the baselines of each PAGE-XML file; the article ids ("a<label>", none for noise) are written onto the text
lines and the file is rewritten in place.  This process owns the GPU: the pages of a group go through each kernel in
one launch; ``--num_threads`` host threads (at most the container's CPU quota) read and write the files.
``--use_java_code`` is accepted with either value: the results always follow the reference's Python path.
"""
import sys
from multiprocessing.pool import ThreadPool

from . import cli_flags
from .host_util import effective_cpus
from .page_xml import Page

GROUP = 32


def build_parser():
    p = cli_flags.LineArgumentParser(fromfile_prefix_chars="@")
    p.add_argument("--path_to_xml_lst", type=str, default="",
                   help="path to the lst file containing the file paths of the page xml's to be processed")
    p.add_argument("--path_to_xml_file", type=str, default="", help="a single page xml file (instead of a list)")
    p.add_argument("--min_polygons_for_cluster", type=int, default=2,
                   help="minimum number of required polygons in neighborhood to form a cluster")
    p.add_argument("--min_polygons_for_article", type=int, default=1,
                   help="minimum number of required polygons forming an article")
    p.add_argument("--rectangle_interline_factor", type=float, default=1.25,
                   help="multiplication factor to calculate the height of the rectangles during the clustering "
                        "progress with the help of the interline distances")
    p.add_argument("--des_dist", type=int, default=5,
                   help="desired distance (measured in pixels) of two adjacent pixels in the normed polygons")
    p.add_argument("--max_d", type=int, default=500,
                   help="maximum distance (measured in pixels) for the calculation of the interline distances")
    p.add_argument("--use_java_code", nargs="?", const=True, default=True, type=cli_flags.str2bool,
                   help="accepted for compatibility with either value; the interline distances are always those of the "
                        "reference's Python path (computed on the GPU), the Java class is not used")
    p.add_argument("--target_average_interline_distance", "--target_avg_interline_distance", type=int, default=50,
                   dest="target_average_interline_distance", help="target interline distance for scaling of the polygons")
    p.add_argument("--num_threads", type=int, default=1, help="number of host threads reading / writing the files")
    return p


def read_baselines(path):
    """baseline_clustering.py:12-37: the page's text lines with a baseline of at least two points, and their polygons."""
    page = Page(path)
    lines, polys = [], []
    for tl in page.get_textlines():
        if len(tl.baseline) > 1:
            lines.append(tl)
            polys.append(([p[0] for p in tl.baseline], [p[1] for p in tl.baseline]))
    return page, lines, polys


def write_labels(path, page, lines, labels):
    """baseline_clustering.py:40-56: article id "a<label>", -1 removes the id; the file is rewritten in place."""
    for tl, lab in zip(lines, labels):
        tl.set_article_id(None if lab == -1 else "a" + str(lab))
    page.set_textline_attr(lines)
    page.write_page_xml(path)


def _safely(fn, *args):
    """fn(*args), or the exception it raised: one bad file fails alone, as in the reference's per-file subprocesses"""
    try:
        return fn(*args)
    except Exception as e:      # noqa: BLE001 (reported as the file's error line)
        return e


def process(paths, flags, device=0, log=print, start=1):
    """All pages of ``paths`` in groups of GROUP; returns the list of error lines (the reference's "saving errors").
    A file that cannot be read, normed, clustered or written is reported there and left as it was."""
    from . import textblock
    n_threads = max(1, min(flags.num_threads, effective_cpus()))
    errors = []
    with ThreadPool(n_threads) as pool:
        for g0 in range(0, len(paths), GROUP):
            group = paths[g0:g0 + GROUP]
            read = pool.starmap(_safely, [(read_baselines, p) for p in group])
            good = [r for r in read if not isinstance(r, Exception)]
            clustered = iter(textblock.cluster_baselines(
                [r[2] for r in good], flags.min_polygons_for_cluster, flags.min_polygons_for_article,
                flags.rectangle_interline_factor, flags.des_dist, flags.max_d, flags.target_average_interline_distance,
                device))
            jobs = []
            for k, (path, rd) in enumerate(zip(group, read)):
                log("No {:5d}: {}".format(start + g0 + k, path))
                if isinstance(rd, Exception):
                    msg = "{}: not read ({}: {})".format(path, type(rd).__name__, rd)
                    log(msg + "\n")
                    errors.append(msg)
                    continue
                page, lines, polys = rd
                res = next(clustered)
                log("Number of (detected) baselines contained by the image: {}".format(len(polys)))
                if isinstance(res, Exception):
                    msg = "{}: not clustered ({}: {})".format(path, type(res).__name__, res)
                    log(msg + "\n")
                    errors.append(msg)
                    continue
                labels, n_articles = res
                log("Number of detected articles (inclusive the \"noise\" class): {}\n".format(n_articles))
                jobs.append((path, page, lines, labels))
            for (path, *_), w in zip(jobs, pool.starmap(_safely, [(write_labels, *j) for j in jobs])):
                if isinstance(w, Exception):
                    msg = "{}: not written ({}: {})".format(path, type(w).__name__, w)
                    log(msg)
                    errors.append(msg)
    return errors


def main(argv=None):
    flags = build_parser().parse_known_args(sys.argv[1:] if argv is None else argv)[0]
    if flags.path_to_xml_file:
        paths = [flags.path_to_xml_file]
    elif flags.path_to_xml_lst:
        paths = [line.rstrip("\n") for line in open(flags.path_to_xml_lst) if line.strip()]
    else:
        build_parser().error("--path_to_xml_lst (or --path_to_xml_file) is required")
    print("####################\ntotal number of xml files:")
    print(len(paths))
    print("####################\n")
    errors = process(paths, flags)
    print("####################\nsaving errors:")
    for e in errors:
        print(e)
    print("####################\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
