"""CLI mirror of ``article_separation/run_textregion_generation.py`` (+ ``textregion_generation/textregion_generation.py``).

    python -m citlab_article_separation_new_amd.run_textregion_generation --path_to_xml_lst pages.lst \\
        [--des_dist 50] [--max_d 100] [--alpha 75] [--num_threads N] [--device_regions True [--device_triangulation True]]

One alpha-shape TextRegion per article of each PAGE-XML file (one per line for lines without an article id), with
reading orders for the regions and their lines; the existing text regions are replaced and the file is rewritten in
place.  As in the reference the region outlines use the normed baselines of ``--des_dist`` while the interline
distances use the default des_dist of 5.  This process owns the GPU (one distance launch per group of pages);
``--num_threads`` host threads (at most the container's CPU quota) read the files and build the regions.
``--use_java_code`` is accepted with either value: the results always follow the reference's Python path.
``--device_regions True`` (off by default): the host triangulates each article of a group of pages once and one engine
call gives the alpha shapes of the whole group (textblock.create_text_regions_pages); files and printed lines are the same.
``--device_triangulation True`` (off by default, needs ``--device_regions True``): that call triangulates the articles too, the
host no longer calls scipy.  The printed lines are the same; every region is the same polygon as without the flag (the same
cyclic vertex sequence after the same alpha retries) but NOT the same bytes: it is written from its vertex with the smallest
(y, x) in the direction of positive shoelace area (textblock.canonical_ring), where the default path starts at an edge that
Qhull's internal order picks.  Articles with a bounding box over 16383 px, more than 4096 points, fewer than 3 distinct points
or all points on one line go through the host function.
"""
import io
import sys
from multiprocessing.pool import ThreadPool

from . import cli_flags
from .host_util import effective_cpus
from .page_xml import Page

GROUP = 32
INTERLINE_DES_DIST = 5          # textregion_generation.py:48: get_list_of_interline_distances with its default des_dist


def build_parser():
    p = cli_flags.LineArgumentParser(fromfile_prefix_chars="@")
    p.add_argument("--path_to_xml_lst", type=str, default="",
                   help="path to the lst file containing the file paths of the page xml's to be processed")
    p.add_argument("--path_to_xml_file", type=str, default="", help="a single page xml file (instead of a list)")
    p.add_argument("--des_dist", type=int, default=50,
                   help="desired distance (measured in pixels) of two adjacent pixels in the normed polygons")
    p.add_argument("--max_d", type=int, default=100,
                   help="maximum distance (measured in pixels) for the calculation of the interline distances")
    p.add_argument("--alpha", type=float, default=75,
                   help="alpha value for the alpha shape algorithm "
                        "(for alpha -> infinity we get the convex hulls, recommended: alpha >= des_dist)")
    p.add_argument("--use_java_code", nargs="?", const=True, default=False, type=cli_flags.str2bool,
                   help="accepted for compatibility with either value; the interline distances are always those of the "
                        "reference's Python path (computed on the GPU), the Java class is not used")
    p.add_argument("--num_threads", type=int, default=1, help="number of host threads reading / writing the files")
    p.add_argument("--device_regions", type=cli_flags.str2bool, default=False,
                   help="alpha shapes of all articles of a group of pages in one GPU call behind the host triangulation; "
                        "same files and printed lines")
    p.add_argument("--device_triangulation", type=cli_flags.str2bool, default=False,
                   help="with --device_regions True: the GPU call triangulates the articles too (no scipy).  Same printed lines "
                        "and the same polygons (same cyclic vertex sequence, same alpha retries), written from the vertex with "
                        "the smallest (y, x) in the direction of positive shoelace area: not the same bytes as the default path.  "
                        "Articles with a box over 16383 px or more than 4096 points and degenerate ones take the host function")
    return p


def parse_flags(argv):
    """the known flags of ``argv``; --device_triangulation without --device_regions is a usage error"""
    parser = build_parser()
    flags = parser.parse_known_args(argv)[0]
    if flags.device_triangulation and not flags.device_regions:
        parser.error("--device_triangulation True needs --device_regions True")
    return flags


def read_page(path, des_dist):
    """textregion_generation.py:17-77 up to the distances: the article dict, the lines with a baseline of at least two
    points, their polygons and their normed polygons at ``des_dist`` (the region outlines)."""
    from . import textblock_geometry as geo
    page = Page(path)
    all_lines = page.get_textlines()
    art = page.get_article_dict(all_lines)
    lines, polys = [], []
    for tl in all_lines:
        if len(tl.baseline) > 1:
            lines.append(tl)
            polys.append(([p[0] for p in tl.baseline], [p[1] for p in tl.baseline]))
    return page, art, lines, polys, geo.norm_poly_dists(polys, des_dist)


def page_geometry(art, lines, normed, dists):
    """textregion_generation.py:50-77: synthetic Coords for the lines without, and what create_text_regions reads:
    ({line id: line}, {article id: [line id, ...]}, {line id: (normed polygon, interline distance)})"""
    from . import textblock
    by_id = {tl.id: tl for ls in art.values() for tl in ls}
    geom = {}
    for tl, poly, d in zip(lines, normed, dists):
        if not tl.has_coords():
            tl.set_coords(textblock.synthetic_coords(poly[0], poly[1], d))
        geom[tl.id] = (poly, float(d))
    return by_id, {a: [tl.id for tl in ls] for a, ls in art.items()}, geom


def write_regions(path, page, by_id, regions):
    """textregion_generation.py:102-127: reading orders, the regions in place of the page's, write back"""
    from . import textblock
    objs = []
    for rid, points, members, ro in regions:
        tls = [by_id[i] for i in members]
        for tl, r in zip(tls, textblock.reading_order([([p[0] for p in tl.baseline], [p[1] for p in tl.baseline])
                                                       for tl in tls])):
            tl.set_reading_order(r)
        objs.append((rid, points, tls, ro))
    page.replace_text_regions(objs)
    page.write_page_xml(path)


def finish_page(path, page, art, lines, normed, dists, alpha):
    """textregion_generation.py:50-77 and 102-172: synthetic Coords, alpha-shape regions, reading orders, write back.
    Returns the lines the reference prints (its alpha retries)."""
    from . import textblock
    out = io.StringIO()
    by_id, art_ids, geom = page_geometry(art, lines, normed, dists)
    regions = textblock.create_text_regions(art_ids, geom, alpha, log=lambda s: print(s, file=out))
    write_regions(path, page, by_id, regions)
    return out.getvalue()


def _safely(fn, *args):
    """fn(*args), or the exception it raised: one bad file fails alone, as in the reference's per-file subprocesses"""
    try:
        return fn(*args)
    except Exception as e:      # noqa: BLE001 (reported as the file's error line)
        return e


def process(paths, flags, device=0, log=print, start=1):
    """All pages of ``paths`` in groups of GROUP; returns the list of error lines (the reference's "saving errors").
    A file that cannot be read, normed or given its regions is reported there and left as it was."""
    from . import textblock
    n_threads = max(1, min(flags.num_threads, effective_cpus()))
    errors = []
    with ThreadPool(n_threads) as pool:
        for g0 in range(0, len(paths), GROUP):
            group = paths[g0:g0 + GROUP]
            read = pool.starmap(_safely, [(read_page, p, flags.des_dist) for p in group])
            normed5 = [r if isinstance(r, Exception) else textblock.normed_pages_or_errors([r[3]], INTERLINE_DES_DIST)[0]
                       for r in read]
            dists = textblock.interline_distances_or_errors(normed5, INTERLINE_DES_DIST, flags.max_d, device)

            def failed(k, e):
                return "", "{}: not written ({}: {})".format(group[k], type(e).__name__, e)

            def finish(k):
                if isinstance(dists[k], Exception):      # not read, or its baselines could not be normed
                    return failed(k, dists[k])
                page, art, lines, polys, normed = read[k]
                try:
                    return finish_page(group[k], page, art, lines, normed, dists[k], flags.alpha), None
                except Exception as e:        # the reference's per-file subprocess fails without saving
                    return failed(k, e)

            step = finish
            if getattr(flags, "device_regions", False):
                # the same steps with the alpha shapes of the whole group from one engine call in between
                good = [k for k in range(len(group)) if not isinstance(dists[k], Exception)]
                geoms = pool.map(lambda k: _safely(page_geometry, read[k][1], read[k][2], read[k][4], dists[k]), good)
                ready = [(k, g) for k, g in zip(good, geoms) if not isinstance(g, Exception)]
                outs = [io.StringIO() for _ in ready]
                regions = textblock.create_text_regions_pages(
                    [(g[1], g[2]) for _, g in ready], flags.alpha,
                    [lambda s, o=o: print(s, file=o) for o in outs], device, pool,
                    device_triangulation=getattr(flags, "device_triangulation", False))
                staged = {k: g for k, g in zip(good, geoms) if isinstance(g, Exception)}
                staged.update({k: (g[0], r, o) for (k, g), r, o in zip(ready, regions, outs)})

                def step(k):            # finish(k) with the regions already there
                    if isinstance(dists[k], Exception):
                        return failed(k, dists[k])
                    if isinstance(staged[k], Exception):
                        return failed(k, staged[k])
                    by_id, regs, out = staged[k]
                    if isinstance(regs, Exception):
                        return failed(k, regs)
                    try:
                        write_regions(group[k], read[k][0], by_id, regs)
                        return out.getvalue(), None
                    except Exception as e:
                        return failed(k, e)
            for k, (printed, err) in enumerate(pool.map(step, range(len(group)))):
                log("No {:5d}: {}".format(start + g0 + k, group[k]))
                if printed:
                    log(printed.rstrip("\n"))
                if err:
                    log(err)
                    errors.append(err)
    return errors


def main(argv=None):
    flags = parse_flags(sys.argv[1:] if argv is None else argv)
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
