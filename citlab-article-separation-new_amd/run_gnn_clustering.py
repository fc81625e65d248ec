"""CLI mirror of ``article_separation/gnn/run_gnn_clustering.py`` on the MI355X engine.

    python -m citlab_article_separation_new_amd.run_gnn_clustering --model_dir net.pb --eval_list jsons.lst \\
        --input_params node_feature_dim=15 edge_feature_dim=2 node_input_feature_mask=[1,1,1,1,0,0,0,0,0,0,0,0,1,1,1] \\
        --clustering_method dbscan --out_dir out

Same flags (``run_gnn_clustering.py:19-73``), same per-page loop (``:237-300``): json -> feed dict -> engine ->
confidences [N,N] -> (optional json) -> TextblockClustering -> ``<out_dir>/.../clustering/<info>/<name>_clustering.xml``.
``--num_workers`` > 1: that many host worker processes prepare feeds ahead of / cluster and write behind one GPU-owning process
per entry of ``--gpu_devices`` (the reference forks one session-owning ``mp.Process`` per sub-list, ``:322-340``).  Worker errors
are surfaced (the reference drops them).
"""
import logging
import multiprocessing as mp
import queue
import os
import sys
import time

import numpy as np

from . import cli_flags
from .host_util import split_list
from .path_util import get_page_from_json_path, get_path_from_exportdir, load_list_file


def build_parser():
    p = cli_flags.LineArgumentParser(fromfile_prefix_chars="@")
    p.add_argument("--model_dir", type=str, default="")
    p.add_argument("--eval_list", type=str, default="")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--num_relation_components", type=int, default=2)
    p.add_argument("--sample_num_relations_to_consider", type=int, default=100)
    p.add_argument("--sample_relations", type=cli_flags.str2bool, default=False)
    p.add_argument("--image_input", type=cli_flags.str2bool, default=False)
    # extension: the backbone end points a graph exported with --image_input reads its visual node features from
    # (the reference fixed them at training time with --feature_map_generation_params from_layer=[...])
    # and, for a layout with generated maps (feature_map_generators.py:72-197), their depths: --visual_layer_depths -1 32 32 with '' in
    # --visual_layers for "from the previous map", or the reference's own spelling
    # --feature_map_generation_params from_layer=[scale_0_unet_up_1_conv,,] layer_depth=[-1,32,32]
    cli_flags.define_feature_map_layout(p)
    # extension: True = the scan goes to the device as decoded (uint8) and is resized there (asep_prep_resize_tf1_dev: the host resize bit
    # for bit; a colour file under load_mode=L is decoded as RGB and the kernel takes Pillow's luma).  The default stays the host resize
    # until the device path is no slower on every leg: with host workers it loses on colour scans
    p.add_argument("--device_resize", type=cli_flags.str2bool, default=False)
    # extension: up to N prepared pages, of whatever image sizes, go through the engine in ONE call (gnn_io.run_pages ->
    # asep_gnn_forward_visual_batch_dev2; a graph without the visual branch: GnnSession.run_confidences -> asep_gnn_forward_batch);
    # 1 = page by page.  The files written are the same bytes for every N
    p.add_argument("--pages_per_call", type=cli_flags.pages_per_call, default=1)
    p.add_argument("--assign_visual_features_to_nodes", type=cli_flags.str2bool, default=True)
    p.add_argument("--assign_visual_features_to_edges", type=cli_flags.str2bool, default=False)
    p.add_argument("--mvn", type=cli_flags.str2bool, default=True)
    cli_flags.define_dict(p, "input_params", {})
    p.add_argument("--clustering_method", type=str, default="dbscan", choices=["dbscan", "linkage", "greedy", "dbscan_std"])
    p.add_argument("--mask_horizontally_separated_confs", type=cli_flags.str2bool, default=False)
    p.add_argument("--mask_heading_separated_confs", type=cli_flags.str2bool, default=False)
    # extension: True = the pair rules of the two masks run on the device (edge_features.py); the masked confidences are the same
    p.add_argument("--device_edges", type=cli_flags.str2bool, default=False)
    cli_flags.define_dict(p, "clustering_params", {})
    p.add_argument("--out_dir", type=str, default="")
    p.add_argument("--save_conf", type=str, default="no_conf", choices=["no_conf", "with_conf", "only_conf"])
    p.add_argument("--num_workers", type=int, default=1)
    p.add_argument("--gpu_devices", type=int, nargs="*", default=[])
    p.add_argument("--gpu_memory_fraction", type=float, default=0.95)
    p.add_argument("--batch_limiter", type=int, default=-1)
    p.add_argument("--try_gpu", type=cli_flags.str2bool, default=None)
    return p


def resolve_model_path(flags):
    """run_gnn_clustering.py:191-204 (also accepts the engine's .asepw container)."""
    if os.path.isfile(flags.model_dir):
        ext = os.path.splitext(os.path.basename(flags.model_dir))[1]
        if ext not in (".pb", ".asepw"):
            raise IOError(f"Given model path {flags.model_dir} is not a .pb")
        return flags.model_dir
    pb = None
    try_gpu = flags.try_gpu if flags.try_gpu is not None else bool(flags.gpu_devices)
    if try_gpu:
        try:
            pb = get_path_from_exportdir(flags.model_dir, "*_gpu.pb", "cpu")
        except IOError:
            logging.warning("Could not find gpu-model-pb-file, continue with cpu-model-pb-file")
    return pb or get_path_from_exportdir(flags.model_dir, "*best*.pb", "_gpu.pb")


def _prepare_page(input_fn, flags, json_path, image_later=False):
    """:237-262 for one page: json (+ scan for a graph exported with image_input) -> (PAGE-XML path, feed dict, number of nodes), or
    None if the json does not exist.  ``image_later``: the json half only, the caller adds the scan (a decode slot)"""
    page_path = get_page_from_json_path(json_path)
    if not os.path.isfile(json_path):
        logging.warning(f"No json file found to given pageXML {page_path}. Skipping.")
        return None
    feed, n = _prepare_feed(input_fn, flags, json_path, image_later=image_later)
    return page_path, feed, n


def _device_resize(flags):
    return bool(getattr(flags, "device_resize", False))


def _prepare_feed(input_fn, flags, json_path, targets=None, image_later=False, device_resize=None):
    """the feed dict of one graph json (+ its scan for a graph exported with image_input) and its number of nodes; ``targets``
    (a dict) receives the json's ground truth relations (lav_rel); ``device_resize`` None: as ``flags`` say"""
    image = None
    device_resize = _device_resize(flags) if device_resize is None else bool(device_resize)
    if flags.image_input and not image_later:
        from .gnn_input import load_page
        from .path_util import get_img_from_json_path
        # input_dataset.py:279-280: the scan as mode "L", or [H,W,3] in R, G, B order for load_mode=RGB; with --device_resize a colour
        # file under load_mode=L stays RGB (the resize kernel takes Pillow's luma)
        image = load_page(get_img_from_json_path(json_path), input_fn.input_params["load_mode"], device_resize)
    feed = input_fn.feed_from_json(json_path, image, targets, device_resize=device_resize,
                                   image_later=image_later and flags.image_input)
    n = feed["node_features:0"].shape[1] if "node_features:0" in feed else int(feed["num_nodes:0"][0])
    return feed, n


def _finish_page(tb, flags, output, n, page_path, device=None):
    """:269-300 for one page: net output -> confidences [N,N] -> (masks, json) -> clustering -> PAGE-XML with article ids;
    -> path of the written file, or None with --save_conf only_conf.  ``device``: the GPU of the calling owner process, where
    --device_edges computes the masks' pair rules; None (a host worker, which owns no GPU) keeps them on the host"""
    from . import gnn_results
    # (a page of a batched graph call arrives as its confidence matrix [N, N]: the class-1 column is all that call returns)
    confidences = output if np.ndim(output) == 2 else gnn_results.confidences_from_output(output, n)
    if flags.mask_heading_separated_confs or flags.mask_horizontally_separated_confs:      # :279-281
        from .feature_generation import mask_horizontally_separated_confs
        confidences = mask_horizontally_separated_confs(confidences, page_path,
                                                        mask_heading=flags.mask_heading_separated_confs,
                                                        mask_horizontal=flags.mask_horizontally_separated_confs,
                                                        device_edges=device is not None and bool(getattr(flags, "device_edges", False)),
                                                        device=device or 0)
    if flags.save_conf != "no_conf":
        gnn_results.save_conf_to_json(confidences, page_path, flags.out_dir)
        if flags.save_conf == "only_conf":
            return None
    tb.set_confs(confidences)
    tb.calc(method=flags.clustering_method)
    return gnn_results.save_clustering_to_page(tb.tb_labels, page_path, flags.out_dir, info=tb.get_info(flags.clustering_method))


def _load_session(flags, device):
    from . import gnn_io
    layers, depths = cli_flags.visual_layout(flags)
    graph = gnn_io.load_graph(resolve_model_path(flags), visual_layers=layers, visual_layer_depths=depths)
    if graph.cfg.visual_dims and not flags.image_input:
        raise ValueError("this model was exported with image_input: pass --image_input True")
    from .gnn_input import check_load_mode
    check_load_mode(flags.input_params, graph.cfg)           # load_mode against the backbone's channels, before the device sees the model
    return gnn_io.GnnSession(graph, device)


def _pages_per_call(flags):
    return max(1, int(getattr(flags, "pages_per_call", 1) or 1))


def _run_group(sess, feeds):
    """the net outputs of the feed dicts, in their order: one page through ``run`` as ever, several through one engine call"""
    if len(feeds) == 1:
        return [sess.run("output_belong_to_same_instance:0", feed_dict=feeds[0])]
    from . import gnn_io
    if gnn_io.graph_batch_serves(sess.graph.cfg):            # no visual branch: the graph part of the pages in one set of launches ->
        return sess.run_confidences(feeds)                   # the confidence matrices themselves (``_finish_page`` takes either)
    return gnn_io.run_pages(sess, feeds)


def gnn_clustering(json_paths, flags, device="0"):
    from .clustering import TextblockClustering
    from .gnn_input import InputGNN
    sess = _load_session(flags, device)
    input_fn = InputGNN(flags)
    tb = TextblockClustering(flags)
    results = []
    t0 = time.time()
    group = []

    def flush():
        """the collected pages through one engine call; their results leave in input order"""
        outputs = _run_group(sess, [feed for _, feed, _ in group])
        for (page_path, _, n), output in zip(group, outputs):
            out = _finish_page(tb, flags, output, n, page_path, device=int(device))
            if out is not None:
                results.append(out)
        del group[:]
    for count, json_path in enumerate(list(json_paths)):
        if flags.batch_limiter != -1 and flags.batch_limiter <= count:
            break
        page = _prepare_page(input_fn, flags, json_path)
        if page is None:
            continue
        group.append(page)
        if len(group) >= _pages_per_call(flags):
            flush()
    if group:                                               # the tail: fewer pages than a full call
        flush()
    logging.info(f"Time: {time.time() - t0:.2f} seconds")
    return results


# ---- host workers around one GPU owner ------------------------------------------------------------------------------------------
# The forward of a page is 0.1 - 0.7 ms; everything else of the loop above is host work (json, scan decode and resize, clustering,
# PAGE-XML: 50 - 200 ms per page).  With --num_workers > 1 the pages of a GPU go through worker processes that prepare feeds ahead
# of the owner and cluster / write behind it; the owner only runs the sessions, in list order.
_task_state = {}


def _task_objects(argv):
    key = tuple(argv)
    if key not in _task_state:
        from .clustering import TextblockClustering
        from .gnn_input import InputGNN
        flags = build_parser().parse_known_args(list(argv))[0]
        _task_state[key] = (flags, InputGNN(flags), TextblockClustering(flags))
    return _task_state[key]


def _prepare_task(argv, json_path, image_later=False):
    flags, input_fn, _ = _task_objects(argv)
    return _prepare_page(input_fn, flags, json_path, image_later)


def _finish_task(argv, output, n, page_path):
    flags, _, tb = _task_objects(argv)
    return _finish_page(tb, flags, output, n, page_path)


def _slot_decoders(host_workers):
    """of a GPU owner's host workers, those that decode scans into slots; the rest parse jsons ahead of the owner and cluster / write
    behind it.  Three of four: decoding a 4500 x 3000 png is the larger part of a page's host work, several times the rest for a colour
    scan (DESIGN section 4.4 has the measured rates).  DecodePool runs worker processes from two workers on, so a request of two starts
    two decoders and one executor process."""
    return max(2, (3 * host_workers) // 4)


class _ScanSlots:
    """--device_resize: the scans of the list's jsons, decoded ahead by DecodePool workers into page-locked shared-memory slots (a
    13 - 40 MB uint8 page is not pickled; its upload is a DMA from the slot) -> iterator over (path, page) in list order.  The workers
    are started and the first page is awaited on a thread of its own, so decoding runs while the caller loads the model; the slots are
    page-locked from that thread once the engine is there."""

    def __init__(self, json_paths, load_mode, device, host_workers):
        import threading
        from .host_pipeline import DecodePool, page_loader_name
        from .path_util import get_img_from_json_path
        present = [get_img_from_json_path(p) for p in json_paths if os.path.isfile(p)]
        pin = []

        def register(addr, nbytes):
            if not pin:
                from .host_pipeline import pin_callbacks
                pin.extend(pin_callbacks(int(device)))
            return pin[0](addr, nbytes)

        def unregister(addr):
            if pin:
                pin[1](addr)
        self._it = iter(DecodePool(present, _slot_decoders(host_workers), loader=page_loader_name(load_mode, True), register=register,
                                   unregister=unregister))
        self._first = []
        self._thread = threading.Thread(target=self._prime, daemon=True)
        self._thread.start()

    def _prime(self):
        try:
            self._first.append(("page", next(self._it)))
        except StopIteration:
            self._first.append(("end", None))
        except BaseException as e:                          # surfaced by the first __next__
            self._first.append(("error", e))

    def __iter__(self):
        return self

    def __next__(self):
        if self._thread is not None:
            self._thread.join()
            self._thread = None
            kind, value = self._first.pop()
            if kind == "page":
                return value
            if kind == "end":
                raise StopIteration
            raise value
        return next(self._it)

    def close(self):
        """stops the decode workers and releases the slots; the caller holds no view of a slot any more"""
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        del self._first[:]
        self._it.close()


def gnn_clustering_pipelined(json_paths, argv, device="0", host_workers=2):
    from concurrent.futures import ProcessPoolExecutor
    from .host_pipeline import single_threaded_children
    flags = build_parser().parse_known_args(list(argv))[0]
    json_paths = list(json_paths)
    if flags.batch_limiter != -1:
        json_paths = json_paths[:max(0, flags.batch_limiter)]
    t0 = time.time()
    results = []
    later = bool(flags.image_input and _device_resize(flags))               # the json half only: the scan comes through a slot
    executor_workers = max(1, host_workers - _slot_decoders(host_workers)) if later else host_workers
    scans = input_fn = None
    if later:                                                               # the decoders start first: they work through the model load
        from .gnn_input import InputGNN
        input_fn = InputGNN(flags)
        scans = _ScanSlots(json_paths, input_fn.input_params["load_mode"], device or 0, host_workers)
    with ProcessPoolExecutor(max(1, executor_workers), mp_context=mp.get_context("spawn")) as pool:
        def submit(fn, *args):
            with single_threaded_children():                # (the executor spawns its processes inside submit, on demand)
                return pool.submit(fn, list(argv), *args)
        ahead = 2 * max(1, host_workers)
        finishing = []
        per_call = _pages_per_call(flags)
        group = []

        def flush():
            outputs = _run_group(sess, [f for _, f, _ in group])
            for (path, _, nodes), output in zip(group, outputs):
                finishing.append(submit(_finish_task, output, nodes, path))
            del group[:]
            while len(finishing) > 4 * max(1, host_workers):                 # bounded backlog: surface errors early
                out = finishing.pop(0).result()
                if out is not None:
                    results.append(out)
        try:
            prepared = [submit(_prepare_task, p, later) for p in json_paths[:ahead]]   # the workers start on the first pages while the
            sess = _load_session(flags, device)                              # owner imports the engine and loads the model
            for k in range(len(json_paths)):
                page = prepared[k].result()
                prepared[k] = None
                if k + ahead < len(json_paths):
                    prepared.append(submit(_prepare_task, json_paths[k + ahead], later))
                if page is None:
                    continue
                page_path, feed, n = page
                if scans is not None:
                    _, scan = next(scans)                                    # (valid until the next one is asked for: run() returns
                    feed.update(input_fn.image_feeds(scan, True))            # after the page's results have arrived)
                    if per_call > 1:                                         # a page that waits for its call leaves the slot: a copy
                        feed = {k: (np.array(v) if k == "image_u8:0" else v) for k, v in feed.items()}
                    del scan
                group.append((page_path, feed, n))
                feed = page = None                                           # (no view of a slot outlives it)
                if len(group) >= per_call:
                    flush()
            if group:                                                        # the tail: fewer pages than a full call
                flush()
        finally:
            feed = page = None                                               # (also when run() raised: no view of a slot outlives it)
            del group[:]
            if scans is not None:
                scans.close()                                                # stops the decode workers, releases the slots
        for f in finishing:
            out = f.result()
            if out is not None:
                results.append(out)
    logging.info(f"Time: {time.time() - t0:.2f} seconds")
    return results


def _worker(json_paths, argv, device, q, index=0, host_workers=0):
    try:
        if host_workers > 1:
            q.put((index, "ok", gnn_clustering_pipelined(json_paths, argv, device, host_workers)))
        else:
            flags = build_parser().parse_known_args(argv)[0]
            q.put((index, "ok", gnn_clustering(json_paths, flags, device)))
    except Exception as e:  # surfaced to the parent instead of being dropped
        q.put((index, "err", repr(e)))


def _collect_results(procs, q):
    """One (worker index, "ok" | "err", payload) message per worker.  A worker that ends WITHOUT having posted its message is an
    error (native crash, OOM kill, HIP abort: fail the run, do not hang); a worker that posted its result and then exits
    non-zero (a crash at interpreter / HIP teardown) is not -- its pages are done."""
    out, errors = [], []
    reported = set()
    while len(reported) < len(procs):
        try:
            index, status, payload = q.get(timeout=1.0)
        except queue.Empty:
            dead = [k for k, pr in enumerate(procs) if k not in reported and not pr.is_alive() and pr.exitcode not in (0, None)]
            if dead and q.empty():
                errors.extend(f"worker {k} (pid {procs[k].pid}) ended with exit code {procs[k].exitcode} without a result" for k in dead)
                break
            continue
        reported.add(index)
        (out.extend if status == "ok" else errors.append)(payload)
    for pr in procs:
        if errors and pr.is_alive():
            pr.terminate()
        pr.join()
    return out, errors


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    flags = build_parser().parse_known_args(argv)[0]
    logging.getLogger().setLevel(logging.INFO)
    json_paths = [p for p in load_list_file(flags.eval_list) if p]
    devices = [str(d) for d in flags.gpu_devices] or ["0"]
    if flags.num_workers <= 1:
        return gnn_clustering(json_paths, flags, devices[0])
    # --num_workers = HOST workers (feeds ahead of / clustering and PAGE-XML behind the GPU owners), split evenly over one
    # GPU-owning process per device -- like --num_processes of run_net_post_processing; the reference forks one session-owning
    # process per sub-list (:322-340), which on one GPU means N HIP contexts and N model copies for 0.1 ms of work per page
    n_owners = max(1, min(len(devices), flags.num_workers, len(json_paths) or 1))
    host_workers = max(1, flags.num_workers // n_owners)
    if n_owners == 1:
        return gnn_clustering_pipelined(json_paths, argv, devices[0], host_workers)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = []
    for k, part in enumerate(split_list(json_paths, n_owners)):
        pr = ctx.Process(target=_worker, args=(part, argv, devices[k], q, k, host_workers))
        pr.start()
        procs.append(pr)
    out, errors = _collect_results(procs, q)
    if errors:
        raise RuntimeError("worker failure: " + "; ".join(errors))
    return out


if __name__ == "__main__":
    main()
