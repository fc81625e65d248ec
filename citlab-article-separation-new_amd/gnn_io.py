"""Drop-in mirror of the reference's GNN inference boundary

    article_separation/gnn/io.py:12-25            load_graph(pb_path)
    article_separation/gnn/run_gnn_clustering.py:216-269
        sess = tf.Session(graph=graph); out = sess.run(output_node, feed_dict=...)

``load_graph`` returns a :class:`GnnGraph`; ``GnnSession(graph).run(fetch, feed_dict)`` accepts the
reference's feed keys *by tensor name* (``run_gnn_clustering.py:76-148``, names fixed at export time by
``model_relation.py:258-337``) and returns ``[1, R, num_classes]`` float32 like the frozen graph did.
The TensorFlow runtime underneath is replaced by ``csrc/libasep_hip.so`` (``include/asep_hip.h``).
"""
import ctypes as C
import os
import warnings

import numpy as np

from . import _lib
from .config import GnnConfig
from .weights import load_weights, pack_blob

OUTPUT_NODE = "output_belong_to_same_instance:0"
FEED_NAMES = (
    "num_nodes:0", "num_interacting_nodes:0", "interacting_nodes:0", "node_features:0", "edge_features:0",
    "image:0", "image_shape:0", "visual_regions_nodes:0", "num_points_visual_regions_nodes:0",
    "visual_regions_edges:0", "num_points_visual_regions_edges:0",
    "relations_to_consider_belong_to_same_instance:0",
)
# extension: the scan as decoded (uint8 [1,H,W], [1,H,W,1] or [1,H,W,3]) in place of 'image:0'; the engine resizes it on the device to
# the [h, w] of 'image_shape:0' (gnn_input.resize_bilinear_tf1 bit for bit, include/asep_hip.h asep_prep_resize_tf1_dev)
IMAGE_U8 = "image_u8:0"


class GnnGraph:
    def __init__(self, tensors, cfg: GnnConfig, path: str = None):
        self.tensors = tensors
        self.cfg = cfg
        self.path = path
        self._blob = None
        self._handles = {}
        self._backbones = {}

    def blob(self) -> bytes:
        """GNN + compression-layer tensors (the backbone goes into its own ARU-Net handle)."""
        if self._blob is None:
            self._blob = pack_blob({k: v for k, v in self.tensors.items() if not k.startswith("aru_net/")})
        return self._blob

    def backbone_graph(self):
        """ARU-Net over the ``aru_net/...`` tensors of the same frozen graph (graph_relation.py:17-22)."""
        from .net_post_processing_helper import AruGraph
        return AruGraph({k: v for k, v in self.tensors.items() if k.startswith("aru_net/")}, self.cfg.backbone_cfg(),
                        self.path)

    def handle(self, device_id: int = 0):
        if device_id not in self._handles:
            lib = _lib.init_device(device_id)
            c = self.cfg
            def widths(name, lst, lo, hi=_lib.MLP_MAX_HIDDEN):
                """the hidden-width list of an MLP as `hi` struct fields (0 = absent)"""
                lst = [int(v) for v in lst]
                if not lo <= len(lst) <= hi or any(v < 1 for v in lst):
                    raise _lib.AsepError(f"{name} = {lst}: the engine serves {lo} to {hi} hidden layers of positive width")
                return lst + [0] * (hi - len(lst))
            ih = widths("num_hidden_units_interaction_fct", c.interaction_hidden, 1)
            ah = widths("num_hidden_units_attention_fct", c.attention_hidden, 1) if c.use_attention else [0, 0, 0, 0]
            ch = widths("num_hidden_units (classifier)", c.classifier_hidden, 1)
            if c.visual_edges and not c.visual_dims:
                raise _lib.AsepError("visual_edges needs the visual branch (visual_dims / visual_layers)")
            cfg = _lib.GnnCfg(c.u_dim, c.edge_in_dim, c.num_transition_steps, c.hidden_dim,
                              c.interaction_dim, ih[0], ch[0], ch[1], c.num_classes, int(c.undirected_graph),
                              c.u_in_dim if c.compress_node_feature_dim > 0 else 0, c.output_type_code,
                              c.num_attention_heads if c.use_attention else 0,
                              {"concat": 0, "average": 1}[c.multihead_attention_merge_type], ah[0],
                              c.aggregation_code, ih[1], ih[2], ih[3], ah[1], ah[2], ah[3], ch[2], ch[3],
                              int(c.incorporate_hidden_features_in_update), int(c.incorporate_node_input_features_in_update),
                              c.visual_edge_dim)
            blob = self.blob()
            h = lib.asep_gnn_load(blob, len(blob), C.byref(cfg))
            if not h:
                raise _lib.AsepError("asep_gnn_load failed: " + _lib.last_error())
            if c.visual_dims:
                bb = self.backbone_graph()
                names = (C.c_char_p * len(c.visual_layers))(*[n.encode() for n in c.visual_layers])
                try:
                    depths = c.layer_depths()                # (refuses a layout the reference cannot build, with the reason)
                except ValueError as e:
                    lib.asep_gnn_free(h)
                    raise _lib.AsepError(str(e))
                if any(d != -1 for d in depths):             # generated maps (feature_map_generators.py:72-197)
                    rc = lib.asep_gnn_attach_backbone_maps(h, bb.handle(device_id), len(c.visual_layers), names,
                                                           (C.c_int32 * len(depths))(*depths))
                else:
                    rc = lib.asep_gnn_attach_backbone(h, bb.handle(device_id), len(c.visual_layers), names)
                if rc < 0:
                    lib.asep_gnn_free(h)
                    raise _lib.AsepError("asep_gnn_attach_backbone failed: " + _lib.last_error())
                self._backbones[device_id] = bb          # keeps the ARU-Net handle alive
            self._handles[device_id] = h
        return self._handles[device_id]

    def close(self):
        if self._handles:
            lib = _lib.load_library()
            for h in self._handles.values():
                lib.asep_gnn_free(h)
            self._handles = {}
            for bb in self._backbones.values():
                bb.close()
            self._backbones = {}

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def load_graph(pb_path, visual_layers=None, num_transition_steps=None, visual_layer_depths=None) -> GnnGraph:
    """gnn/io.py:12-25.  Accepts a TF1 frozen graph (``*.pb``, decoded without TensorFlow by ``pb_import.py``)
    or the engine's ``*.asepw`` container (+ ``.json`` side-car).  ``visual_layers`` names the backbone end points
    of a graph exported with ``--image_input`` (``--feature_map_generation_params from_layer=[...]``); the names
    are not recoverable from the constants alone, the default is ``scale_0_unet_up_<level>_conv`` per map.
    ``num_transition_steps`` is read from the op graph (one edge-MLP MatMul per step); only a constants-only container
    without that structure needs it passed in.  ``visual_layer_depths``: the ``layer_depth`` list of a layout with generated maps
    (``''`` in ``visual_layers`` = from the previous map); a frozen graph says the depths itself (the generator's variable names), what is
    passed must agree with it."""
    if isinstance(pb_path, GnnGraph):
        return pb_path
    if not os.path.isfile(pb_path):
        raise IOError(f"No such model file: {pb_path}")
    if str(pb_path).endswith(".pb"):
        from . import pb_import
        tensors, cfg = pb_import.gnn_from_nodes(pb_import.read_graph(pb_path), visual_layers=visual_layers,
                                                num_transition_steps=num_transition_steps, visual_layer_depths=visual_layer_depths)
    else:
        tensors, meta = load_weights(pb_path)
        cfg = GnnConfig(**(meta or {}).get("gnn_cfg", {}))
        if visual_layer_depths is not None and [int(d) for d in visual_layer_depths] != cfg.layer_depths():
            raise IOError(f"visual_layer_depths {list(visual_layer_depths)} given, the container was written for {cfg.layer_depths()}")
    if cfg.visual_dims:                                      # ASEP_COMPUTE_DTYPE: the conv backbone of the visual branch (graph stays fp32)
        from .net_post_processing_helper import compute_dtype_from_env
        cfg.backbone = dict(cfg.backbone, compute_dtype=compute_dtype_from_env(cfg.backbone.get("compute_dtype", cfg.backbone_cfg().compute_dtype)))
    return GnnGraph(tensors, cfg, pb_path)


def _key(k):
    """feed_dict keys may be tensor names ('num_nodes:0'), bare names, or objects with a .name."""
    name = getattr(k, "name", k)
    if not isinstance(name, str):
        raise KeyError(f"unsupported feed key {k!r}")
    return name if ":" in name else name + ":0"


class GnnSession:
    """Stands in for ``tf.Session(graph=graph)`` in ``run_gnn_clustering.py:221``."""

    def __init__(self, graph: GnnGraph, gpu_devices="0"):
        self.graph = graph
        self.device = 0 if gpu_devices in (None, "") else int(str(gpu_devices).split(",")[0])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def page_arrays(self, feed_dict):
        """the arrays ``run`` takes out of a feed dict, checked the same way (for :func:`run_pages`): N, E, edges, u, ef, rel, and for a
        visual model image | page_u8 + size, regions, npts, eregions, enpts"""
        feed = {_key(k): v for k, v in feed_dict.items()}
        for k in feed:
            if k not in FEED_NAMES and k != IMAGE_U8:
                raise KeyError(f"The name '{k}' refers to a Tensor which does not exist")
        if IMAGE_U8 in feed and "image:0" in feed:
            raise KeyError(f"feed_dict holds both image:0 and {IMAGE_U8}: feed the resized image or the scan, not both")
        cfg = self.graph.cfg
        num_nodes = np.asarray(feed["num_nodes:0"]).reshape(-1)
        if num_nodes.shape[0] != 1:
            raise ValueError("batch size must be 1 (input_dataset.py:134)")
        N = int(num_nodes[0])
        E = int(np.asarray(feed["num_interacting_nodes:0"]).reshape(-1)[0])
        a = {"N": N, "E": E, "edges": np.ascontiguousarray(np.asarray(feed["interacting_nodes:0"], dtype=np.int32)[0][:E]).reshape(-1, 2)}
        if "node_features:0" in feed:
            u = np.ascontiguousarray(np.asarray(feed["node_features:0"], dtype=np.float32)[0][:N])
        elif cfg.visual_dims and cfg.node_feature_dim == 0:
            u = np.zeros((N, 0), dtype=np.float32)
        else:
            raise KeyError("feed_dict lacks node_features:0")
        if u.shape[1] != cfg.node_feature_dim:
            raise ValueError(f"node_features has dim {u.shape[1]}, model expects {cfg.node_feature_dim}")
        a["u"] = u
        a["ef"] = None
        if cfg.edge_feature_dim:
            ef = np.ascontiguousarray(np.asarray(feed["edge_features:0"], dtype=np.float32)[0][:E])
            if ef.shape[1] != cfg.edge_feature_dim:
                raise ValueError(f"edge_features has dim {ef.shape[1]}, model expects {cfg.edge_feature_dim}")
            a["ef"] = ef
        a["rel"] = np.ascontiguousarray(np.asarray(feed["relations_to_consider_belong_to_same_instance:0"], dtype=np.int32)[0]).reshape(-1, 2)
        a["eregions"] = a["enpts"] = None
        if cfg.visual_dims:
            from_scan = IMAGE_U8 in feed
            for k in ((IMAGE_U8, "image_shape:0") if from_scan else ("image:0",)) + ("visual_regions_nodes:0",
                                                                                     "num_points_visual_regions_nodes:0"):
                if k not in feed:
                    raise KeyError(f"this graph was exported with image_input: feed_dict lacks {k}")
            image = np.asarray(feed[IMAGE_U8]) if from_scan else np.asarray(feed["image:0"], dtype=np.float32)
            if image.shape[0] != 1:
                raise ValueError("batch size must be 1 (input_dataset.py:134)")
            image = image[0]
            if from_scan:
                if image.dtype != np.uint8:
                    raise ValueError(f"{IMAGE_U8} is the scan as decoded (uint8), got {image.dtype}")
                ish = np.asarray(feed["image_shape:0"]).reshape(-1, 3)[0]
                if int(ish[0]) < 1 or int(ish[1]) < 1:
                    raise ValueError(f"the target size must be positive, got {int(ish[0])} x {int(ish[1])}")
                a["page_u8"], a["size"] = image, (int(ish[0]), int(ish[1]))
            else:
                if "image_shape:0" in feed:                 # crop to the true shape (no padding at batch size 1)
                    ish = np.asarray(feed["image_shape:0"]).reshape(-1, 3)[0]
                    image = image[:int(ish[0]), :int(ish[1])]
                a["image"] = image
            a["regions"] = np.ascontiguousarray(np.asarray(feed["visual_regions_nodes:0"], dtype=np.float32)[0][:N])
            a["npts"] = np.ascontiguousarray(np.asarray(feed["num_points_visual_regions_nodes:0"], dtype=np.int32)[0][:N]).reshape(N)
            if cfg.visual_edges:                            # graph_relation.py:141-146
                for k in ("visual_regions_edges:0", "num_points_visual_regions_edges:0"):
                    if k not in feed:
                        raise KeyError(f"this graph assigns visual features to edges: feed_dict lacks {k}")
                a["eregions"] = np.ascontiguousarray(np.asarray(feed["visual_regions_edges:0"], dtype=np.float32)[0][:E])
                a["enpts"] = np.ascontiguousarray(np.asarray(feed["num_points_visual_regions_edges:0"], dtype=np.int32)[0][:E]).reshape(E)
        return a

    def run_confidences(self, feed_dicts):
        """the confidence matrices [N_b, N_b] of several pages of a graph without visual features from ONE engine call
        (asep_gnn_forward_batch); per page ``confidences_from_output(self.run(...))`` bit for bit"""
        return page_confidences(self, list(feed_dicts))

    def run(self, fetches, feed_dict):
        name = _key(fetches)
        if name != OUTPUT_NODE:
            raise KeyError(f"The name '{name}' refers to a Tensor which does not exist (only {OUTPUT_NODE})")
        a = self.page_arrays(feed_dict)                      # one parser for run and run_pages
        cfg = self.graph.cfg
        N, edges, u, ef, rel = a["N"], a["edges"], a["u"], a["ef"], a["rel"]
        if cfg.visual_dims:
            if "page_u8" in a:
                probs = gnn_forward_visual_u8(self.graph, N, edges, u, ef, a["page_u8"], a["size"][0], a["size"][1], a["regions"], a["npts"], rel,
                                              self.device, edge_regions=a["eregions"], edge_num_points=a["enpts"])
            else:
                probs = gnn_forward_visual(self.graph, N, edges, u, ef, a["image"], a["regions"], a["npts"], rel, self.device,
                                           edge_regions=a["eregions"], edge_num_points=a["enpts"])
        else:
            probs = gnn_forward(self.graph, N, edges, u, ef, rel, self.device)
        return probs[None]


def pack_graph_pages(pages, node_dim, edge_dim):
    """the pages of one asep_gnn_forward_batch call one behind the other: ``pages`` = dicts with N, edges [E, 2] (page-local node numbers),
    u [N, node_dim], ef [E, edge_dim] or None, rel [R, 2] or None (all N * N ordered pairs) -> (N, E, R int32 arrays, u, edges, ef, rel);
    rel is None when no page lists relations (a call lists them for all of its pages or for none)"""
    N = np.array([int(p["N"]) for p in pages], np.int32)
    edges = [np.ascontiguousarray(p["edges"], dtype=np.int32).reshape(-1, 2) for p in pages]
    E = np.array([e.shape[0] for e in edges], np.int32)
    listed = [p.get("rel") is not None for p in pages]
    if any(listed) and not all(listed):
        raise ValueError("the pages of one call list their relations all or none")
    rels = [np.ascontiguousarray(p["rel"], dtype=np.int32).reshape(-1, 2) for p in pages] if all(listed) else None
    R = np.array([r.shape[0] for r in rels] if rels is not None else [int(n) * int(n) for n in N], np.int32)
    u = np.concatenate([np.ascontiguousarray(p["u"], dtype=np.float32).reshape(int(p["N"]), node_dim) for p in pages], axis=0)
    ef = None
    if edge_dim:
        ef = np.concatenate([np.ascontiguousarray(p["ef"], dtype=np.float32).reshape(e.shape[0], edge_dim) if e.shape[0]
                             else np.zeros((0, edge_dim), np.float32) for p, e in zip(pages, edges)], axis=0)
    return (N, E, R, np.ascontiguousarray(u), np.ascontiguousarray(np.concatenate(edges, axis=0)), ef,
            np.ascontiguousarray(np.concatenate(rels, axis=0)) if rels is not None else None)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def gnn_forward_batch(graph: GnnGraph, pages, device=0):
    """The graph part of several pages in ONE engine call (asep_gnn_forward_batch: every stage one launch over all pages), for a graph
    without visual features -> per page the class-1 probabilities of its relations [R_b] (R_b = N_b * N_b ordered pairs row major when
    the pages list no relations): the values of :func:`gnn_forward` ``[:, 1]`` on the page alone, bit for bit.  ``pages``:
    :func:`pack_graph_pages`."""
    lib = _lib.init_device(device)
    cfg = graph.cfg
    N, E, R, u, edges, ef, rel = pack_graph_pages(pages, cfg.node_feature_dim, cfg.edge_feature_dim)
    out = np.empty(max(int(R.sum(dtype=np.int64)), 1), dtype=np.float32)
    rc = lib.asep_gnn_forward_batch(graph.handle(device), len(N), _i32p(N), _i32p(E), _i32p(R), u.ctypes.data,
                                    edges.ctypes.data if edges.size else None, ef.ctypes.data if ef is not None and ef.size else None,
                                    rel.ctypes.data if rel is not None and rel.size else None, out.ctypes.data, int(R.sum(dtype=np.int64)))
    _lib.check(rc, "asep_gnn_forward_batch")
    ends = np.cumsum(R.astype(np.int64))
    return [out[int(e - r):int(e)].copy() for e, r in zip(ends, R)]


def gnn_forward_batch_dev(graph: GnnGraph, N, E, R, d_node_feat, d_edges, d_edge_feat, d_relations, d_probs_out, max_floats, stream=None,
                          device=0):
    """asep_gnn_forward_batch_dev: the same call on device addresses (N, E, R: host int32 arrays), queued on ``stream``"""
    lib = _lib.init_device(device)
    N, E, R = (np.ascontiguousarray(a, dtype=np.int32) for a in (N, E, R))
    rc = lib.asep_gnn_forward_batch_dev(graph.handle(device), len(N), _i32p(N), _i32p(E), _i32p(R), d_node_feat, d_edges, d_edge_feat,
                                        d_relations, d_probs_out, int(max_floats), stream)
    _lib.check(rc, "asep_gnn_forward_batch_dev")


def graph_batch_serves(cfg) -> bool:
    """whether --pages_per_call N > 1 groups this graph's pages into asep_gnn_forward_batch calls: no visual features (those pages go
    through the visual batch call), and two classes (the call returns the class-1 probability, which is then every consumer's score)"""
    return not cfg.visual_dims and not cfg.visual_edges and cfg.num_classes == 2


def page_confidences(sess, feed_dicts):
    """feed dicts of several pages -> their confidence matrices [N_b, R_b / N_b] (``gnn_results.confidences_from_output`` of ``sess.run``,
    bit for bit) from ONE batched graph call"""
    arrays = [sess.page_arrays(f) for f in feed_dicts]
    for a in arrays:
        _check_node_indices("interacting_nodes", a["edges"], a["N"])
        _check_node_indices("relations", a["rel"], a["N"])
    probs = gnn_forward_batch(sess.graph, arrays, sess.device)
    return [np.reshape(p, [a["N"], -1]) for p, a in zip(probs, arrays)]


def gnn_page_hidden(graph: GnnGraph, page, num_nodes, device=0):
    """hidden states [N_b, hidden_dim] of page ``page`` of the last batched graph call"""
    lib = _lib.init_device(device)
    out = np.empty((int(num_nodes), graph.cfg.hidden_dim), dtype=np.float32)
    _lib.check(lib.asep_gnn_get_page_hidden(graph.handle(device), int(page), out.ctypes.data, out.size), "asep_gnn_get_page_hidden")
    return out


def gnn_page_edges(graph: GnnGraph, page, num_edges, device=0):
    """corrected edge list of page ``page`` of the last batched graph call -> (edges [E', 2], first occurrence [E']), as
    :func:`correct_edges` orders them; ``num_edges``: the page's fed edges"""
    lib = _lib.init_device(device)
    cap = max((2 if graph.cfg.undirected_graph else 1) * int(num_edges), 1)
    out_e, out_f = np.empty((cap, 2), np.int32), np.empty(cap, np.int32)
    n = lib.asep_gnn_get_page_edges(graph.handle(device), int(page), out_e.ctypes.data, out_f.ctypes.data, cap)
    _lib.check(n, "asep_gnn_get_page_edges")
    return out_e[:n].copy(), out_f[:n].copy()


def gnn_batch_launches(graph: GnnGraph, device=0) -> int:
    """kernels the handle's last batched graph call launched (0: it was refused before any launch)"""
    return int(_lib.init_device(device).asep_gnn_batch_launches(graph.handle(device)))


def run_pages(sess: GnnSession, feed_dicts):
    """``[sess.run(OUTPUT_NODE, f) for f in feed_dicts]`` with the pages of a visual model in ONE engine call
    (:func:`gnn_forward_visual_batch_dev2`), whatever their image sizes; fed as 'image:0' or as 'image_u8:0' scans.  A model without
    the visual branch, or a single page, goes through ``run``: its graph part has nothing to share between pages.  The outputs are
    those of ``run`` bit for bit, in the order of ``feed_dicts``."""
    feeds = list(feed_dicts)
    cfg = sess.graph.cfg
    if len(feeds) < 2 or not cfg.visual_dims:
        return [sess.run(OUTPUT_NODE, f) for f in feeds]
    import torch
    device = sess.device
    handle = sess.graph.handle(device)                       # (initialises the device before torch allocates on it)
    dev = torch.device("cuda", int(device))
    chans = cfg.backbone_cfg().channels
    keep, pages, hs, ws, outs, scans = [], [], [], [], [], []
    P = None
    with torch.cuda.device(dev):
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev) if x is not None and x.size else None      # noqa: E731
        ptr = lambda t: t.data_ptr() if t is not None else None                                                      # noqa: E731
        for feed in feeds:
            a = sess.page_arrays(feed)
            N, E = a["N"], a["E"]
            _check_node_indices("interacting_nodes", a["edges"], N)
            _check_node_indices("relations", a["rel"], N)
            with warnings.catch_warnings():                  # (a page Pillow decoded is read-only: it is only read here)
                warnings.simplefilter("ignore", UserWarning)
                if "page_u8" in a:
                    h, w = a["size"]
                    resize_mode(a["page_u8"].shape, chans)   # (a gray scan into a colour backbone: the ValueError of the single-page path)
                    d_image = up(a["page_u8"])
                    sh = a["page_u8"].shape
                    scans.append((d_image.data_ptr(), sh[0], sh[1], sh[2] if len(sh) == 3 else 1))
                else:
                    img = a["image"]
                    got = img.shape[2] if img.ndim == 3 else 1
                    if img.ndim not in (2, 3) or got != chans:
                        raise ValueError(f"this graph's backbone takes {chans} image channel(s), the image {img.shape} has {got}")
                    if img.ndim == 3 and chans == 1:
                        img = img[:, :, 0]
                    d_image = up(img)
                    h, w = img.shape[:2]
            if P is None:
                P = a["regions"].shape[2]
            if a["regions"].ndim != 3 or a["regions"].shape[:2] != (N, 2) or a["regions"].shape[2] != P:
                raise ValueError(f"visual_regions_nodes must be [N, 2, {P}] on every page of a call, got {a['regions'].shape}")
            if cfg.visual_edges and a["eregions"].shape != (E, 2, P):
                raise ValueError(f"visual_regions_edges must be [E, 2, P] = {(E, 2, P)}, got {a['eregions'].shape}")
            t = [up(a[k]) for k in ("edges", "u", "ef", "regions", "npts", "eregions", "enpts", "rel")]
            R = a["rel"].shape[0]
            out = torch.empty((R, cfg.num_classes), dtype=torch.float32, device=dev)
            keep.append((t, d_image))
            outs.append(out)
            hs.append(int(h)); ws.append(int(w))
            pages.append(dict(N=N, E=E, R=R, d_edges=ptr(t[0]), d_node_feat=ptr(t[1]), d_edge_feat=ptr(t[2]) if E else None,
                              d_image=d_image.data_ptr(), d_regions=ptr(t[3]), d_num_points=ptr(t[4]),
                              d_edge_regions=ptr(t[5]) if E else None, d_edge_num_points=ptr(t[6]) if E else None,
                              d_relations=ptr(t[7]), d_probs_out=out.data_ptr() if R else None))
        if scans and len(scans) != len(pages):
            raise ValueError("the pages of one call are fed all as image:0 or all as image_u8:0")
        stream = torch.cuda.current_stream(dev)
        if scans:                                            # every scan resized in one launch, in front of the grouped backbone
            for d in pages:
                d["d_image"] = None
            gnn_forward_visual_batch_u8_dev(sess.graph, pages, scans, hs, ws, P, stream.cuda_stream or None, device)
        else:
            gnn_forward_visual_batch_dev2(sess.graph, pages, hs, ws, P, stream.cuda_stream or None, device)
        results = [o.cpu().numpy()[None] for o in outs]      # (waits for the stream: the uploads above stay alive until here)
    del handle, keep
    return results


def gnn_forward(graph: GnnGraph, num_nodes, edges, node_feat, edge_feat, relations=None, device=0):
    """One page through the engine -> probabilities [R, num_classes] (R = N*N when relations is None)."""
    lib = _lib.init_device(device)
    N = int(num_nodes)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    u = np.ascontiguousarray(node_feat, dtype=np.float32).reshape(N, -1)
    ef = np.ascontiguousarray(edge_feat, dtype=np.float32).reshape(E, -1) if edge_feat is not None else None
    if relations is None:
        R, rel_p = N * N, None
    else:
        rel = np.ascontiguousarray(relations, dtype=np.int32).reshape(-1, 2)
        R, rel_p = rel.shape[0], rel.ctypes.data
    out = np.empty((R, graph.cfg.num_classes), dtype=np.float32)
    rc = lib.asep_gnn_forward(graph.handle(device), N, E, edges.ctypes.data if E else None, u.ctypes.data,
                              ef.ctypes.data if (ef is not None and E) else None, R, rel_p, out.ctypes.data)
    _lib.check(rc, "asep_gnn_forward")
    return out


def gnn_forward_visual(graph: GnnGraph, num_nodes, edges, node_feat, edge_feat, image, regions, num_points,
                       relations=None, device=0, edge_regions=None, edge_num_points=None):
    """graph_relation.py:84-139 + GNN: image float32 [h,w(,1)] as fed (0..255; [h,w,3] in R, G, B order when the backbone was trained
    with ``load_mode=RGB``, a mismatch of the channel counts is a ``ValueError``), regions [N,2,P] relative
    coordinates, num_points [N] -> probabilities [R, num_classes].  ``edge_regions`` [E,2,P] / ``edge_num_points`` [E]: the
    interactions' regions of a graph with ``visual_edges`` (graph_relation.py:141-172)."""
    lib = _lib.init_device(device)
    cfg = graph.cfg
    N = int(num_nodes)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    u = np.ascontiguousarray(node_feat, dtype=np.float32).reshape(N, cfg.node_feature_dim)
    ef = np.ascontiguousarray(edge_feat, dtype=np.float32).reshape(E, -1) if edge_feat is not None else None
    img = np.asarray(image, dtype=np.float32)
    chans = cfg.backbone_cfg().channels
    got = img.shape[2] if img.ndim == 3 else 1
    if img.ndim not in (2, 3) or got != chans:
        raise ValueError(f"this graph's backbone takes {chans} image channel(s), the image {img.shape} has {got}")
    if img.ndim == 3 and chans == 1:
        img = img[:, :, 0]
    img = np.ascontiguousarray(img)                          # [h,w], or the interleaved [h,w,3] of a colour backbone
    reg = np.ascontiguousarray(regions, dtype=np.float32)
    if reg.ndim != 3 or reg.shape[0] != N or reg.shape[1] != 2:
        raise ValueError(f"visual_regions_nodes must be [N, 2, P], got {reg.shape}")
    npts = np.ascontiguousarray(num_points, dtype=np.int32).reshape(N)
    ereg_p = enp_p = None
    if cfg.visual_edges:
        if edge_regions is None or edge_num_points is None:
            raise ValueError("this graph assigns visual features to edges: edge_regions / edge_num_points required")
        ereg = np.ascontiguousarray(edge_regions, dtype=np.float32)
        if ereg.shape != (E, 2, reg.shape[2]):
            raise ValueError(f"visual_regions_edges must be [E, 2, P] = {(E, 2, reg.shape[2])}, got {ereg.shape}")
        enp = np.ascontiguousarray(edge_num_points, dtype=np.int32).reshape(E)
        if E:
            ereg_p, enp_p = ereg.ctypes.data, enp.ctypes.data
    if relations is None:
        R, rel_p = N * N, None
    else:
        rel = np.ascontiguousarray(relations, dtype=np.int32).reshape(-1, 2)
        R, rel_p = rel.shape[0], rel.ctypes.data
    out = np.empty((R, cfg.num_classes), dtype=np.float32)
    rc = lib.asep_gnn_forward_visual(graph.handle(device), N, E, edges.ctypes.data if E else None,
                                     u.ctypes.data if u.size else None,
                                     ef.ctypes.data if (ef is not None and ef.size and E) else None, img.ctypes.data,
                                     img.shape[0], img.shape[1], reg.ctypes.data, reg.shape[2], npts.ctypes.data,
                                     ereg_p, enp_p, R, rel_p, out.ctypes.data)
    _lib.check(rc, "asep_gnn_forward_visual")
    return out


def resize_mode(page_shape, backbone_channels):
    """how a uint8 page [H,W] / [H,W,1] / [H,W,3] reaches a backbone of ``backbone_channels``: 'keep' when the counts agree, 'luma'
    (Pillow's ``convert('L')``, taken per tap on the device) for a colour page into a gray backbone; a gray page into a colour
    backbone is the ``ValueError`` of :func:`gnn_forward_visual`"""
    got = page_shape[2] if len(page_shape) == 3 else 1
    if len(page_shape) not in (2, 3) or got not in (1, 3) or (got != backbone_channels and not (got == 3 and backbone_channels == 1)):
        raise ValueError(f"this graph's backbone takes {backbone_channels} image channel(s), the image {tuple(page_shape)} has {got}")
    return "keep" if got == backbone_channels else "luma"


def _check_node_indices(what, idx, N):
    """the host-pointer entries refuse an index outside the page (csrc/gnn_engine.hip check_indices); the device entries cannot"""
    bad = np.flatnonzero(((idx < 0) | (idx >= N)).any(axis=1)) if idx.size else ()
    if len(bad):
        i = int(bad[0])
        raise _lib.AsepError(f"{what}[{i}] = ({int(idx[i, 0])}, {int(idx[i, 1])}) names a node outside 0..{N - 1}")


def gnn_forward_visual_u8(graph: GnnGraph, num_nodes, edges, node_feat, edge_feat, page_u8, h, w, regions, num_points,
                          relations=None, device=0, edge_regions=None, edge_num_points=None):
    """:func:`gnn_forward_visual` from the scan as decoded: ``page_u8`` uint8 [H,W(,1)] or [H,W,3] (R, G, B) is uploaded as it is and
    resized to [h,w] on the device (``asep_prep_resize_tf1_dev`` = ``gnn_input.resize_bilinear_tf1`` bit for bit; a colour page
    for a gray backbone becomes Pillow's ``convert('L')`` there), then ``asep_gnn_forward_visual_dev`` runs behind it on torch's
    current stream.  ``h``, ``w``: ``gnn_input.compute_new_size`` of the page.  The device buffers are torch tensors."""
    import torch
    from . import image_ops
    cfg = graph.cfg
    N = int(num_nodes)
    page = np.asarray(page_u8)
    if page.dtype != np.uint8:
        raise ValueError(f"the page is the scan as decoded (uint8), got {page.dtype}")
    mode = resize_mode(page.shape, cfg.backbone_cfg().channels)
    if int(h) < 1 or int(w) < 1:
        raise ValueError(f"the target size must be positive, got {h} x {w}")
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    _check_node_indices("interacting_nodes", edges, N)
    u = np.ascontiguousarray(node_feat, dtype=np.float32).reshape(N, cfg.node_feature_dim)
    ef = np.ascontiguousarray(edge_feat, dtype=np.float32).reshape(E, -1) if edge_feat is not None else None
    reg = np.ascontiguousarray(regions, dtype=np.float32)
    if reg.ndim != 3 or reg.shape[0] != N or reg.shape[1] != 2:
        raise ValueError(f"visual_regions_nodes must be [N, 2, P], got {reg.shape}")
    npts = np.ascontiguousarray(num_points, dtype=np.int32).reshape(N)
    ereg = enp = None
    if cfg.visual_edges:
        if edge_regions is None or edge_num_points is None:
            raise ValueError("this graph assigns visual features to edges: edge_regions / edge_num_points required")
        ereg = np.ascontiguousarray(edge_regions, dtype=np.float32)
        if ereg.shape != (E, 2, reg.shape[2]):
            raise ValueError(f"visual_regions_edges must be [E, 2, P] = {(E, 2, reg.shape[2])}, got {ereg.shape}")
        enp = np.ascontiguousarray(edge_num_points, dtype=np.int32).reshape(E)
    rel = None
    R = N * N
    if relations is not None:
        rel = np.ascontiguousarray(relations, dtype=np.int32).reshape(-1, 2)
        R = rel.shape[0]
        _check_node_indices("relations", rel, N)
    handle = graph.handle(device)                            # (initialises the device before torch allocates on it)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        up = lambda x: torch.from_numpy(x).to(dev, non_blocking=True) if x is not None and x.size else None      # noqa: E731
        ptr = lambda t: t.data_ptr() if t is not None else None                                                  # noqa: E731
        with warnings.catch_warnings():                      # (a page Pillow decoded is read-only: it is only read here)
            warnings.simplefilter("ignore", UserWarning)
            d_page = torch.from_numpy(np.ascontiguousarray(page)).to(dev, non_blocking=True)     # a DMA from a page-locked slot
        d_image = image_ops.resize_tf1_dev(d_page, h, w, mode, device)
        t = [up(a) for a in (edges, u, ef, reg, npts, ereg, enp, rel)]
        out = torch.empty((R, cfg.num_classes), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        gnn_forward_visual_dev(graph, N, E, ptr(t[0]), ptr(t[1]), ptr(t[2]) if E else None, d_image.data_ptr(), int(h), int(w),
                               ptr(t[3]), reg.shape[2], ptr(t[4]), R, ptr(t[7]), out.data_ptr() if R else None,
                               stream.cuda_stream or None, device, d_edge_regions=ptr(t[5]) if E else None,
                               d_edge_num_points=ptr(t[6]) if E else None)
        probs = out.cpu().numpy()                            # (waits for the stream: the uploads above stay alive until here)
    del handle
    return probs


def gnn_forward_visual_dev(graph: GnnGraph, num_nodes, num_edges, d_edges, d_node_feat, d_edge_feat, d_image, h, w, d_regions,
                           num_region_points, d_num_points, num_relations, d_relations, d_probs_out, stream=None, device=0,
                           d_edge_regions=None, d_edge_num_points=None):
    """``asep_gnn_forward_visual_dev``: every array is a device address (int), nothing is synchronised -- the call returns
    once backbone, ROI kernels and the graph are queued on ``stream`` (a hipStream_t handle as int, None = null stream)."""
    lib = _lib.init_device(device)
    rc = lib.asep_gnn_forward_visual_dev(graph.handle(device), int(num_nodes), int(num_edges), d_edges, d_node_feat,
                                         d_edge_feat, d_image, int(h), int(w), d_regions, int(num_region_points),
                                         d_num_points, d_edge_regions, d_edge_num_points, int(num_relations), d_relations,
                                         d_probs_out, stream)
    _lib.check(rc, "asep_gnn_forward_visual_dev")


def gnn_forward_visual_batch_dev(graph: GnnGraph, pages, h, w, num_region_points, stream=None, device=0):
    """``asep_gnn_forward_visual_batch_dev``: ``pages`` is a sequence of dicts with the fields of ``asep_gnn_page`` (device
    addresses as ints; ``d_relations`` may be None = all N*N ordered pairs) or a ready ``(_lib.GnnPage * n)`` array.  The
    backbones of all pages run as one grouped forward; nothing is synchronised."""
    lib = _lib.init_device(device)
    if not isinstance(pages, C.Array):
        arr = (_lib.GnnPage * len(pages))()
        for q, d in zip(arr, pages):
            for k, v in d.items():
                setattr(q, k, v)
        pages = arr
    rc = lib.asep_gnn_forward_visual_batch_dev(graph.handle(device), len(pages), pages, int(h), int(w), int(num_region_points),
                                               stream)
    _lib.check(rc, "asep_gnn_forward_visual_batch_dev")
    return pages


def gnn_forward_visual_batch_dev2(graph: GnnGraph, pages, hs, ws, num_region_points, stream=None, device=0):
    """``asep_gnn_forward_visual_batch_dev2``: :func:`gnn_forward_visual_batch_dev` for pages of different image sizes, ``hs[b]`` x
    ``ws[b]`` being page b's.  One grouped backbone forward, one launch per generated-map convolution and one for all regions over
    a page table, the graphs page by page; per page the results of the single-page call bit for bit.  Like every float entry it trusts
    ``d_image`` to hold ``hs[b] * ws[b] *`` (the backbone's channels) values: a page struct carries no channel count (the u8 entry does, and
    checks it).  Queued on ``stream``; the only host wait is on a table buffer whose readers were queued four calls back."""
    lib = _lib.init_device(device)
    if not isinstance(pages, C.Array):
        arr = (_lib.GnnPage * len(pages))()
        for q, d in zip(arr, pages):
            for k, v in d.items():
                setattr(q, k, v)
        pages = arr
    n = len(pages)
    if len(hs) != n or len(ws) != n:
        raise ValueError(f"{n} pages, {len(hs)} heights and {len(ws)} widths")
    Ints = C.c_int32 * max(n, 1)
    rc = lib.asep_gnn_forward_visual_batch_dev2(graph.handle(device), n, pages, Ints(*[int(v) for v in hs]), Ints(*[int(v) for v in ws]),
                                                int(num_region_points), stream)
    _lib.check(rc, "asep_gnn_forward_visual_batch_dev2")
    return pages


def gnn_forward_visual_batch_u8_dev(graph: GnnGraph, pages, scans, hs, ws, num_region_points, stream=None, device=0):
    """``asep_gnn_forward_visual_batch_u8_dev``: :func:`gnn_forward_visual_batch_dev2` fed with the scans as decoded.  ``scans[b]`` =
    (device address of the uint8 scan, H, W, C); all scans are resized to ``hs[b]`` x ``ws[b]`` in ONE launch
    (``asep_prep_resize_tf1_dev``'s bytes), ``d_image`` of the page dicts is not read."""
    lib = _lib.init_device(device)
    n = len(pages)
    if len(hs) != n or len(ws) != n or len(scans) != n:
        raise ValueError(f"{n} pages, {len(scans)} scans, {len(hs)} heights and {len(ws)} widths")
    arr = (_lib.GnnPageU8 * max(n, 1))()
    for q, d, (addr, H, W, Cn) in zip(arr, pages, scans):
        for k, v in d.items():
            setattr(q.page, k, v)
        q.d_scan, q.src_h, q.src_w, q.src_c = addr, int(H), int(W), int(Cn)
    Ints = C.c_int32 * max(n, 1)
    rc = lib.asep_gnn_forward_visual_batch_u8_dev(graph.handle(device), n, arr, Ints(*[int(v) for v in hs]), Ints(*[int(v) for v in ws]),
                                                  int(num_region_points), stream)
    _lib.check(rc, "asep_gnn_forward_visual_batch_u8_dev")
    return arr


def gnn_page_node_features(graph: GnnGraph, page, num_nodes, device=0):
    """node features [N, u] of page ``page`` of the last call over a page table (tests)"""
    lib = _lib.init_device(device)
    out = np.empty((int(num_nodes), graph.cfg.u_in_dim), dtype=np.float32)
    _lib.check(lib.asep_gnn_get_page_node_features(graph.handle(device), int(page), out.ctypes.data, out.size), "asep_gnn_get_page_node_features")
    return out


def _page_map(graph, fn_name, args, device):
    lib = _lib.init_device(device)
    fn = getattr(lib, fn_name)
    dims = (C.c_int32 * 3)()
    _lib.check(fn(graph.handle(device), *args, None, 0, dims), fn_name)
    out = np.empty((dims[0], dims[1], dims[2]), dtype=np.float32)
    _lib.check(fn(graph.handle(device), *args, out.ctypes.data, out.size, dims), fn_name)
    return out


def gnn_page_feature_map(graph: GnnGraph, page, index, device=0):
    """feature map ``index`` of page ``page`` of the last call over a page table as float32 [fh, fw, C] (tests)"""
    return _page_map(graph, "asep_gnn_get_page_feature_map", (int(page), int(index)), device)


def gnn_page_image(graph: GnnGraph, page, device=0):
    """the resized image [h, w, C] of page ``page`` of the last ``asep_gnn_forward_visual_batch_u8_dev`` call (tests)"""
    return _page_map(graph, "asep_gnn_get_page_image", (int(page),), device)


STEP_MODES = {0: "generic", 1: "mfma_registers", 2: "mfma_lds", 3: "factored"}


def step_mode(graph: GnnGraph, device=0) -> str:
    """which message-passing kernel the engine picked for this model (include/asep_hip.h asep_gnn_step_mode)"""
    lib = _lib.init_device(device)
    return STEP_MODES[_lib.check(lib.asep_gnn_step_mode(graph.handle(device)), "asep_gnn_step_mode")]


def gnn_node_features(graph: GnnGraph, num_nodes, device=0):
    """Concatenated [geometric | visual] node features of the last visual forward (tests)."""
    lib = _lib.init_device(device)
    out = np.empty((int(num_nodes), graph.cfg.u_in_dim), dtype=np.float32)
    _lib.check(lib.asep_gnn_get_node_features(graph.handle(device), out.ctypes.data, out.size),
               "asep_gnn_get_node_features")
    return out


def gnn_feature_map(graph: GnnGraph, index, device=0):
    """Feature map ``index`` of the last visual forward as float32 [fh, fw, C], generated or not (``asep_gnn_get_feature_map``; tests)."""
    lib = _lib.init_device(device)
    dims = (C.c_int32 * 3)()
    _lib.check(lib.asep_gnn_get_feature_map(graph.handle(device), int(index), None, 0, dims), "asep_gnn_get_feature_map")
    out = np.empty((dims[0], dims[1], dims[2]), dtype=np.float32)
    _lib.check(lib.asep_gnn_get_feature_map(graph.handle(device), int(index), out.ctypes.data, out.size, dims), "asep_gnn_get_feature_map")
    return out


def gnn_hidden(graph: GnnGraph, num_nodes, device=0):
    lib = _lib.init_device(device)
    out = np.empty((int(num_nodes), graph.cfg.hidden_dim), dtype=np.float32)
    _lib.check(lib.asep_gnn_get_hidden(graph.handle(device), out.ctypes.data, out.size), "asep_gnn_get_hidden")
    return out


def correct_edges(graph: GnnGraph, num_nodes, edges, edge_feat=None, device=0):
    """Device version of misc.py:7-151 -> (edges' [E',2] int32, features' [E',e] float32 or None)."""
    lib = _lib.init_device(device)
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    mult = 2 if graph.cfg.undirected_graph else 1
    out_e = np.empty((max(mult * E, 1), 2), dtype=np.int32)
    ed = graph.cfg.edge_feature_dim
    ef = out_f = None
    if edge_feat is not None and ed:
        ef = np.ascontiguousarray(edge_feat, dtype=np.float32).reshape(E, ed)
        out_f = np.empty((max(mult * E, 1), ed), dtype=np.float32)
    n = lib.asep_gnn_correct_edges(graph.handle(device), int(num_nodes), E, edges.ctypes.data if E else None,
                                   ef.ctypes.data if ef is not None and E else None, out_e.ctypes.data,
                                   out_f.ctypes.data if out_f is not None else None)
    _lib.check(n, "asep_gnn_correct_edges")
    return out_e[:n].copy(), (out_f[:n].copy() if out_f is not None else None)
