"""numpy restatement of the relation net's feature-map generator (feature_map_generators.py:72-197 with insert_1x1_conv=True, the form
graph_relation.py:100-104 builds) and of the visual forward over those maps.  Pinned by tests/golden/fmap_golden.npz
(tests/test_fmap_host.py); the GPU tests compare the engine with it.  The graph itself stays oracle/gnn_oracle.py: imported, not copied."""
import numpy as np


def same_pad(n, k, stride):
    """TensorFlow SAME along one axis: (output size, padding in front, padding behind); the smaller half goes in front"""
    out = -(-n // stride)
    total = max((out - 1) * stride + k - n, 0)
    return out, total // 2, total - total // 2


def conv2d_same(x, w, b, stride, dtype=np.float64):
    """layers.conv2d (layers.py:191-247) at its defaults: SAME padding, bias, ReLU.  x [h, w, Ci], w [k, k, Ci, Co], b [Co]"""
    x, w, b = np.asarray(x, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    k = w.shape[0]
    oh, pt, pb = same_pad(x.shape[0], k, stride)
    ow, pl, pr = same_pad(x.shape[1], k, stride)
    xp = np.pad(x, ((pt, pb), (pl, pr), (0, 0)))
    out = np.zeros((oh, ow, w.shape[3]), dtype)
    for ky in range(k):
        for kx in range(k):
            tap = xp[ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride]
            out += tap @ w[ky, kx]
    return np.maximum(out + b, 0).astype(dtype)


def variable_names(layers, depths):
    """the generator's variable scopes per generated map, as the reference's f-strings spell them: [(index, conv1 scope, conv2 scope)];
    ``layer_depth / 2`` is Python's true division (a float) and the base is the last from_layer that had depth -1"""
    out, base = [], ""
    for i, (name, d) in enumerate(zip(layers, depths)):
        if name and d == -1:
            base = name
            continue
        out.append((i, f"{base}_1_Conv2d_{i}_1x1_{d / 2}", f"{base}_2_Conv2d_{i}_3x3_s2_{d}"))
    return out


def variable_shapes(end_point_channels, layers, depths):
    """[(name, shape)] in the reference's creation order"""
    out, chans = [], []
    scopes = {i: (a, b) for i, a, b in variable_names(layers, depths)}
    for i, (name, d) in enumerate(zip(layers, depths)):
        if name and d == -1:
            chans.append(end_point_channels[name])
            continue
        cin = end_point_channels[name] if name else chans[-1]
        s1, s2 = scopes[i]
        out += [(s1 + "/weights", [1, 1, cin, d // 2]), (s1 + "/biases", [d // 2]), (s2 + "/weights", [3, 3, d // 2, d]), (s2 + "/biases", [d])]
        chans.append(d)
    return out


def generated_maps(end_points, layers, depths, w, dtype=np.float64):
    """every feature map of the layout, in order: end_points name -> [h, w, C]; w name -> array"""
    maps = []
    scopes = {i: (a, b) for i, a, b in variable_names(layers, depths)}
    for i, (name, d) in enumerate(zip(layers, depths)):
        if name and d == -1:
            maps.append(np.asarray(end_points[name], dtype))
            continue
        if not name and not maps:
            raise ValueError("an empty from_layer in position 0")
        pre, stride = (end_points[name], 1) if name else (maps[-1], 2)
        s1, s2 = scopes[i]
        mid = conv2d_same(pre, w[s1 + "/weights"], w[s1 + "/biases"], 1, dtype)
        maps.append(conv2d_same(mid, w[s2 + "/weights"], w[s2 + "/biases"], stride, dtype))
    return maps


def roi_features(maps, regions, num_points, w, scope_kind="node"):
    """oracle.gnn_oracle.visual_node_features' ROI max + compression (misc.py:322-368), over the given maps -> [N, sum dims] float32"""
    regions = np.asarray(regions, dtype=np.float32)
    N = regions.shape[0]
    feats = []
    for i, fm in enumerate(maps):
        fm = np.asarray(fm, np.float32)
        fh, fw, _ = fm.shape
        vmax = np.empty((N, fm.shape[2]), dtype=np.float32)
        for n in range(N):
            k = int(num_points[n])
            if k == 0:
                xmin = xmax = ymin = ymax = np.float32(0)
            else:
                xmin, xmax = regions[n, 0, :k].min(), regions[n, 0, :k].max()
                ymin, ymax = regions[n, 1, :k].min(), regions[n, 1, :k].max()
            x0 = max(min(int(np.floor(np.float32(xmin) * np.float32(fw))), fw - 1), 0)
            x1 = max(min(int(np.floor(np.float32(xmax) * np.float32(fw))), fw - 1), 0)
            y0 = max(min(int(np.floor(np.float32(ymin) * np.float32(fh))), fh - 1), 0)
            y1 = max(min(int(np.floor(np.float32(ymax) * np.float32(fh))), fh - 1), 0)
            nx, ny = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
            vmax[n] = fm[y0:y0 + ny, x0:x0 + nx].max(axis=(0, 1))
        scope = f"visual_{scope_kind}_feature_compression_fm_{i}/dense"
        feats.append(np.maximum(vmax @ w[scope + "/weights"].astype(np.float32) + w[scope + "/bias"].astype(np.float32), 0).astype(np.float32))
    return np.concatenate(feats, axis=1)


def backbone_end_points(image, w, cfg):
    """the ARU_v1 backbone's end points of the page (oracle.aru_oracle, fp32)"""
    from oracle import aru_oracle
    img = np.asarray(image, dtype=np.float32)
    if img.ndim == 3:
        img = img[:, :, 0]
    _, inter = aru_oracle.forward_torch(img, {k: v for k, v in w.items() if k.startswith("aru_net/")}, cfg.backbone_cfg(), return_intermediates=True)
    return inter


def forward_visual_maps(num_nodes, edges, node_feat, edge_feat, image, regions, num_points, relations, w, cfg, edge_regions=None,
                        edge_num_points=None):
    """oracle.gnn_oracle.forward_visual with the layout's generated maps in the place of the plain end points -> (probs, u)"""
    from oracle import gnn_oracle
    N = int(num_nodes)
    maps = [m.astype(np.float32) for m in generated_maps(backbone_end_points(image, w, cfg), cfg.visual_layers, cfg.layer_depths(), w)]
    vis = roi_features(maps, regions, num_points, w)
    geo = np.asarray(node_feat, dtype=np.float32).reshape(N, -1) if node_feat is not None else np.zeros((N, 0), np.float32)
    u = np.concatenate([geo, vis], axis=1)
    if getattr(cfg, "visual_edges", False):
        E = np.asarray(edges).reshape(-1, 2).shape[0]
        evis = roi_features(maps, edge_regions, edge_num_points, w, scope_kind="edge")
        egeo = np.asarray(edge_feat, dtype=np.float32).reshape(E, -1) if edge_feat is not None else np.zeros((E, 0), np.float32)
        edge_feat = np.concatenate([egeo, evis], axis=1)
    return gnn_oracle.forward(N, edges, u, edge_feat, relations, w, cfg), u
