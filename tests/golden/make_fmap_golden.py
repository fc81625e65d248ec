"""Golden of the relation net's feature-map generator (tests/golden/fmap_golden.npz): the reference's own
``multi_resolution_feature_maps`` (gnn/model/graph_util/feature_map_generators.py:72-197), executed as graph_relation.py:100-104 calls it
(``insert_1x1_conv=True``), with tf_eager_standin.py in the place of ``tensorflow`` (ref_import.install_stubs(), like
make_model_wiring_golden.py).

Inputs: a dict of small random "end points" A and B (CASES below); every variable the reference asks for gets its value from
model_wiring_cases.variable_value(name, shape).  The reference passes ``filters=layer_depth / 2`` -- a float -- into the kernel's shape
(layers.py:220); the stand-in's get_variable takes whole numbers, so the source handed to it here turns a whole-valued float dimension
into the int it stands for.  That is the only adaptation, and it is made here, not in the stand-in.

Stored per case: the end points, the (name, shape) list in creation order, every variable's value, every returned map (``map::<i>``)
and the returned dict's keys in order.  float32 / int32, fixed time stamps:

    python tests/golden/make_fmap_golden.py --check

regenerates the file in memory and compares with the committed one byte for byte (exit 0), exit 3 when the reference is not importable.
"""
import logging
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import model_wiring_cases as mc  # noqa: E402

FILE = "fmap_golden.npz"

# end points: 7 x 10 and 6 x 9 maps, so that even and odd sides occur in both axes of the strided convolutions
END_POINTS = {"A": (7, 10, 5), "B": (6, 9, 3)}
CASES = [
    {"name": "chain", "hw": "7x10", "from_layer": ["A", "A", "", ""], "layer_depth": [-1, 6, 8, 2]},
    {"name": "two_bases", "hw": "6x9", "from_layer": ["A", "B", ""], "layer_depth": [12, -1, 4]},
    {"name": "one_extra", "hw": "7x10", "from_layer": ["A", ""], "layer_depth": [-1, 16]},
]
# the three cases once more on the other map size
CASES = CASES + [dict(c, name=c["name"] + "_swapped", hw="6x9" if c["hw"] == "7x10" else "7x10") for c in CASES]


def end_points(case):
    """A and B of a case: both of the case's spatial size (one backbone level), values in -1 .. 1"""
    h, w = (int(v) for v in case["hw"].split("x"))
    out = {}
    for k, (_, _, c) in END_POINTS.items():
        out[k] = (mc.uniform(f"fmap:{case['name']}:{k}", h * w * c) * 2 - 1).reshape(h, w, c).astype(np.float32)
    return out


def _whole(shape):
    out = []
    for s in (shape if isinstance(shape, (list, tuple)) else [shape]):
        if float(s) != int(s):
            raise ValueError(f"variable shape {shape}: not whole")
        out.append(int(s))
    return out


def generate():
    import ref_import
    import tf_eager_standin as standin
    from make_model_wiring_golden import pack          # (installs the stubs and the stand-in on import)
    ref_import.install_stubs()
    tf = standin.install()
    standin.self_check()
    saved = sys.argv
    sys.argv = ["make_fmap_golden.py"]
    try:
        from article_separation.gnn.model.graph_util import feature_map_generators as fmg
    finally:
        sys.argv = saved

    class Source:
        def __init__(self):
            self.values = {}

        def __call__(self, name, shape):
            if name not in self.values:
                self.values[name] = mc.variable_value(name, _whole(shape))
            return self.values[name].astype(np.float64)

    # layers.conv2d hands [kh, kw, Cin, layer_depth / 2] to get_variable: whole-valued floats become the ints they stand for
    real_get = tf.compat.v1.get_variable

    def get_variable(name, shape=None, *a, **k):
        return real_get(name, _whole(shape) if shape is not None else None, *a, **k)
    tf.compat.v1.get_variable = get_variable
    try:
        arrays, meta = {}, {"cases": []}
        for case in CASES:
            src = Source()
            standin.VARIABLES.reset(src)
            eps = end_points(case)
            feats = {k: tf.Tensor(v[None].astype(np.float64)) for k, v in eps.items()}
            layout = {"from_layer": list(case["from_layer"]), "layer_depth": list(case["layer_depth"])}
            maps = fmg.multi_resolution_feature_maps(feature_map_layout=layout, is_training=False, insert_1x1_conv=True,
                                                     image_features=feats)
            # the returned OrderedDict is keyed by name: a repeated from_layer would collapse there; graph_relation.py uses .values()
            keys = list(maps.keys())
            for k, v in eps.items():
                arrays[f"{case['name']}::ep::{k}"] = v
            for i, v in enumerate(maps.values()):
                assert v.numpy().shape[0] == 1
                arrays[f"{case['name']}::map::{i}"] = v.numpy()[0].astype(np.float32)
            names = [[k, _whole(list(v.shape))] for k, v in standin.VARIABLES.created.items()]
            for k, _ in names:
                arrays[f"{case['name']}::var::{k}"] = src.values[k]
            meta["cases"].append({"name": case["name"], "hw": case["hw"], "from_layer": case["from_layer"], "layer_depth": case["layer_depth"],
                                  "variables": names, "keys": keys})
    finally:
        tf.compat.v1.get_variable = real_get
        standin.VARIABLES.reset(None)
    return pack(arrays, meta)


def main():
    logging.getLogger().setLevel("ERROR")
    check = "--check" in sys.argv[1:]
    try:
        data = generate()
    except ImportError as e:
        print(f"the reference is not importable here: {e}")
        sys.exit(3)
    limit = os.path.getsize(os.path.join(HERE, "host_goldens.json"))
    if len(data) >= limit:
        raise SystemExit(f"{FILE}: {len(data)} bytes, the limit is {limit}")
    path = os.path.join(HERE, FILE)
    if check:
        with open(path, "rb") as f:
            same = f.read() == data
        print(f"{FILE}: {'reproduced byte for byte' if same else 'DIFFERS'} ({len(data)} bytes)")
        sys.exit(0 if same else 1)
    with open(path, "wb") as f:
        f.write(data)
    print(path, len(data), "bytes")


if __name__ == "__main__":
    main()
