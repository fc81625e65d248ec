"""Golden of the RU_v2 graph's WIRING (tests/golden/model_wiring_ru_v2.npz): the reference's own ``backbones/RU_v2.py``, executed.

As make_model_wiring_golden.py does for ARU_v1.py: the reference's module is imported through ref_import.install_stubs() with
tf_eager_standin.py in the place of ``tensorflow`` (float64), ``RU_v2_CNN.infer`` runs on a small page, and every variable the reference's code
asks for gets its value from model_wiring_cases.variable_value(name, shape).

Stored per case: the page, the (name, shape) list in creation order and the logits -- RU_v2_CNN.infer returns no end points (RU_v2.py:31), and
every weight of the graph feeds the logits.  float32 arrays in a zip of .npy members with fixed time stamps, so that

    python tests/golden/make_ru_v2_golden.py --check

regenerates the file in memory and compares it with the committed one byte for byte.

Run:  python tests/golden/make_ru_v2_golden.py [--check]
"""
import importlib
import logging
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_model_wiring_golden as base  # noqa: E402  (installs ref_import's stubs and the TensorFlow stand-in)
import model_wiring_cases as mc  # noqa: E402

import numpy as np  # noqa: E402

tf = base.tf
standin = base.standin
FILE = "model_wiring_ru_v2.npz"

# cfg: keyword arguments of AruConfig(graph="RU_v2", ...).  37 x 53 -> 19 x 27 -> 10 x 14 -> 5 x 7 -> 3 x 4: odd sizes at every level, so every
# average pool of the pyramid has partial windows at both borders.  Small widths except in the default case (the fixture stores no weights).
CASES = [
    {"name": "ru_v2_defaults", "hw": (37, 53), "cfg": {}},
    {"name": "ru_v2_no_inp4up", "hw": (13, 22), "cfg": {"inp4up": False, "feat_root": 4}},
    {"name": "ru_v2_mvn", "hw": (16, 9), "cfg": {"mvn": True, "feat_root": 4}},
    {"name": "ru_v2_rgb", "hw": (13, 22), "cfg": {"channels": 3, "feat_root": 4}},
    {"name": "ru_v2_res_depth1_scale_space3", "hw": (16, 9), "cfg": {"res_depth": 1, "scale_space_num": 3, "feat_root": 4}},
    {"name": "ru_v2_elu", "hw": (13, 22), "cfg": {"activation_name": "elu", "feat_root": 4}},
    {"name": "ru_v2_leaky_rgb_no_inp4up", "hw": (16, 9), "cfg": {"activation_name": "leaky", "channels": 3, "inp4up": False, "feat_root": 4,
                                                               "n_classes": 3}},
]


def run_case(RU2, case):
    cfg = case["cfg"]
    backbone = {}
    for ours, theirs in (("mvn", "mvn"), ("inp4up", "inp4up"), ("feat_root", "featRoot"), ("scale_space_num", "scale_space_num"),
                         ("res_depth", "res_depth"), ("activation_name", "activation_name")):
        if ours in cfg:
            backbone[theirs] = cfg[ours]
    flags = types.SimpleNamespace(graph_backbone_params=backbone, channels=cfg.get("channels", 1), n_classes=cfg.get("n_classes", 2))
    image = mc.aru_image(case)
    src = base.Source()
    standin.VARIABLES.reset(src)
    net = RU2({"flags": flags})
    logits, end_points = net.infer(tf.Tensor(image[None].astype(np.float64)), is_training=False)
    assert end_points == {}, "RU_v2_CNN.infer returns no end points"
    names = [[k, [int(s) for s in v.shape]] for k, v in standin.VARIABLES.created.items()]
    return {"image": image, "logits": logits.numpy()[0].astype(np.float32)}, names


def generate():
    standin.self_check()
    base.import_reference()                                       # the module aliases RU_v2.py imports its siblings under
    RU2 = importlib.import_module("article_separation.backbones.RU_v2").RU_v2_CNN
    arrays, meta = {}, {"cases": []}
    for case in CASES:
        out, names = run_case(RU2, case)
        arrays.update({f"{case['name']}::{k}": v for k, v in out.items()})
        meta["cases"].append({"name": case["name"], "hw": list(case["hw"]), "cfg": case["cfg"], "variables": names})
    standin.VARIABLES.reset(None)
    return base.pack(arrays, meta)


def main():
    logging.getLogger().setLevel("ERROR")
    check = "--check" in sys.argv[1:]
    data = generate()
    path = os.path.join(HERE, FILE)
    if len(data) >= base.SIZE_LIMIT:
        raise SystemExit(f"{FILE}: {len(data)} bytes, the limit is {base.SIZE_LIMIT}")
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
