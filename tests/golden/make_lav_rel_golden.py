"""Golden of the relation net evaluation (tests/golden/lav_rel_golden.json), from the imported reference on the CPU.

The reference's article_separation/gnn/trainer/lav_rel.py is imported through ref_import.install_stubs() and its own
LavGNN.evaluate() runs on the recorded (targets, output) batches of lav_rel_cases.cases(): TensorFlow's session, graph and
dataset iterator, load_graph, InputGNN and the model class are recording stand-ins that hand evaluate() the batches one by
one and end the list the way tf.data does; sklearn computes the curves.  Stored per case: the log lines evaluate() wrote
(without the wall time), the arrays precision_recall_curve returned, the values of roc_auc_score and accuracy_score, and the
(fps, tps, thresholds) of sklearn's _binary_clf_curve as the precision-recall call saw them.  Stored once: the flag names and
defaults the reference's module defines, and the sklearn version (the yardstick: precision_recall_curve changed over the
years).

Run:  python tests/golden/make_lav_rel_golden.py
"""
import json
import logging
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.install_stubs()

import numpy as np  # noqa: E402
import sklearn  # noqa: E402
import sklearn.metrics._ranking as ranking  # noqa: E402
import tensorflow as tf  # noqa: E402  (the stub)

import lav_rel_cases as lc  # noqa: E402


class EndOfData(Exception):
    pass


class Tensor:
    def __init__(self, name):
        self.name = name


class Graph:
    def as_default(self):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def get_tensor_by_name(self, name):
        return Tensor(name)


class Session:
    """sess.run([next_batch]) -> the next recorded batch (or the end of the data); sess.run(output_nodes, feed_dict) -> its output"""
    batches = []

    def __init__(self, graph=None, config=None):
        self.graph = graph
        self.at = -1

    def run(self, fetches, feed_dict=None):
        if feed_dict is None:
            self.at += 1
            if self.at >= len(Session.batches):
                raise EndOfData()
            targets, _ = Session.batches[self.at]
            return [({}, {"relations_to_consider_gt": targets})]
        return [Session.batches[self.at][1]]


class Model:
    def get_placeholder(self):
        return {}

    def get_output_nodes(self, has_graph=False):
        return "output_belong_to_same_instance"

    def get_target_keys(self):
        return "relations_to_consider_gt"

    def print_evaluate_summary(self):
        pass


class Input:
    def get_eval_dataset(self):
        return None


class Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def main():
    import importlib
    importlib.import_module("tensorflow.errors").OutOfRangeError = EndOfData     # (imported: an attribute of the stub is a fresh
    importlib.import_module("tensorflow.compat.v1").Session = Session            # placeholder on every access, a submodule stays)
    tf.Graph = Graph
    # the model class and the input pipeline are TensorFlow (and TensorBoard) code: stand-in modules take their place
    model_mod = types.ModuleType("article_separation.gnn.model.model_relation")
    model_mod.ModelRelation = lambda params: Model()
    input_mod = types.ModuleType("article_separation.gnn.input.input_dataset")
    input_mod.InputGNN = lambda flags: Input()
    for mod in (model_mod, input_mod):
        parent, _, leaf = mod.__name__.rpartition(".")
        sys.modules[mod.__name__] = mod
        setattr(importlib.import_module(parent), leaf, mod)
    saved = sys.argv
    sys.argv = ["lav_rel.py"]
    try:
        from article_separation.gnn.trainer import lav_rel as ref
        import python_util.basic.flags as rflags
    finally:
        sys.argv = saved
    names = ("model_dir", "model_type", "eval_list", "num_classes", "num_relation_components", "sample_num_relations_to_consider",
             "sample_relations", "image_input", "assign_visual_features_to_nodes", "assign_visual_features_to_edges", "backbone", "mvn",
             "graph_backbone_params", "feature_map_generation_params", "input_params", "num_p_r_thresholds", "gpu_devices",
             "gpu_memory_fraction", "batch_limiter", "try_gpu")
    defaults = {a.dest: a.default for a in rflags.global_parser._actions if a.dest in names}
    assert set(defaults) == set(names), sorted(set(names) - set(defaults))
    ref.load_graph = lambda path: Graph()
    recorded = {}

    def recording(fn, key):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            recorded.setdefault(key, out)
            return out
        return wrapped

    ref.precision_recall_curve = recording(ref.precision_recall_curve, "prc")
    ref.roc_auc_score = recording(ref.roc_auc_score, "auc")
    ref.accuracy_score = recording(ref.accuracy_score, "acc")
    ranking._binary_clf_curve = recording(ranking._binary_clf_curve, "clf")
    cap = Capture()
    logging.getLogger().addHandler(cap)
    logging.getLogger().setLevel("INFO")
    out_cases = []
    for case in lc.cases():
        recorded.clear()
        cap.lines.clear()
        Session.batches = case["pages"]
        lav = object.__new__(ref.LavGNN)
        lav._flags = types.SimpleNamespace(gpu_devices=[], gpu_memory_fraction=0.95, assign_visual_features_to_nodes=True,
                                           assign_visual_features_to_edges=False, **case["flags"])
        lav._pb_path, lav._model, lav._input_fn_generator = "net.pb", Model(), Input()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lav.evaluate()
        lines = [ln for ln in cap.lines if not ln.startswith("Time: ")]
        prec, rec, thr = recorded["prc"]
        fps, tps, thr_desc = recorded["clf"]
        assert thr.dtype == np.float32 and prec.dtype == np.float64, (thr.dtype, prec.dtype)
        y, p = lc.concatenated(case)
        out_cases.append({
            "name": case["name"], "flags": case["flags"], "n_pairs": int(len(y)), "log": lines,
            "warnings": sorted({str(w.message) for w in caught}),
            "precision": [float(v) for v in prec], "recall": [float(v) for v in rec], "thresholds": [float(v) for v in thr],
            "fps": [int(v) for v in fps], "tps": [int(v) for v in tps], "thresholds_desc": [float(v) for v in thr_desc],
            "auc_roc": float(recorded["auc"]), "accuracy": float(recorded["acc"]),
            "n_correct": int(np.sum((p > 0.5) == (y != 0)))})
    logging.getLogger().removeHandler(cap)
    out = {"sklearn": sklearn.__version__, "numpy": np.__version__, "flags": {k: defaults[k] for k in names}, "cases": out_cases}
    path = os.path.join(HERE, "lav_rel_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes;", len(out_cases), "cases, sklearn", sklearn.__version__)


if __name__ == "__main__":
    main()
