"""Golden of the segmentation net evaluation (tests/golden/seg_eval_golden.npz), from the imported reference on the CPU.

article_separation/plot_net_output.py is imported with placeholder modules for tensorflow, cv2 and matplotlib; its own
compute_accuracy, apply_mask and plot_image_with_net_output run on the small arrays of seg_eval_cases below:

  acc_<case>_<cl>     compute_accuracy(one-hot arg max of class cl, gt_cl / 255) as :241 calls it.  The one-hot planes are built
                      with the reference's own loop (:216-226), restated here because it sits inside plot_net_output;
  blend_<case>        plot_image_with_net_output(scan.astype(uint32), mask) as :245 calls it, then uint8 as :253 writes it;
  blend8_<case>       the same on the uint8 scan itself, in place, as :249 calls it for the ground truth side;
  flags               the arguments of the reference's ArgumentParser (:287-298), read off its source: name, type, default, action.

The inputs are stored next to the results, so the test needs neither this script nor the reference.  Data only.

Run:  python tests/golden/make_seg_eval_golden.py
"""
import ast
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

if "matplotlib" not in ref_import.STUBBED:
    ref_import.STUBBED = tuple(ref_import.STUBBED) + ("matplotlib",)
ref_import.install_stubs()

from article_separation import plot_net_output as ref  # noqa: E402


def prob_cases():
    """name -> (probabilities float32 [H,W,C], ground truth uint8 [C,H,W], thresholded?)"""
    rng = np.random.default_rng(20240611)
    cases = {}
    special = np.array([0.0, 1.0, 0.6, np.float32(0.6), np.nextafter(np.float32(0.6), np.float32(1)), 0.59999, 0.5, 0.25, 0.75,
                        1e-30, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    for name, (H, W, C) in {"a": (5, 7, 2), "b": (3, 9, 3), "c": (4, 4, 1), "d": (2, 11, 5)}.items():
        p = special[rng.integers(0, len(special), size=(H, W, C))]
        p[0, 0, :] = 0.5                                            # a tie of every class
        if C > 1:
            p[0, 1, :] = 0.0
            p[0, 1, C - 1] = p[0, 1, C - 2] = 1.0                   # a tie of the last two
        gt = np.array([0, 255, 128, 1, 254], np.uint8)[rng.integers(0, 5, size=(C, H, W))]
        gt[:, 0, :3] = np.array([0, 255, 128], np.uint8)
        for thr in (False, True):
            cases[name + ("_thr" if thr else "")] = (p.copy(), gt.copy(), thr)
    return cases


def blend_cases():
    """name -> (scan uint8 [H,W,3], mask uint8 [H,W])"""
    rng = np.random.default_rng(77)
    cases = {}
    for name, (H, W) in {"p1": (1, 1), "p2": (2, 9), "p3": (6, 5)}.items():
        scan = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
        scan.reshape(-1)[::5] = 0
        scan.reshape(-1)[1::7] = 255
        mask = np.array([0, 255, 254, 128, 1], np.uint8)[rng.integers(0, 5, size=(H, W))]
        cases[name] = (scan, mask)
    cases["all0"] = (cases["p3"][0].copy(), np.zeros((6, 5), np.uint8))
    cases["all255"] = (cases["p3"][0].copy(), np.full((6, 5), 255, np.uint8))
    cases["white"] = (np.full((2, 3, 3), 255, np.uint8), np.full((2, 3), 255, np.uint8))
    cases["black"] = (np.zeros((2, 3, 3), np.uint8), np.full((2, 3), 255, np.uint8))
    return cases


def one_hot_like_the_reference(out_img):
    """:216-226 on a [1,H,W,C] array"""
    values = np.argmax(out_img, axis=3)
    one_hot = np.zeros_like(out_img)
    for i in range(out_img.shape[0]):
        for j in range(out_img.shape[1]):
            for k in range(out_img.shape[2]):
                one_hot[i, j, k, values[i, j, k]] = 1
    return one_hot


def parser_flags():
    tree = ast.parse(open(ref.__file__).read())
    flags = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            entry = {"name": ast.literal_eval(node.args[0]), "type": None, "default": None, "action": None}
            for kw in node.keywords:
                if kw.arg == "type":
                    entry["type"] = kw.value.id
                elif kw.arg in ("default", "action"):
                    entry[kw.arg] = ast.literal_eval(kw.value)
            flags.append(entry)
    return flags


def main():
    out = {}
    for name, (p, gt, thr) in prob_cases().items():
        out[f"prob_{name}"], out[f"gt_{name}"] = p, gt
        out_img = p[None]
        if thr:
            out_img = np.array((out_img > 0.6), np.int32)           # :202
        one_hot = one_hot_like_the_reference(out_img)
        for cl in range(p.shape[2]):
            out[f"acc_{name}_{cl}"] = np.float64(ref.compute_accuracy(one_hot[0, :, :, cl], gt[cl] / 255))
    for name, (scan, mask) in blend_cases().items():
        out[f"scan_{name}"], out[f"mask_{name}"] = scan, mask
        with contextlib.redirect_stdout(io.StringIO()):              # (plot_image_with_net_output prints its random colours)
            out[f"blend_{name}"] = np.uint8(ref.plot_image_with_net_output(scan.astype(np.uint32), mask))
            inplace = scan.copy()
            res = ref.plot_image_with_net_output(inplace, mask)
        assert res is inplace and res.dtype == np.uint8
        out[f"blend8_{name}"] = inplace
    out["flags"] = np.array(json.dumps(parser_flags()))
    path = os.path.join(HERE, "seg_eval_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
