"""--pages_per_call of run_gnn_clustering and lav_rel on the visual net: pages of three image sizes collected into one engine call
(asep_gnn_forward_visual_batch_dev2) must leave the files and the evaluation of the page-by-page run, byte for byte.  Five pages with
three per call: one full call and a tail of two, which has to be flushed after the loop.  The owner with host workers (--num_workers 3:
gnn_clustering_pipelined, scans through decode slots under --device_resize) is held to the same bytes; lav_rel with four per call leaves a tail of
one, which under --device_resize goes through the u8 entry alone.

The only bytes of a written PAGE-XML that depend on the clock are the text of its ``LastChange`` element: blanked before comparing."""
import json
import logging
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 14
SCANS = [(450, 300), (300, 420), (380, 380)]                          # H x W: three aspect ratios -> three sizes after the resize
_NOT_RESULTS = ("Time:", "Using pb_path", "Saved", "No json")


def _inputs(root, n_pages=5):
    """synth.write_gnn_cli_inputs, then the scans replaced by scans of the sizes above (page k: SCANS[k % 3]) and planted ground truth"""
    from PIL import Image
    from citlab_article_separation_new_amd import gnn_input, synth
    argv = synth.write_gnn_cli_inputs(str(root), n_pages, visual=True, W=300, H=450, N=N)
    rng = np.random.default_rng(4)
    data = root / "data"
    sizes = set()
    for k in range(n_pages):
        png, jp = data / f"p{k:03d}.png", data / "json15d2bb" / f"p{k:03d}.json"
        H, W = SCANS[k % 3]
        d = json.loads(jp.read_text())
        if png.is_symlink():
            png.unlink()
        if jp.is_symlink():
            jp.unlink()
        Image.fromarray(synth.synth_page(50 + k, W=W, H=H).astype(np.uint8)).save(str(png), compress_level=1)
        member = rng.integers(-1, 3, size=N)
        gt = [[0, int(i), int(j)] for i in range(N) for j in range(N) if member[i] >= 0 and member[i] == member[j]]
        d["gt_relations"], d["gt_num_relations"] = gt, len(gt)
        jp.write_text(json.dumps(d))
        sizes.add(gnn_input.compute_new_size(H, W, 256, 1024))
    assert len(sizes) == 3, sizes
    return argv + ["--gpu_devices", "0"]


def _files(root, out_dir):
    found = {}
    for top in (root / out_dir, root / "data" / "confidences"):
        for dirpath, _, names in os.walk(top):
            for n in names:
                p = os.path.join(dirpath, n)
                with open(p, "rb") as f:
                    raw = f.read()
                if n.endswith(".xml"):
                    raw = re.sub(rb"(<(?:\w+:)?LastChange>)[^<]*(</)", rb"\1\2", raw)
                found[os.path.relpath(p, top)] = raw
    return found


@pytest.mark.parametrize("extra", [(), ("--device_resize", "True"), ("--num_workers", "3"), ("--num_workers", "3", "--device_resize", "True")],
                         ids=["host_resize", "device_resize", "pipelined_host_resize", "pipelined_device_resize"])
def test_run_gnn_clustering_three_pages_per_call_writes_the_bytes_of_page_by_page(extra, tmp_path):
    from citlab_article_separation_new_amd import run_gnn_clustering
    argv = _inputs(tmp_path) + ["--save_conf", "with_conf", *extra]
    cwd = os.getcwd()
    os.chdir(tmp_path)
    got = {}
    try:
        for n in ("1", "3"):
            conf = tmp_path / "data" / "confidences"
            for f in conf.glob("*.json") if conf.is_dir() else ():
                f.unlink()
            outs = run_gnn_clustering.main(argv + ["--out_dir", "out_" + n, "--pages_per_call", n])
            assert len(outs) == 5
            got[n] = _files(tmp_path, "out_" + n)
    finally:
        os.chdir(cwd)
    assert sorted(got["1"]) == sorted(got["3"])
    assert sum(k.endswith("_clustering.xml") for k in got["3"]) == 5 and sum(k.endswith("_confidences.json") for k in got["3"]) == 5
    for k in got["1"]:
        assert got["1"][k] == got["3"][k], k


class _Capture(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _evaluate(argv):
    from citlab_article_separation_new_amd import lav_rel
    cap = _Capture()
    root = logging.getLogger()
    level = root.level
    root.addHandler(cap)
    root.setLevel(logging.INFO)
    try:
        curve = lav_rel.LavGNN(argv=argv).evaluate()
    finally:
        root.removeHandler(cap)
        root.setLevel(level)
    return curve, [ln for ln in cap.lines if not ln.startswith(_NOT_RESULTS)]


@pytest.mark.parametrize("extra", [(), ("--device_resize", "True")], ids=["host_resize", "device_resize"])
def test_lav_rel_four_pages_per_call_gives_the_tables_and_auc_of_page_by_page(extra, tmp_path):
    argv = _inputs(tmp_path) + list(extra)
    (one, one_lines), (four, four_lines) = (_evaluate(argv + ["--pages_per_call", n]) for n in ("1", "4"))
    assert one.n == 5 * N * N and four.n == one.n and four.n_correct == one.n_correct and four.a2 == one.a2
    assert np.array_equal(four.thresholds.view(np.uint32), one.thresholds.view(np.uint32))
    assert np.array_equal(four.tps, one.tps) and np.array_equal(four.fps, one.fps)
    assert four.auc_roc == one.auc_roc and np.isfinite(one.auc_roc)
    assert four_lines == one_lines and "Evaluation finished." in four_lines
