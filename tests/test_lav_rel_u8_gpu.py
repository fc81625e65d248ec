"""lav_rel on the visual net with host workers: under --device_resize the scans reach the GPU owner through DecodePool's slots and are
resized on the device; the evaluation must be the one of --device_resize False (the host resize), count for count and line for line."""
import json
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_NOT_RESULTS = ("Time:", "Using pb_path", "Saved", "No json")


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


@pytest.mark.parametrize("load_mode", ["L", "RGB"])
def test_visual_evaluation_with_host_workers_is_the_same_with_and_without_device_resize(load_mode, tmp_path):
    from citlab_article_separation_new_amd import synth
    N = 14
    argv = synth.write_gnn_cli_inputs(str(tmp_path), 3, visual=True, W=300, H=450, N=N, load_mode=load_mode)
    rng = np.random.default_rng(4)
    for k in range(3):
        jp = tmp_path / "data" / "json15d2bb" / f"p{k:03d}.json"
        d = json.loads(jp.read_text())
        member = rng.integers(-1, 3, size=N)
        gt = [[0, int(i), int(j)] for i in range(N) for j in range(N) if member[i] >= 0 and member[i] == member[j]]
        d["gt_relations"], d["gt_num_relations"] = gt, len(gt)
        jp.write_text(json.dumps(d))
    got = {}
    for flag in ("True", "False"):
        got[flag] = _evaluate(argv + ["--gpu_devices", "0", "--num_workers", "3", "--device_resize", flag])
    (dev, dev_lines), (host, host_lines) = got["True"], got["False"]
    assert dev.n == 3 * N * N and dev.n == host.n and dev.n_correct == host.n_correct and dev.a2 == host.a2
    assert np.array_equal(dev.thresholds.view(np.uint32), host.thresholds.view(np.uint32))
    assert np.array_equal(dev.tps, host.tps) and np.array_equal(dev.fps, host.fps)
    assert dev_lines == host_lines and "Evaluation finished." in dev_lines
