"""The f32s level-0 DOWN strip walker (res8ws_kernel<false>, csrc/res8ws_kernels.h) after its raw-t ring left LDS: the walker recomputes conv1
for the rows that stage 3 finishes, out of an image ring of sixteen rows, and runs eight waves per CU.

  * same results as the other implementation (ASEP_SPLIT_WALK=0, res8v_down_kernel) at the 1e-5 gate of tests/test_split_walk_gpu.py: the
    block's output d0 and its 2 x 2 pool, on the cases of tests/split_walk_down_cases.py (smallest walking page, odd sizes, a band seam inside
    the page, a mixed batch of five pages, with and without per-page standardisation, large values at the border and at the bands' first rows);
  * bit-identical to the walker of the parent commit: tests/golden/split_walk_down_golden.json holds float64 sums and CRC-32 of d0 and of the
    level-1 block's output (a function of the pool alone), recorded there by tests/golden/make_split_walk_down_golden.py; the pool itself is
    held to max-pooling the identical d0, which is exact;
  * the runtime keeps eight DOWN walker blocks on a CU, and four UP ones as before."""
import json
import os

import numpy as np
import pytest

import split_walk_down_cases as sc

pytestmark = pytest.mark.gpu

FORM_GATE = 1e-5                # walker against res8v (max |d| / max(1, max |ref|)), the gate of tests/test_split_walk_gpu.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_walk_down_golden.json")

_results = {}


def _both(case, monkeypatch):
    """the end points of a case on the walker ("1") and on res8v ("0"), computed once per session and left unchanged"""
    name, pages, kind, mvn = case
    if name not in _results:
        _results[name] = {f: sc.run(pages, kind, mvn, f, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False)) for f in ("1", "0")}
    return _results[name]


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))


def _maxpool2(d):
    """2 x 2 max pool of [H, W, C] with partial last row / column (the values are ReLU outputs: >= 0)"""
    H, W, C = d.shape
    p = np.zeros((2 * ((H + 1) // 2), 2 * ((W + 1) // 2), C), np.float32)
    p[:H, :W] = d
    return p.reshape((H + 1) // 2, 2, (W + 1) // 2, 2, C).max(axis=(1, 3))


def _num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_walker_matches_vector_alu_form(case, monkeypatch):
    name, pages, kind, mvn = case
    res = _both(case, monkeypatch)
    walks = [sc.walk_region(*s)[2] for s in pages]
    assert any(walks)
    assert sc.POOL in res["1"] and sc.POOL in res["0"]
    for b, (H, W) in enumerate(pages):
        d1, d0 = res["1"][sc.D0][b], res["0"][sc.D0][b]
        p1, p0 = res["1"][sc.POOL][b], res["0"][sc.POOL][b]
        assert d1.shape == d0.shape == (H, W, 8) and p1.shape == p0.shape == ((H + 1) // 2, (W + 1) // 2, 8)
        if walks[b]:
            assert not np.array_equal(d1, d0), (name, b)          # another arithmetic: the walker ran
        else:
            assert np.array_equal(d1, d0) and np.array_equal(p1, p0), (name, b)
        print(name, b, "d0", _rel(d1, d0), "pool", _rel(p1, p0))
        assert _rel(d1, d0) <= FORM_GATE, (name, b, _rel(d1, d0))
        assert _rel(p1, p0) <= FORM_GATE, (name, b, _rel(p1, p0))
        assert _rel(res["1"][sc.D1][b], res["0"][sc.D1][b]) <= FORM_GATE, (name, b)
        # the pool is the exact maximum of the block's own output, partial last row and column included
        assert np.array_equal(p1, _maxpool2(d1)), (name, b)


def test_seam_page_has_two_bands():
    """the page of the seam cases is cut into at least two bands by the launcher's rule, and an item's image rows wrap the ring more than once"""
    n_strips, rows, fits = sc.walk_region(*sc.SEAM_PAGE)
    assert fits and rows >= 2 * 32 + 20
    band = sc.walk_band([sc.SEAM_PAGE], _num_cus(), 8)
    assert -(-rows // band) >= 2
    assert min(band, rows) + 8 > 2 * 16                           # rows Ya - 4 .. Ya + nb + 3 of an item through a ring of 16


@pytest.mark.parametrize("case", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_walker_is_bit_identical_to_the_parent(case, monkeypatch):
    name, pages, kind, mvn = case
    gold = json.load(open(GOLDEN))["cases"][name]
    assert gold["pages"] == [list(s) for s in pages] and gold["image"] == kind and gold["mvn"] == mvn
    res = _both(case, monkeypatch)["1"]
    for n in (sc.D0, sc.D1):
        got = [sc.digest(a) for a in res[n]]
        assert got == gold["digests"][n], (name, n)


def test_resident_walker_blocks_per_cu():
    from citlab_article_separation_new_amd import _lib
    lib = _lib.init_device(0)
    down, up = lib.asep_aru_walker_occupancy(0), lib.asep_aru_walker_occupancy(1)
    print("resident blocks per CU: DOWN", down, "UP", up)
    assert down >= 8
    assert up == 4
