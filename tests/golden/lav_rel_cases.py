"""Seeded cases of the relation net evaluation golden (tests/golden/lav_rel_golden.json): per case a list of pages, each a
(targets int32 [1, R], output float32 [1, R, 2]) batch as the reference's loop sees it, and the flags that steer the tables."""
import numpy as np


def _labels(rng, n, frac):
    """a planted partition of n nodes into articles -> the N * N labels of build_full_relations (pairs of one article, both
    directions, no self pairs), thinned to about `frac` of them"""
    art = rng.integers(0, max(2, n // 3), size=n)
    same = (art[:, None] == art[None, :]) & ~np.eye(n, dtype=bool)
    return (same & (rng.random((n, n)) < frac)).reshape(-1).astype(np.int32)


def _scores(rng, labels, sharp):
    """float32 scores in [0, 1] that lean towards the label"""
    z = rng.normal(0.0, 1.0, labels.shape) + sharp * (2.0 * labels - 1.0)
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def _case(name, seed, sizes, transform=None, frac=0.9, sharp=1.0, **flags):
    rng = np.random.default_rng(seed)
    pages = []
    for n in sizes:
        y = _labels(rng, n, frac)
        p = _scores(rng, y, sharp)
        if transform is not None:
            p, y = transform(rng, p, y)
        p = np.ascontiguousarray(p, np.float32)
        out = np.stack([np.float32(1) - p, p], axis=-1)[None]          # [1, R, 2]: the last class column is the score
        pages.append((np.ascontiguousarray(y, np.int32)[None], out))
    return {"name": name, "pages": pages, "flags": dict({"num_p_r_thresholds": 20, "batch_limiter": -1}, **flags)}


def _quantised(levels):
    return lambda rng, p, y: (np.round(p * levels) / np.float32(levels), y)


def _all_equal(rng, p, y):
    return np.full_like(p, 0.5), y


def _zeros_ones(rng, p, y):
    p = p.copy()
    k = rng.random(p.shape)
    p[k < 0.2] = 0.0
    p[k > 0.8] = 1.0
    return p, y


def _denormals(rng, p, y):
    p = p.copy()
    tiny = np.array([1e-45, 3e-45, 1e-40, 1e-39, 1.1754942e-38, 1.17549435e-38, 0.0], np.float32)   # denormals, the largest one, the smallest normal
    k = rng.random(p.shape) < 0.5
    p[k] = tiny[rng.integers(0, len(tiny), size=int(k.sum()))]
    return p, y


def _no_positive(rng, p, y):
    return p, np.zeros_like(y)


def _no_negative(rng, p, y):
    return p, np.ones_like(y)


def cases():
    return [
        _case("pages_of_different_n", 11, (7, 12, 5, 9)),
        _case("quantised_4", 12, (10, 6), _quantised(4)),
        _case("quantised_2_blurred", 13, (8, 8, 3), _quantised(2), sharp=0.2),
        _case("all_equal", 14, (6, 4), _all_equal),
        _case("zeros_and_ones", 15, (9, 7), _zeros_ones),
        _case("denormals", 16, (8, 6), _denormals),
        _case("few_thresholds", 17, (5,), _quantised(5)),                 # 6 distinct scores at most, 20 table rows asked for
        _case("seven_table_rows", 18, (11, 4), num_p_r_thresholds=7),
        _case("three_table_rows_sharp", 19, (10,), sharp=3.0, num_p_r_thresholds=3),
        _case("batch_limiter_2", 20, (6, 7, 8, 5), batch_limiter=2),
        _case("one_page_one_node", 21, (1, 6)),
        _case("no_positive", 22, (6,), _no_positive),
        _case("no_negative", 23, (5,), _no_negative),
    ]


def concatenated(case):
    """(labels int32 [n], scores float32 [n]) of the pages the evaluation reads (batch_limiter applied)"""
    lim = case["flags"]["batch_limiter"]
    pages = case["pages"] if lim == -1 else case["pages"][:lim]
    return (np.concatenate([t[0] for t, _ in pages]), np.concatenate([o[0, :, -1] for _, o in pages]))
