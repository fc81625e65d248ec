"""Point sets for the device triangulation tests (tests/test_delaunay_host.py, tests/test_delaunay_gpu.py): the smallest shapes at
which a triangulation can go wrong, the fuzzed articles of the contract check and the rule that sets an article aside."""
import numpy as np

import alpha_shape_cases as ac

# A second fuzz beside alpha_shape_cases.fuzz_articles(): lattices with holes and jitter, where cocircular cells are the rule.
# The seed was chosen on the CPU (tests/test_delaunay_host.py::test_contract_on_fuzz) so that scipy's triangulation alone sets
# aside at most 5 % of the articles of both fuzzes together; that test records the count.
LATTICE_SEED, LATTICE_COUNT = 4711, 160
NEAR_ALPHA_REL = 1e-9


def lattice(nx, ny, step=10, x0=0, y0=0):
    return np.array([(x0 + step * i, y0 + step * j) for j in range(ny) for i in range(nx)], np.int64)


def shapes(lds_points, max_extent):
    """(name, points, status the device must give) of the named shapes"""
    rng = np.random.RandomState(11)
    base = lattice(2, 40, 7)[:, ::-1].copy()                      # y = 0 and y = 7, x = 0, 7, ..: two parallel baselines
    dup = np.array([(0, 0), (10, 0), (0, 10), (10, 10), (10, 0), (5, 4), (5, 4), (0, 0)])

    def jittered(n, seed):
        return ac.big_article(n, seed)
    return [
        ("three_points", np.array([(0, 0), (5, 0), (2, 7)]), 0),
        ("three_points_clockwise", np.array([(0, 0), (2, 7), (5, 0)]), 0),
        ("square", np.array([(0, 0), (10, 0), (10, 10), (0, 10)]), 0),
        ("one_inside", np.array([(0, 0), (10, 0), (5, 10), (5, 3)]), 0),
        ("lattice_5x5", lattice(5, 5), 0),
        ("lattice_3x40", lattice(40, 3), 0),
        ("lattice_40x3", lattice(3, 40), 0),
        ("two_baselines", base, 0),
        ("first_points_collinear", np.array([(0, 0), (0, 5), (0, 10), (0, 15), (3, 7), (9, 9), (-4, 2)]), 0),
        ("negative_coordinates", rng.randint(-5000, -4000, (40, 2)), 0),
        ("one_baseline", np.array([(3 * i, 100 + 2 * i) for i in range(30)]), 2),
        ("two_points", np.array([(0, 0), (4, 4)]), 1),
        ("two_distinct_points", np.array([(0, 0), (4, 4), (0, 0), (4, 4), (4, 4)]), 1),
        ("duplicates", dup, 0),
        ("box_at_the_bound", np.array([(7, -3), (7 + max_extent, -3), (7, -3 + max_extent), (7 + max_extent, -3 + max_extent),
                                       (400, 9000), (16000, 12)]), 0),
        ("box_one_pixel_wider", np.array([(7, -3), (8 + max_extent, -3), (7, 50), (300, 300)]), 3),
        ("box_one_pixel_taller", np.array([(7, -3), (60, -3), (7, -2 + max_extent), (300, 300)]), 3),
        ("box_beyond_int32_differences", np.array([(-2 ** 31, -2 ** 31), (2 ** 31 - 1, 2 ** 31 - 1), (0, 5), (9, 1)]), 3),
        ("lds_points", jittered(lds_points, 5), 0),
        ("lds_points_plus_1", jittered(lds_points + 1, 6), 0),
    ]


def lattice_fuzz():
    """160 seeded articles on lattices of pitch 5-25: full, with holes, with a few jittered points, with duplicates; alpha0 around the
    cells' circumradii, so that accepting or refusing whole cocircular cells decides the boundary"""
    rng = np.random.RandomState(LATTICE_SEED)
    out = []
    for k in range(LATTICE_COUNT):
        nx, ny, step = int(rng.randint(2, 9)), int(rng.randint(2, 9)), int(rng.choice([5, 10, 17, 25]))
        pts = lattice(nx, ny, step, int(rng.randint(-50, 50)), int(rng.randint(-50, 50)))
        kind = k % 4
        if kind == 1 and len(pts) > 6:
            pts = pts[rng.rand(len(pts)) > 0.25]
        elif kind == 2:
            idx = rng.randint(0, len(pts), max(1, len(pts) // 6))
            pts[idx] += rng.randint(-2, 3, (len(idx), 2))
        elif kind == 3:
            pts = np.concatenate([pts, pts[rng.randint(0, len(pts), 3)]])
        # a corner triangle keeps every article two-dimensional
        pts = np.concatenate([pts, np.array([(-60, -60), (300, -55), (-58, 290)])])
        alpha = float(rng.choice([0.8, 1.1, 2.0, 6.0]) * step)
        out.append(("lattice/%d" % k, pts, alpha))
    return out


def fuzz_articles():
    """both fuzzes: (name, points, alpha0)"""
    return ac.fuzz_articles() + lattice_fuzz()


def near_tried_alpha(circ, alpha0, retries):
    """True when a circumradius lies within NEAR_ALPHA_REL (relative) of an alpha the reference tries: alpha0 and its ``retries``
    increases alpha + alpha * 0.2.  Two splits of a cocircular cell may then round to different sides of that alpha."""
    circ = np.asarray(circ, np.float64)
    circ = circ[np.isfinite(circ)]
    alpha = float(alpha0)
    for _ in range(retries + 1):
        if len(circ) and np.any(np.abs(circ - alpha) <= NEAR_ALPHA_REL * alpha):
            return True
        alpha = alpha + alpha * 0.2
    return False
