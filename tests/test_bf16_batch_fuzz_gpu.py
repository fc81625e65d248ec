"""Seeded fuzz of the bf16 engine over calls of 1 .. 5 pages of DIFFERENT sizes (asep_aru_forward_batch_dev2).

The hand-scheduled bf16 kernels decide by the composition of a call, not by one page's size: convr_kernel (csrc/convr_kernels.h) linearises its
work over (problem, strip, row) of ALL problems of a launch and cuts it into one contiguous range per wave -- a range that crosses a strip's end
restarts its input ring; res8w_kernel's band height comes from the strip rows of all problems (csrc/level0_plan.h, walk_band); five pages are
fifteen problems, more than the twelve of one launch (MAXP), so the launches split.  CASES is a fixed list (SEED) of 18 calls, 56 pages, whose page
sizes are drawn from classes chosen for those edges (level-3 maps = page / 8 at scale 0, / 16 and / 32 at scales 1 and 2):

  l3w<32, l3w=32, l3w=33, l3w=64, l3w=65   level-3 map of scale 0 narrower than one 32-column strip of convr_kernel, exactly one strip, one strip + one
                                           column, two strips, two strips + one column (page widths <= 248, 249..256, 257..264, 505..512, 513..520)
  l3h=1, l3h=2, l3h<8                      level-3 maps of 1, 2 and 3 .. 7 rows: shorter than convr_kernel's ring of 8 rows (page heights <= 8, 9..16, 17..56)
  strip_rem=0 .. strip_rem=23              pages that walk (four 24-column strips right of column 32, two 16-row bands below row 16): every residue of
                                           (W - 36) mod 24, the width of the border column right of the last strip
  one_band, several_bands, band_rem        walker regions of one 32-row band (H = 52, 53), of several, and of a last band shorter than 32 rows
                                           (the band is walk_band's minimum of 32 rows at these sizes)
  odd_H                                    a page that walks with an odd height: y_end = H - 5, the bottom border band one row higher
  walk@0, walk@0+1, walk@0+1+2, walk@none  room for the walkers at scale 0 only, at scales 0 and 1, at every scale, at none: walker and tile kernels
                                           side by side in one launch
  1x1, 2x3                                 pages of 1 x 1 and 2 x 3 pixels
and, per call: pages=1 .. pages=5, identical_pair (the same page twice in one call), tiny_beside_large (a 1 x 1 and a 2 x 3 page next to a large one).
Pages are at most 640 x 640 pixels.  test_the_case_list_covers_every_size_class (no GPU) holds the list to these classes.

On the GPU, every call of the list:
  * every page is bit-identical to its single-page call;
  * default against ASEP_BF_CONVR=0 and against ASEP_BF_RES32=0: the probabilities of every page bit-identical (same accumulation order).
Two forms of one engine share what they have in common, so ORACLE_MAX = 12 distinct pages of the list of at most 200 x 300 pixels, at least one of
every size class that fits under that cap (strip remainders: the residues the cover happens to take), are also held to the CPU oracle with the
engine's roundings: every end point block by block at BF16_BLOCK_MAX_GATE / BF16_BLOCK_RMS_GATE, the probabilities at BF16_EMU_PROB_GATE against
the free-running emulation (the gates of tests/test_aru_gpu.py).

Known gap: at pages of at most 640 x 640 pixels every launch's strip rows stay below walk_band's threshold, so the band is its 32-row minimum in
every call (the engine computes it per launch of at most MAXP problems, over the pages that walk; the CPU test bounds it from above with the
strip rows of the whole call): the composition of a call varies the walkers' item list and the launch splitting, not the band height.

The GPU tests share three engines (module fixture) and the default engine's batched results: every comparison reads results of calls that were
complete before it.  The comparison of the strip walkers with the tile kernels (ASEP_BF_WALK=0 / 2) over this list is not part of this file."""
import ctypes as C

import numpy as np
import pytest

SEED = 20261018
MAX_SIDE = 640
ORACLE_CAP = (200, 300)
ORACLE_MAX = 12
MAXP = 12
BAND = 32                           # walk_band(strip rows, 256 CUs, 8 waves) at these sizes: its minimum


def _cdiv(a, b):
    return -(-a // b)


def walks(H, W):
    """csrc/level0_plan.h, walk_region(H, W).fits (restated as in tests/test_split_walk_gpu.py; held to the header by tests/test_level0_plan_host.py)"""
    return (W - 4 - 32) // 24 >= 4 and H - 4 - 16 >= 32


def walk_band(strip_rows, num_cus=256, waves_per_cu=8):
    band = min(256, max(32, strip_rows // (6 * waves_per_cu * num_cus)))
    return (band + 1) & ~1


def strip_rows(H, W):
    return ((W - 36) // 24) * (2 * ((H - 20) // 2)) if walks(H, W) else 0


def page_classes(H, W):
    out = set()
    l3h, l3w = _cdiv(H, 8), _cdiv(W, 8)
    out.add("l3w<32" if l3w < 32 else f"l3w={l3w}" if l3w in (32, 33, 64, 65) else "l3w=other")
    out.add("l3h=1" if l3h == 1 else "l3h=2" if l3h == 2 else "l3h<8" if l3h < 8 else "l3h>=8")
    at = [s for s in range(3) if walks(_cdiv(H, 1 << s), _cdiv(W, 1 << s))]
    out.add("walk@" + ("+".join(map(str, at)) if at else "none"))
    if walks(H, W):
        rows = 2 * ((H - 20) // 2)
        out.add(f"strip_rem={(W - 36) % 24}")
        out.add("one_band" if rows <= BAND else "several_bands")
        if rows % BAND:
            out.add("band_rem")
        if H % 2:
            out.add("odd_H")
    if (H, W) in ((1, 1), (2, 3)):
        out.add(f"{H}x{W}")
    return out


def call_classes(call):
    out = {f"pages={len(call)}"}
    if len(set(call)) < len(call):
        out.add("identical_pair")
    sizes = [(H, W) for H, W, _ in call]
    if (1, 1) in sizes and (2, 3) in sizes and any(H >= 300 and W >= 300 for H, W in sizes):
        out.add("tiny_beside_large")
    return out


REQUIRED = ({"l3w<32", "l3w=32", "l3w=33", "l3w=64", "l3w=65", "l3h=1", "l3h=2", "l3h<8", "one_band", "several_bands", "band_rem", "odd_H",
             "walk@0", "walk@0+1", "walk@0+1+2", "walk@none", "1x1", "2x3", "identical_pair", "tiny_beside_large"}
            | {f"strip_rem={r}" for r in range(24)} | {f"pages={n}" for n in range(1, 6)})


def _cases():
    """[[(H, W, image seed), ...], ...]: the calls.  Pages with the same triple are the same image."""
    rng = np.random.default_rng(SEED)
    R = lambda a, b: int(rng.integers(a, b + 1))
    sizes = []
    for r in range(24):                                      # every strip remainder; every fourth small enough for the oracle
        small = r % 4 == 0
        sizes.append((R(52, 200) if small else R(52, MAX_SIDE), 36 + 24 * (R(4, 10) if small else R(4, 24)) + r))
    for lo, hi in ((249, 256), (257, 264), (505, 512), (513, 520)):          # level-3 maps of 32, 33, 64, 65 columns
        sizes.append((R(57, 200), R(lo, hi)))
    sizes += [(R(2, 8), R(40, 300)), (R(9, 16), R(40, 300)), (R(17, 51), R(132, 300)), (R(57, 63), R(300, MAX_SIDE))]       # level-3 maps of 1, 2, < 8, 8 rows
    sizes += [(52, R(132, 300)), (53, R(132, 300))]                           # one 32-row band (53: odd H)
    sizes += [(R(54, 102), R(132, 300)), (R(104, 200), R(264, 300)), (R(208, MAX_SIDE), R(528, MAX_SIDE)), (R(60, 200), R(33, 131))]   # walkers at 0 / 0+1 / all / none
    sizes += [(R(16, MAX_SIDE), R(16, MAX_SIDE)) for _ in range(12)]
    pages = [(H, W, 1000 + i) for i, (H, W) in enumerate(sizes)]
    rng.shuffle(pages)
    pages = [tuple(int(v) for v in p) for p in pages]
    twin = (R(150, 330), R(250, 540), 7)
    calls = [[(1, 1, 1), (R(300, MAX_SIDE), R(300, MAX_SIDE), 2), (2, 3, 3)],
             [twin, (R(40, 200), R(40, 300), 8), twin]]
    counts = [5, 2, 4, 1, 3]
    i = 0
    while pages:
        n = counts[i % len(counts)]
        calls.append(pages[:n])
        pages = pages[n:]
        i += 1
    return calls


CASES = _cases()


def distinct_pages(calls=None):
    seen, out = set(), []
    for call in (CASES if calls is None else calls):
        for p in call:
            if p not in seen:
                seen.add(p)
                out.append(p)
    return out


def oracle_pages(calls=None):
    """the pages under ORACLE_CAP that go to the CPU oracle: in list order, every page that adds a size class not seen yet (strip remainders count
    as they come), at most ORACLE_MAX"""
    fitting = [p for p in distinct_pages(calls) if p[0] <= ORACLE_CAP[0] and p[1] <= ORACLE_CAP[1]]
    covered, out = set(), []
    for generic in (False, True):                            # first the pages that add a named class, then further strip remainders
        for p in fitting:
            new = {c for c in page_classes(p[0], p[1]) - covered if generic or not c.startswith("strip_rem=")}
            if new and p not in out and len(out) < ORACLE_MAX:
                out.append(p)
                covered |= page_classes(p[0], p[1])
    return out


def test_the_case_list_covers_every_size_class():
    calls = CASES
    assert 18 <= len(calls) <= 24
    seen = set()
    for call in calls:
        assert 1 <= len(call) <= 5
        seen |= call_classes(call)
        for H, W, _ in call:
            assert 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE
            seen |= page_classes(H, W)
        assert walk_band(sum(strip_rows(_cdiv(H, 1 << s), _cdiv(W, 1 << s)) for H, W, _ in call for s in range(3))) == BAND
    assert not REQUIRED - seen, sorted(REQUIRED - seen)
    assert max(len(c) for c in calls) * 3 > MAXP             # five pages: fifteen problems, the launches split
    assert _cases() == calls                                 # the list is a function of SEED alone
    # the oracle's share: every class that a page under the cap can have, at most ORACLE_MAX pages
    chosen = oracle_pages()
    assert 0 < len(chosen) <= ORACLE_MAX and all(H <= ORACLE_CAP[0] and W <= ORACLE_CAP[1] for H, W, _ in chosen)
    got = set().union(*(page_classes(H, W) for H, W, _ in chosen))
    named = lambda s: {c for c in s if not c.startswith("strip_rem=")}
    fitting = set().union(*(page_classes(H, W) for H, W, _ in distinct_pages() if H <= ORACLE_CAP[0] and W <= ORACLE_CAP[1]))
    assert named(got) == named(fitting)
    assert named(got) >= {"l3w<32", "l3w=32", "l3w=33", "l3h=1", "l3h=2", "l3h<8", "one_band", "several_bands", "band_rem", "odd_H", "walk@0", "walk@0+1",
                          "walk@none", "1x1", "2x3"}
    assert len(got - named(got)) >= 3                        # several strip remainders


# ---- GPU ---------------------------------------------------------------------------------------
def _image(page):
    H, W, seed = page
    return np.random.default_rng(seed).random((H, W), dtype=np.float32)


class _Engines:
    """the bf16 engines of the comparisons, each created under its switch (the switches are read when the engine is created), side by side in
    this process; results that several tests need are computed once"""
    ENVS = {"default": {}, "convr0": {"ASEP_BF_CONVR": "0"}, "res320": {"ASEP_BF_RES32": "0"}}

    def __init__(self):
        from citlab_article_separation_new_amd import _lib, net_post_processing_helper as helper
        from citlab_article_separation_new_amd.config import AruConfig
        from citlab_article_separation_new_amd.weights import init_aru_weights
        self.helper = helper
        self.cfg = AruConfig(compute_dtype="bf16")
        self.w = init_aru_weights(self.cfg, 31, bias_jitter=0.05, logit_scale=0.05)
        self.lib = _lib.init_device(0)
        self.check = _lib.check
        switches = self.lib.asep_engine_switches().decode().split()
        self.graphs = {}
        mp = pytest.MonkeyPatch()
        try:
            for name, env in self.ENVS.items():
                for k in switches:
                    mp.delenv(k, raising=False)
                for k, v in env.items():
                    mp.setenv(k, v)
                g = helper.AruGraph(self.w, self.cfg)
                g.handle(0)                                  # the engine is created here, under the switch
                self.graphs[name] = g
        finally:
            mp.undo()
        self._batched = {}

    def close(self):
        for g in self.graphs.values():
            g.close()

    def single(self, name, page, endpoints=()):
        g = self.graphs[name]
        out = self.helper.get_net_output(_image(page), g, "0")
        return out, {n: self.helper.get_endpoint(g, n) for n in endpoints}

    def batched(self, name):
        """[[probabilities of page b of call c]] of every call of CASES through asep_aru_forward_batch_dev2"""
        if name not in self._batched:
            import torch
            h = self.graphs[name].handle(0)
            res = []
            for call in CASES:
                B = len(call)
                d_in = [torch.from_numpy(_image(p)).cuda() for p in call]
                d_out = [torch.empty(p[0], p[1], 2, device="cuda") for p in call]
                Arr, Ints = C.c_void_p * B, C.c_int32 * B
                rc = self.lib.asep_aru_forward_batch_dev2(h, B, Arr(*[t.data_ptr() for t in d_in]), Ints(*[p[0] for p in call]), Ints(*[p[1] for p in call]),
                                                          Arr(*[t.data_ptr() for t in d_out]), None, None, 0.5, None)
                self.check(rc, "asep_aru_forward_batch_dev2")
                torch.cuda.synchronize()
                res.append([t.cpu().numpy() for t in d_out])
            self._batched[name] = res
        return self._batched[name]


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


def _where(a, b):
    """where two maps differ: count and bounding box, for the message of a failed bit identity"""
    d = (a != b).any(axis=2)
    ys, xs = np.nonzero(d)
    return f"{int(d.sum())} pixels differ, rows {ys.min()}..{ys.max()}, columns {xs.min()}..{xs.max()}, max |d| {float(np.abs(a - b).max()):.3e}" if len(ys) else "equal"


def _assert_same_probabilities(e, other):
    a, b = e.batched("default"), e.batched(other)
    bad = [f"call {c} {[p[:2] for p in call]} page {i} {call[i][:2]}: {_where(a[c][i], b[c][i])}"
           for c, call in enumerate(CASES) for i in range(len(call)) if not np.array_equal(a[c][i], b[c][i])]
    assert not bad, f"{len(bad)} pages differ between the default engine and {_Engines.ENVS[other]}:\n" + "\n".join(bad[:10])


@pytest.mark.gpu
def test_every_page_of_a_call_is_bit_identical_to_its_single_page_call(engines):
    got = engines.batched("default")
    single = {p: engines.single("default", p)[0] for p in distinct_pages()}
    bad = [f"call {c} {[p[:2] for p in call]} page {i} {p[:2]}: {_where(got[c][i], single[p])}"
           for c, call in enumerate(CASES) for i, p in enumerate(call) if got[c][i].shape != single[p].shape or not np.array_equal(got[c][i], single[p])]
    assert not bad, f"{len(bad)} pages differ from their single-page calls:\n" + "\n".join(bad[:10])
    for call, res in zip(CASES, got):                        # the same page twice in a call: the same result twice
        for i, p in enumerate(call):
            for j in range(i):
                if call[j] == p:
                    assert np.array_equal(res[i], res[j])
    assert all(np.isfinite(x).all() for res in got for x in res)


@pytest.mark.gpu
def test_convr_kernel_against_convb_kernel_on_every_call(engines):
    _assert_same_probabilities(engines, "convr0")


@pytest.mark.gpu
def test_fused_32_channel_tail_against_its_layers_on_every_call(engines):
    _assert_same_probabilities(engines, "res320")


@pytest.mark.gpu
def test_pages_of_every_size_class_against_the_oracle_with_the_engines_roundings(engines):
    from citlab_article_separation_new_amd.config import AruConfig
    from oracle import aru_oracle
    from test_aru_gpu import BF16_BLOCK_MAX_GATE, BF16_BLOCK_RMS_GATE, BF16_EMU_PROB_GATE
    cfg32 = AruConfig(compute_dtype="f32")
    worst = [0.0, 0.0, 0.0]
    pages = oracle_pages()
    for p in pages:
        H, W, _ = p
        img = _image(p)
        ref, inter = aru_oracle.forward_torch(img, engines.w, cfg32, return_intermediates=True, storage="bf16")
        names = [n for n in sorted(inter) if n.startswith("scale_") or n.startswith("att_")]
        out, eng = engines.single("default", p, names)
        _, forced = aru_oracle.forward_torch(img, engines.w, cfg32, return_intermediates=True, storage="bf16", teacher=eng)
        for n in names:
            assert eng[n].shape == forced[n].shape, (H, W, n)
            scale = max(1.0, float(np.abs(forced[n]).max()))
            d = eng[n] - forced[n]
            dm, dr = float(np.abs(d).max()) / scale, float(np.sqrt(np.mean(d.astype(np.float64) ** 2))) / scale
            worst[0], worst[1] = max(worst[0], dm), max(worst[1], dr)
            assert dm <= BF16_BLOCK_MAX_GATE and dr <= BF16_BLOCK_RMS_GATE, (H, W, n, dm, dr)
        perr = float(np.abs(out - ref).max())
        worst[2] = max(worst[2], perr)
        assert perr <= BF16_EMU_PROB_GATE, (H, W, perr)
    print(f"\nbf16, {len(pages)} pages {[p[:2] for p in pages]}: block by block max {worst[0]:.2e} rms {worst[1]:.2e} of max|ref|; "
          f"probabilities against the free-running emulation {worst[2]:.2e}")
