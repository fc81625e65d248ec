"""scripts/roofline_from_profiles.py --level0: the f32s level-0 entry of a traced bench run -- the split-product walkers and the
res8v frame launches as one entry priced against mfma_bf16_split6, or the res8v blocks alone (CPU only, on the committed summaries)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import roofline_from_profiles as rfp  # noqa: E402

D = os.path.join(ROOT, "profiles", "l0_split_walk")


def _stats(rows):
    return {k: {"calls": c, "total_ns": t} for k, c, t in rows}


def test_walker_run_groups_the_pair_with_its_frame_and_prices_it_as_split_products():
    st = _stats([("res8ws_kernel<false>", 36, 6e6), ("res8ws_kernel<true>", 36, 9e6), ("res8v_down_kernel<0>", 36, 1e6),
                 ("res8v_up_kernel<0>", 36, 2e6), ("convs_kernel<3,3,true,1,16,2>", 216, 5e7)])
    t = rfp.level0_table(st, 6, 16, flops_page=1e12)
    assert [r["kernel"] for r in t["kernels"]] == list(rfp.LEVEL0_SPLIT_WALK)
    assert [r["role"] for r in t["kernels"]] == ["walker", "walker", "frame units", "frame units"]
    assert abs(t["level0_us_per_page"] - 18e6 / 1e3 / 96) < 0.5
    assert t["pipe"] == "mfma_bf16_split6" and abs(t["peak_tflops"] - 2500.0 / 6) < 1e-9


def test_res8v_run_is_the_whole_block_and_unpriced():
    t = rfp.level0_table(_stats([("res8v_down_kernel<0>", 36, 3e6), ("res8v_up_kernel<0>", 36, 4e6)]), 6, 16, flops_page=1e12)
    assert t["form"] == "res8v blocks" and all(r["role"] == "whole block" for r in t["kernels"]) and "pipe" not in t


def test_committed_traces_run_through_the_command_line(capsys):
    for form in ("res8v", "res8ws"):
        assert rfp.main(["x", "--level0", os.path.join(D, f"kernel_stats_{form}.csv"), os.path.join(D, f"bench_under_trace_{form}.json")]) == 0
        out = capsys.readouterr().out
        assert ("mfma_bf16_split6" in out) == (form == "res8ws")
