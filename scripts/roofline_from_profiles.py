"""Recompute the `roofline` block of a bench.py line from the rocprofv3 summaries of the SAME run.

    python scripts/roofline_from_profiles.py profiles/<tag> [--tol 0.03]

Inputs (written by scripts/profile_bench.sh):
    <tag>/bench_under_trace.json   the bench line printed by the process rocprofv3 traced (--kernel-timing in-situ: every launch of
                                   that process runs in the real schedule, so rocprofv3's averages and the HIP-event averages of the
                                   line describe the same thing)
    <tag>/kernel_stats.csv         rocprofv3 --kernel-trace --stats: Name, Calls, TotalDurationNs, AverageNs
    <tag>/pmc_summary.json         FETCH_SIZE / WRITE_SIZE per kernel from their own --pmc passes (scripts/summarize_pmc.py)

Every field is recomputed WITHOUT the line's own timings: the launch duration from rocprofv3's AverageNs, the FLOPs per launch
from the line's per-kernel FLOP totals (they are shape arithmetic, not measurements), HBM bytes per launch as
(2 * FETCH_SIZE + WRITE_SIZE) * 1024 (gfx950 correction of MI355X_MICROARCH.md), the whole page from the sums over all asep::
kernels.  Prints a JSON report; exit code 1 if a compared field deviates by more than --tol (default 3 %).
The un-traced default run of the same build is <tag>/bench.json; it carries the isolated figure as well and differs from the
traced run by clocks (profiled passes run ~2-3 % slower, guide section 'Clocks')."""
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_traffic_json import kernel_key, traffic_table  # noqa: E402

PEAK_HBM_GBS = 8000.0


def load_line(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def block(line):
    """the line's roofline figures as one dict: round 4 split them into `roofline` (<= 20 keys, what a truncating record keeps) and
    `roofline_detail`; rounds 2-3 had one block"""
    return {**(line.get("roofline_detail") or {}), **line["roofline"]}


def recompute(tagdir):
    line = load_line(os.path.join(tagdir, "bench_under_trace.json"))
    r = block(line)
    layout4 = r.get("layout", 3) >= 4
    stats = {}
    for row in csv.DictReader(open(os.path.join(tagdir, "kernel_stats.csv"))):
        if "asep::" in row["Name"]:
            stats[kernel_key(row["Name"])] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                              "avg_ns": float(row["AverageNs"])}
    B = line["config"]["pages_per_step_per_gpu"]
    pages = (line["warmup"] + line["steps"] + r.get("event_timed_steps", 0)) * B
    kernels, page_bytes = traffic_table(json.load(open(os.path.join(tagdir, "pmc_summary.json"))), pages)
    k = r["kernel"]
    mem = k.split("+")                                         # round 6: the two level-0 blocks are reported as one entry "a+b": the family's mean launch
    for n in mem:
        if n not in stats:
            raise SystemExit(f"{n} not in kernel_stats.csv (have: {sorted(stats)[:6]} ...)")
    avg_us = sum(stats[n]["total_ns"] for n in mem) / sum(stats[n]["calls"] for n in mem) / 1e3
    lk = {q["kernel"]: q for q in line["kernels"]}
    exec_fl = r["executed_flops_per_launch"]
    hbm_bound = r["bound"] == "hbm"                            # bf16 lines: the primary figures are bytes / s, the matrix ones under "mfma"
    peak = (r["mfma_peak"] if layout4 else r["mfma"]["peak"]) if hbm_bound else r["peak"]
    # round 4 (layout 4), fp32: `achieved` is the ALGORITHMIC rate (direct-convolution FLOPs of the launch); before it, and again from
    # round 5 (layout 5): the executed one -- layout 5 prices it against the peak of the pipe the kernel runs on (`peak` of the line)
    layout5 = r.get("layout", 3) >= 5
    achieved = (r["flops_per_launch"] if layout4 and not layout5 and not hbm_bound else exec_fl) / (avg_us * 1e-6) / 1e12
    # whole page: executed FLOPs of all ARU-Net kernels per page (Winograd kernels execute 1/2.25 of their direct-conv credit)
    ev_steps = max(1, r.get("event_timed_steps", 1))
    # (layout 6: the line carries every kernel's executed FLOPs itself -- combine_kernel on the difference filter executes half its credit)
    xfl = lambda q: q["executed_flops"] if "executed_flops" in q else (q["flops"] / 2.25 if "wino" in q["kernel"] else q["flops"])
    exec_page = sum(xfl(q) for q in line["kernels"]) / (B * ev_steps)
    out = {
        "kernel": k,
        "avg_launch_us": avg_us,
        "mfma_achieved" if hbm_bound else "achieved": achieved,
        "mfma_frac" if hbm_bound else "frac": achieved / peak,
        "whole_page_executed_gflop": exec_page / 1e9,
        "whole_page_executed_frac": exec_page * line["value"] / line["n_gpus"] / 1e12 / peak,
    }
    if layout5:
        # the whole page: executed products of every kernel over its own pipe's peak (seconds at peak per page) x pages / s
        pipe_s = sum(xfl(q) / (q["pipe_peak_tflops"] * 1e12) for q in line["kernels"]) / (B * ev_steps)
        out["whole_page_executed_frac"] = pipe_s * line["value"] / line["n_gpus"]
    if all(n in kernels for n in mem):
        out["traffic"] = sum(kernels[n]["bytes_per_launch"] * kernels[n]["dispatches"] for n in mem) / sum(kernels[n]["dispatches"] for n in mem)
        out["hbm_tb_per_s"] = out["traffic"] / (avg_us * 1e-6) / 1e12
        out["hbm_frac"] = out["hbm_tb_per_s"] / (PEAK_HBM_GBS / 1e3)
        if hbm_bound and not layout4:                          # round 3: the bf16 block priced the COUNTER bytes
            out["achieved"] = out["hbm_tb_per_s"] * 1e3
            out["frac"] = out["hbm_frac"]
    if hbm_bound and layout4:                                  # round 4: ALGORITHMIC bytes per launch / rocprofv3's launch time
        out["achieved"] = r["algorithmic_bytes"] / (avg_us * 1e-6) / 1e9
        out["frac"] = out["achieved"] / PEAK_HBM_GBS
    out["whole_page_traffic_gb"] = page_bytes / 1e9
    out["whole_page_hbm_frac"] = page_bytes * line["value"] / line["n_gpus"] / 1e9 / PEAK_HBM_GBS
    # chip time per page by rocprofv3 (sum of all asep:: kernel durations; streams overlap, so this is >= the wall time per page)
    out["kernel_time_ms_per_page"] = sum(v["total_ns"] for v in stats.values()) / 1e6 / pages
    out["wall_ms_per_page"] = 1e3 / line["value"] * line["n_gpus"]
    # per-kernel table: rocprofv3 average vs the line's in-situ HIP-event average
    table = []
    for name, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ns"]):
        q = lk.get(name)
        ev = q and (q.get("avg_us_in_situ") or q.get("avg_us"))
        table.append({"kernel": name, "rocprof_avg_us": round(v["avg_ns"] / 1e3, 2), "hip_event_avg_us": ev,
                      "rel_dev": None if not ev else round(v["avg_ns"] / 1e3 / ev - 1.0, 4),
                      "hbm_bytes_per_launch": kernels.get(name, {}).get("bytes_per_launch")})
    return line, out, table


# f32s level 0: the split-product strip walkers and the res8v_* launches over the frame units around them are ONE level-0 entry,
# priced against the pipe the walkers run on -- six bf16 MFMA products per fp32 product: the dense bf16 peak / 6 (bench.py's pipe_of prices
# res8ws_* against the fp32 MFMA peak until its own labels follow).  The res8v_* launches of a walker build are the frame units only.
PEAK_BF16_MFMA_TFLOPS = 2500.0
LEVEL0_SPLIT_WALK = ("res8ws_kernel<false>", "res8ws_kernel<true>", "res8v_down_kernel<0>", "res8v_up_kernel<0>")


def level0_table(stats, steps, pages_per_step, flops_page=None):
    """per-step / per-page level-0 time of a kernel_stats table (kernel_key -> calls, total_ns): the pair of res8ws walkers and the res8v
    frame launches if the walkers ran, else the res8v blocks alone.  flops_page: useful level-0 FLOPs of a page (direct-convolution
    count) -> the walkers' rate against mfma_bf16_split6."""
    walk = any(k.startswith("res8ws_kernel") for k in stats)
    rows = []
    for k in LEVEL0_SPLIT_WALK:
        if k in stats:
            v = stats[k]
            rows.append({"kernel": k, "calls": v["calls"], "us_per_step": round(v["total_ns"] / 1e3 / steps, 1),
                         "us_per_page": round(v["total_ns"] / 1e3 / (steps * pages_per_step), 1),
                         "role": ("walker" if k.startswith("res8ws") else ("frame units" if walk else "whole block"))})
    total_page_us = sum(r["us_per_page"] for r in rows)
    out = {"form": "split-product strip walkers + res8v frame" if walk else "res8v blocks", "kernels": rows,
           "level0_us_per_page": round(total_page_us, 1)}
    if walk and flops_page:
        wk_s = sum(stats[k]["total_ns"] for k in LEVEL0_SPLIT_WALK[:2] if k in stats) / 1e9 / (steps * pages_per_step)
        out["pipe"] = "mfma_bf16_split6"
        out["peak_tflops"] = PEAK_BF16_MFMA_TFLOPS / 6.0
        out["level0_tflops"] = flops_page / (total_page_us * 1e-6) / 1e12
        out["level0_frac"] = out["level0_tflops"] / out["peak_tflops"]
        out["walker_s_per_page"] = wk_s
    return out


def compare(line, rec, tol):
    r = block(line)
    pairs = {"avg_launch_us": r.get("avg_launch_us_in_situ") or r["avg_launch_us"],
             "whole_page_executed_gflop": r["whole_page_executed_gflop"], "whole_page_executed_frac": r["whole_page_executed_frac"]}
    if r["bound"] == "hbm":
        if r.get("layout", 3) >= 4:
            pairs.update({"mfma_achieved": r["executed_tflops"], "mfma_frac": r["mfma_frac"]})
        else:
            pairs.update({"mfma_achieved": r["mfma"]["achieved"], "mfma_frac": r["mfma"]["frac"]})
        if "achieved" in rec:
            pairs.update({"achieved": r["achieved"], "frac": r["frac"]})
    else:
        pairs.update({"achieved": r["achieved"], "frac": r["frac"]})
    for f in ("traffic", "hbm_tb_per_s", "hbm_frac", "whole_page_traffic_gb", "whole_page_hbm_frac"):
        if r.get(f) is not None and f in rec:
            pairs[f] = r[f]
    dev = {f: (rec[f] / v - 1.0 if v else None) for f, v in pairs.items()}
    # a launch shorter than 1 ms is bracketed by two event records whose own latency (10-25 us together, more when a second lane's
    # launches are queued between them) is inside the HIP-event figure and outside rocprofv3's: the fields that divide by the launch
    # time get 6 % there (profiles/r4b: 518.5 us by events against 492.0 us by rocprofv3 for 864 launches), everything else keeps `tol`
    timed = {"avg_launch_us", "achieved", "frac", "mfma_achieved", "mfma_frac", "hbm_tb_per_s", "hbm_frac"}
    # (a launch of ~80 us -- the bf16 line's deep-level convolutions, round 6 -- pays the same ~5 us of event records: 8 % below 150 us)
    short = pairs["avg_launch_us"] < 1000.0
    short_tol = 0.08 if pairs["avg_launch_us"] < 150.0 else 0.06
    ok = all(d is not None and abs(d) <= (max(tol, short_tol) if short and f in timed else tol) for f, d in dev.items())
    return pairs, dev, ok


def main(argv):
    if argv[1] == "--level0":
        # python scripts/roofline_from_profiles.py --level0 <kernel_stats.csv> <bench line .json>: the level-0 table of a traced bench run
        stats = {}
        for row in csv.DictReader(open(argv[2])):
            if "asep::" in row["Name"]:
                stats[kernel_key(row["Name"])] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"])}
        line = load_line(argv[3])
        H, W = line["config"].get("height", 4500), line["config"].get("width", 3000)
        # useful level-0 work of a page at its three scales: DOWN 9 * 8 + 27 * 64, UP 9 * 128 + 27 * 64 products per pixel
        px = sum(-(-H // 2 ** s) * -(-W // 2 ** s) for s in range(3))
        flops_page = 2.0 * px * ((9 * 8 + 27 * 64) + (9 * 128 + 27 * 64))
        print(json.dumps(level0_table(stats, line["warmup"] + line["steps"], line["config"]["pages_per_step_per_gpu"], flops_page), indent=1))
        return 0
    tagdir = argv[1].rstrip("/")
    tol = float(argv[argv.index("--tol") + 1]) if "--tol" in argv else 0.03
    line, rec, table = recompute(tagdir)
    pairs, dev, ok = compare(line, rec, tol)
    print(json.dumps({"tag": tagdir, "tolerance": tol, "ok": ok, "recomputed": rec, "bench_line": pairs,
                      "rel_dev": {k: None if v is None else round(v, 4) for k, v in dev.items()}, "kernels": table}, indent=1))
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main(sys.argv))
