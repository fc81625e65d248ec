"""bench.py on the CPU: the pieces of the contract that need no GPU -- how `--gpus N` without a torchrun environment starts its own
ranks (VERDICT r3 next #1a), and the shape of the roofline block (<= 20 keys, the HBM keys in front, strings below 120 characters)."""
import json
import os
import shutil
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _is_tracked(path):
    """git's index holds `path`.  The checkout may belong to another user than the one running the suite (git then refuses the
    repository unless it is named safe); a checkout without git metadata holds tracked files only, so there presence is the answer."""
    if not os.path.exists(os.path.join(ROOT, ".git")) or shutil.which("git") is None:
        return os.path.isfile(os.path.join(ROOT, path))
    r = subprocess.run(["git", "-c", f"safe.directory={ROOT}", "ls-files", "--error-unmatch", path], cwd=ROOT, capture_output=True)
    return r.returncode == 0


def test_gpus_n_without_torchrun_environment_spawns_a_child_and_relays_its_line(monkeypatch, capsys):
    calls = {}

    def fake_run(cmd, **kw):
        calls["cmd"], calls["kw"] = cmd, kw
        return types.SimpleNamespace(returncode=0, stdout='NCCL version 2.x banner\n{"metric": "m", "value": 1.0, "n_gpus": 4}\n')
    import subprocess
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    args = bench.parse_args()
    rc = bench.spawn_ranks(args)
    out = capsys.readouterr().out.strip().splitlines()
    assert rc == 0 and len(out) == 1 and json.loads(out[0])["n_gpus"] == 4          # exactly one line: the child's JSON, not its banner
    cmd = calls["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert calls["kw"]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # a child that dies is reported through the exit code, nothing is printed in its place
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: types.SimpleNamespace(returncode=3, stdout=""))
    assert bench.spawn_ranks(args) == 3 and capsys.readouterr().out == ""


def test_main_takes_the_spawn_path_before_anything_touches_the_gpu(monkeypatch):
    """WORLD_SIZE unset and --gpus 2: main() must hand over to spawn_ranks BEFORE importing torch in this process"""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setattr(bench, "spawn_ranks", lambda args: 17)
    monkeypatch.setattr(bench, "torch", None)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 17 and bench.torch is None


def _kernel(name, calls, avg_us, flops, byts, wino=False):
    total_ms = calls * avg_us * 1e-3
    k = {"kernel": name, "calls": calls, "total_ms": total_ms, "avg_us": avg_us, "flops": flops * calls, "bytes": byts * calls}
    k["tflops"] = k["flops"] / (total_ms * 1e-3) / 1e12
    k["executed_flops"] = k["flops"] / 2.25 if wino else k["flops"]
    k["executed_tflops"] = k["tflops"] / 2.25 if wino else k["tflops"]
    k["algo_gbs"] = k["bytes"] / (total_ms * 1e-3) / 1e9
    return k


def test_headline_dtype_is_f32s_and_a_split_product_kernel_is_priced_against_a_sixth_of_the_bf16_peak():
    """round 5: the default line is --dtype f32s; a split-product kernel executes six bf16 MFMA products per fp32 product, so its roofline
    `peak` is 2500 / 6 TFLOP/s of fp32-equivalent products; a vector-ALU kernel is priced against the fp32 peak; `frac` never exceeds 1"""
    args = types.SimpleNamespace(dtype="f32s", no_gnn=False, gnn="visual")
    dom = _kernel("convs_kernel<3,3,false,4,8,2>", 216, 300.0, 56.76e9, 0.374e9)
    other = _kernel("res8v_up_kernel<0>", 18, 3900.0, 282.9e9, 4.7e9)
    for k in (dom, other):
        k["pipe"], k["pipe_peak"] = bench.pipe_of(k["kernel"], "f32s")
    assert abs(dom["pipe_peak"] - bench.PEAK_BF16_MFMA_TFLOPS / 6) < 1e-9 and other["pipe_peak"] == bench.PEAK_F32_MFMA_TFLOPS
    pipe_s = sum(k["executed_flops"] / (k["pipe_peak"] * 1e12) for k in (dom, other)) / (16 * 3)
    r, d = bench.build_roofline(args, dom, dom, dom, [dom, other], 400e9, 135.0, bench.PEAK_F32_MFMA_TFLOPS, 4.0, 3, True, 16, 4500, 3000, pipe_s)
    assert len(r) <= 20 and r["bound"] == "mfma_bf16_split6" and abs(r["peak"] - 416.67) < 0.01 and "bf16 MFMA" in r["pipe"]
    assert abs(r["achieved"] - 56.76e9 / 300e-6 / 1e12) < 1e-2 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["frac"] <= 1.0
    assert abs(r["whole_page_executed_frac"] - pipe_s * 135.0) < 1e-4 and d["launches_per_step"] == 72 and d["layout"] == 6
    r2, _ = bench.build_roofline(args, other, other, other, [dom, other], 400e9, 135.0, bench.PEAK_F32_MFMA_TFLOPS, 4.0, 3, True, 16, 4500, 3000, pipe_s)
    assert r2["peak"] == bench.PEAK_F32_MFMA_TFLOPS and "vector ALU" in r2["pipe"] and r2["frac"] <= 1.0 and r2["bound"] == "valu_fp32"
    import sys as _sys
    old = _sys.argv
    try:
        _sys.argv = ["bench.py"]
        a = bench.parse_args()
    finally:
        _sys.argv = old
    assert a.dtype == "f32s" and a.plain_steps > 0 and a.bf16_steps > 0 and a.steps == 80


def test_compute_dtype_names_of_the_python_side_match_the_header():
    import re
    from citlab_article_separation_new_amd.net_post_processing_helper import COMPUTE_DTYPES
    hdr = open(os.path.join(ROOT, "include", "asep_hip.h")).read()
    m = re.search(r"int32_t compute_dtype;\s*/\*(.*?)\*/", hdr, re.S)
    assert m and "0 = fp32" in m.group(1) and "1 = bf16" in m.group(1) and "2 = fp32 tensors" in m.group(1)
    assert COMPUTE_DTYPES == {"f32": 0, "bf16": 1, "f32s": 2}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_roofline_block_shape_and_arithmetic(dtype, monkeypatch):
    args = types.SimpleNamespace(dtype=dtype, no_gnn=False, gnn="visual")
    if dtype == "f32":
        dom = _kernel("conv_wino_kernel<4,false>", 216, 527.0, 56.76e9, 0.374e9, wino=True)
        iso = _kernel("conv_wino_kernel<4,false>", 216, 319.0, 56.76e9, 0.374e9, wino=True)
        peak = bench.PEAK_F32_MFMA_TFLOPS
    else:
        dom = _kernel("res8f_kernel<true>", 18, 1238.0, 282.9e9, 2.3575e9)
        iso = _kernel("res8f_kernel<true>", 18, 1116.0, 282.9e9, 2.3575e9)
        peak = bench.PEAK_BF16_MFMA_TFLOPS
    other = _kernel("combine_kernel<8,2,false,3>", 48, 150.0, 6.9e9, 0.4e9)
    r, d = bench.build_roofline(args, dom, iso, dom, [dom, other], 400e9, 120.0, peak, 4.0, 3, True, 16, 4500, 3000)
    assert len(r) <= 20 and list(r)[:6] == ["bound", "kernel", "achieved", "peak", "unit", "frac"]
    assert list(r).index("traffic") < 8 and list(r).index("whole_page_hbm_frac") < 12
    assert all(len(v) < 120 for v in r.values() if isinstance(v, str)) and r["traffic_source"]
    assert r["timing"].startswith("in situ, one page lane") and r["frac"] == r["frac_in_situ"] and d["launches_per_step"] == dom["calls"] / 3
    if dtype == "f32":
        # achieved = EXECUTED TFLOP/s: a Winograd kernel executes 1 / 2.25 of its direct-convolution credit; that credit is carried in
        # separately named keys and may exceed the peak (isolated: 1.13 here), `frac` may not
        assert r["bound"] == "mfma_fp32" and abs(r["achieved"] - 56.76e9 / 2.25 / 527e-6 / 1e12) < 1e-2 and r["peak"] == bench.PEAK_F32_MFMA_TFLOPS
        assert abs(r["algorithmic_tflops"] - 2.25 * r["achieved"]) < 1e-2 and abs(d["algorithmic_over_peak"] - 2.25 * r["frac"]) < 2e-3
        assert r["frac"] <= 1.0 and r["frac_isolated"] <= 1.0 and 2.25 * r["frac_isolated"] > 1.0
    else:
        # achieved = ALGORITHMIC bytes per launch / launch time against 8 TB/s; the matrix-core figure beside it
        assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["achieved"] - 2.3575e9 / 1238e-6 / 1e9) < 0.2
        assert abs(r["frac"] - r["achieved"] / 8000.0) < 1e-4 and 0 < r["mfma_frac"] < 0.2
    assert r["algorithmic_bytes"] == round(dom["bytes"] / dom["calls"]) and d["layout"] == 6 and d["pages_per_launch"] == 4.0
    # the committed counters belong to 16 pages per step at 3000 x 4500 with the visual net: used; any other workload: the reason instead
    if r["traffic"] is not None:
        assert r["traffic"] >= 0.98 * r["algorithmic_bytes"] and r["hbm_frac"] > 0 and r["whole_page_traffic_gb"] > 1
    r2, _ = bench.build_roofline(args, dom, iso, dom, [dom, other], 400e9, 120.0, peak, 4.0, 3, True, 3, 4500, 3000)
    assert r2["traffic"] is None and "pages_per_step" in r2["traffic_source"]


def test_dominant_kernel_is_ranked_in_situ_and_the_traffic_label_names_a_tracked_file():
    """round 6: the dominant kernel is the one with the largest IN-SITU summed launch time -- what rocprofv3's
    kernel_stats.csv of the same command puts first -- not the leader of the isolated pass; `traffic_source` names a file of the tree"""
    up_iso, down_iso = _kernel("res8v_up_kernel<0>", 18, 3900.0, 282.9e9, 4.7e9), _kernel("res8v_down_kernel<0>", 18, 2700.0, 176.8e9, 2.2e9)
    up_situ, down_situ = _kernel("res8v_up_kernel<0>", 18, 4106.0, 282.9e9, 4.7e9), _kernel("res8v_down_kernel<0>", 18, 4705.0, 176.8e9, 2.2e9)
    c_iso, c_situ = _kernel("convs_kernel<3,3,true,1,16,2>", 108, 469.0, 30e9, 0.57e9), _kernel("convs_kernel<3,3,true,1,16,2>", 108, 1000.0, 30e9, 0.57e9)
    iso = {k["kernel"]: k for k in (up_iso, down_iso, c_iso)}
    situ = {k["kernel"]: k for k in (up_situ, down_situ, c_situ)}
    top = bench.rank_kernels(iso, situ)
    # in situ the short level-1 launches (108 x 1.0 ms beside the attention branch) outweigh either level-0 block alone, not the pair
    assert top[0]["kernel"] == "res8v_down_kernel<0>+res8v_up_kernel<0>" and top[1]["kernel"] == "convs_kernel<3,3,true,1,16,2>"
    assert abs(top[0]["executed_tflops"] - (176.8e9 + 282.9e9) * 18 / ((4106.0 + 4705.0) * 18e-6) / 1e12) < 1e-6
    args = types.SimpleNamespace(dtype="f32s", no_gnn=False, gnn="visual")
    for k in situ.values():
        k["pipe"], k["pipe_peak"] = bench.pipe_of(k["kernel"], "f32s")
    r, d = bench.build_roofline(args, top[0], bench.entry_of(iso, top[0]), top[0], list(situ.values()), 400e9, 135.0, bench.PEAK_F32_MFMA_TFLOPS, 4.0, 1,
                                True, 16, 4500, 3000)
    assert r["bound"] == "valu_fp32" and r["frac_in_situ"] < r["frac_isolated"] and [m["kernel"] for m in d["members"]] == top[0]["members"]
    assert r["traffic"] is not None and d["members"][0]["frac"] < d["members"][1]["frac"]        # the down block is the one the side stream slows
    for dtype, name in (("f32s", "res8v_up_kernel<0>"), ("bf16", "res8w_kernel<true>"), ("f32", "conv_wino_kernel<4,false>")):
        args = types.SimpleNamespace(dtype=dtype, no_gnn=False, gnn="visual")
        dom = _kernel(name, 18, 1000.0, 282.9e9, 2.3575e9)
        dom["pipe"], dom["pipe_peak"] = bench.pipe_of(name, dtype)
        r, _ = bench.build_roofline(args, dom, dom, dom, [dom], 400e9, 120.0, bench.PEAK_F32_MFMA_TFLOPS, 4.0, 3, True, 16, 4500, 3000)
        assert r["traffic"] is not None, r["traffic_source"]
        path = r["traffic_source"].split("offline PMC: ")[1].split(" @")[0]
        assert path.startswith("profiles/") and os.path.exists(os.path.join(ROOT, path)) and "being collected" not in r["traffic_source"]
        assert _is_tracked(path), f"{path} is not tracked"


def test_every_bf16_mfma_kernel_of_the_bf16_header_is_priced_against_the_bf16_pipe():
    """deconvb8_kernel and att_headb_kernel fell through to the fp32 peak (0.83 / 0.90 of a pipe they do not run on).  Every
    __global__ function of csrc/bf16_kernels.h that issues v_mfma_f32_16x16x32_bf16 must map to the bf16 pipe with --dtype bf16."""
    import re
    mfma, all_names = [], []
    for fname in ("bf16_kernels.h", "res8w_kernels.h", "convr_kernels.h"):
        src = open(os.path.join(ROOT, "citlab-article-separation-new_amd", "csrc", fname)).read()
        names = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", src)
        all_names += names
        for n in names:
            body = src[src.index(n + "("):]
            nxt = re.search(r"\n__global__", body[10:])
            body = body[:nxt.start() + 10] if nxt else body
            if "mfma" in body or "r8w_mm" in body or "cvr_mfma" in body or "mm_pair" in body or "_tile<" in body or "_tile(" in body:
                mfma.append(n)
    assert len(all_names) >= 12, all_names
    assert {"deconvb8_kernel", "att_headb_kernel", "res8f_kernel", "convb_kernel", "res8w_kernel", "res8wb_kernel", "convr_kernel"} <= set(mfma), mfma
    for n in mfma:
        pipe, peak = bench.pipe_of(n + "<1,2>", "bf16")
        assert pipe == "bf16 MFMA" and peak == bench.PEAK_BF16_MFMA_TFLOPS, n
        assert bench.bound_of(pipe, False) == "mfma_bf16"


def test_a_plain_run_measures_the_headline_only_and_full_keeps_the_rest(monkeypatch):
    """a plain `bench.py --gpus 1 --steps N --warmup W` times the steps and prints the line; the CPU baseline, the event passes and the secondary
    figures run with --full only, with the options that select them as before"""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_secondary and a.kernel_timing == "none"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--full", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "d" and not a.no_cpu_baseline and not a.no_secondary and a.kernel_timing == "both"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--kernel-timing", "in-situ", "--no-secondary"])
    a = bench.parse_args()
    assert a.kernel_timing == "in-situ" and a.no_secondary and a.steps == 80
