"""The ARU engine's launch records of one batch call, case by case: a plain helper (no fixtures) shared by tests/test_launch_records_gpu.py and
the recorder of its expectations, tests/golden/make_aru_launch_records.py.

A case = a model with seeded weights in a fresh handle, its environment set before the load, asep_aru_profile mode 2, ONE
asep_aru_forward_batch_dev2 call of the five PAGES (with attention: 15 problems, more than the MAXP = 12 of one launch, so every launcher's second
chunk is recorded too).  A record = [kernel name with layer text, calls, flops, bytes, executed_flops], the three numbers as the report prints them
(%.6e), in the report's order."""
import ctypes as C
import json
import os

import numpy as np

# 160 x 132: the smallest page whose scale 0 walks (test_kernel_selection_gpu.py); 203 x 389: scales 0 and 1 walk; 75 x 131: no walker
# (test_aru_batch_gpu.py); 2 x 3 (W < 32) and 4 x 104 (H < 8) from the pages of test_bf16_batch_fuzz_gpu.py
PAGES = [(160, 132), (203, 389), (75, 131), (2, 3), (4, 104)]

ELU = {"activation_name": "elu"}
# (case name, AruConfig fields, environment)
CASES = [
    ("relu_f32", {"compute_dtype": "f32"}, {}),
    ("relu_f32s", {"compute_dtype": "f32s"}, {}),
    ("relu_bf16", {"compute_dtype": "bf16"}, {}),
    ("elu_f32_fuse_act_1", {"compute_dtype": "f32", **ELU}, {"ASEP_FUSE_ACT": "1"}),
    ("elu_f32_fuse_act_0", {"compute_dtype": "f32", **ELU}, {"ASEP_FUSE_ACT": "0"}),
    ("elu_bf16", {"compute_dtype": "bf16", **ELU}, {}),
    ("u_f32", {"compute_dtype": "f32", "graph": "U"}, {}),
    ("u_bf16", {"compute_dtype": "bf16", "graph": "U"}, {}),
    ("rgb_ru_f32s", {"compute_dtype": "f32s", "graph": "RU", "channels": 3}, {}),
    ("xcd_sched_0_f32s", {"compute_dtype": "f32s"}, {"ASEP_XCD_SCHED": "0"}),
]

_weights = {}


def switch_names():
    from citlab_article_separation_new_amd import _lib
    return set(_lib.load_library().asep_engine_switches().decode().split())


def records(kw, env, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    """the records of one case; the engine's switches are cleared and `env` is set (through setenv / delenv) before the model is loaded"""
    import torch
    from citlab_article_separation_new_amd import _lib
    from citlab_article_separation_new_amd.config import AruConfig
    from citlab_article_separation_new_amd.weights import init_aru_weights
    from citlab_article_separation_new_amd.net_post_processing_helper import AruGraph
    for name in switch_names():
        delenv(name)
    for k, v in env.items():
        setenv(k, v)
    cfg = AruConfig(**kw)
    key = tuple(sorted((k, v) for k, v in kw.items() if k != "compute_dtype"))
    if key not in _weights:
        _weights[key] = init_aru_weights(cfg, 1234, bias_jitter=0.05, logit_scale=0.05)
    graph = AruGraph(_weights[key], cfg)
    try:
        lib = _lib.init_device(0)
        h = graph.handle(0)
        rng = np.random.default_rng(7)
        pages = [rng.random(s if cfg.channels == 1 else (*s, cfg.channels), dtype=np.float32) for s in PAGES]
        B = len(pages)
        d_in = [torch.from_numpy(p).cuda() for p in pages]
        d_out = [torch.empty(s[0], s[1], cfg.n_classes, device="cuda") for s in PAGES]
        Arr, Ints = C.c_void_p * B, C.c_int32 * B
        _lib.check(lib.asep_aru_profile(h, 2), "asep_aru_profile")
        try:
            rc = lib.asep_aru_forward_batch_dev2(h, B, Arr(*[t.data_ptr() for t in d_in]), Ints(*[s[0] for s in PAGES]), Ints(*[s[1] for s in PAGES]),
                                                 Arr(*[t.data_ptr() for t in d_out]), None, None, 0.5, None)
            _lib.check(rc, "asep_aru_forward_batch_dev2")
            torch.cuda.synchronize()
            buf = C.create_string_buffer(1 << 20)
            _lib.check(lib.asep_aru_profile_report(h, buf, len(buf)), "asep_aru_profile_report")
        finally:
            lib.asep_aru_profile(h, 0)
    finally:
        graph.close()
    # parse_float=str: the numbers stay the text the engine printed
    return [[r["kernel"], int(r["calls"]), r["flops"], r["bytes"], r["executed_flops"]] for r in json.loads(buf.value.decode(), parse_float=str)]
