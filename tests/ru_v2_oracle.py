"""Restatement of the reference's ``article_separation/backbones/RU_v2.py`` (graph 'RU_v2': the RU-Net with an input pyramid) in numpy,
float64 by default, built from the primitives of ``oracle/aru_oracle.py``.  ``tests/test_ru_v2_host.py`` holds it to the logits that the
reference's own ``RU_v2_CNN.infer`` produced (``tests/golden/model_wiring_ru_v2.npz``); the GPU tests hold the engine to it.

Unlike the reference, which returns no end points (RU_v2.py:31), ``forward`` returns every block output under the engine's names
``scale_0_unet_{down,up}_<l>_{conv,deconv}`` plus ``logits``."""
import numpy as np

from oracle.aru_oracle import (activation_fn, avg_pool2, conv2d_same, deconv2d, max_pool2, per_image_standardization, relu, softmax)


def input_pyramid(x, levels):
    """RU_v2.py:92-96: I_0 = the (standardised) page, I_l = avg_pool2d(I_{l-1}, 2x2, stride 2, SAME)"""
    pyr = [x]
    for _ in range(1, levels):
        pyr.append(avg_pool2(pyr[-1]))
    return pyr


def _res_block(u, w, p, res_depth, act):
    """RU_v2.py:103-118 / :146-161: conv1 (identity) -> t; relu (always a ReLU); (res_depth - 1) x conv + act; conv (identity); + t; act"""
    t = conv2d_same(u, w[p + "/conv1/weights"], w[p + "/conv1/biases"])
    r = relu(t)
    for a in range(res_depth):
        r = conv2d_same(r, w[p + f"/convR_{a}/weights"], w[p + f"/convR_{a}/biases"])
        if a < res_depth - 1:
            r = act(r)
    return act(r + t)


def conv1_inputs(image, w, cfg, dtype=np.float64):
    """(scope, main operand, pooled page) of every conv1 that reads the pyramid, in graph order -- for the linear-split test"""
    out = []
    forward(image, w, cfg, dtype, _conv1_log=out)
    return out


def forward(image, w, cfg, dtype=np.float64, return_intermediates=False, _conv1_log=None):
    """image [H,W] or [H,W,C] -> probabilities (logits if not cfg.apply_softmax) [H,W,n_classes]"""
    x = np.asarray(image, dtype=dtype)
    if x.ndim == 2:
        x = x[:, :, None]
    w = {k: np.asarray(v, dtype=dtype) for k, v in w.items()}
    if cfg.mvn:
        x = per_image_standardization(x)                           # RU_v2.py:49-51: the pyramid is built from the standardised page
    n = cfg.scale_space_num
    act = activation_fn(cfg.activation_name)
    pyr = input_pyramid(x, n)
    inter, skips = {}, []
    u = x
    for l in range(n):                                              # RU_v2.py:98-130
        p = f"ru_net/featMapG/unet_down_{l}"
        if l > 0:
            if _conv1_log is not None:
                _conv1_log.append((p + "/conv1", u, pyr[l]))
            u = np.concatenate([u, pyr[l]], axis=2)                 # the image rows come last
        d = _res_block(u, w, p, cfg.res_depth, act)
        skips.append(d)
        inter[f"scale_0_unet_down_{l}_conv"] = d
        u = max_pool2(d) if l < n - 1 else d
    for l in range(n - 2, -1, -1):                                  # RU_v2.py:132-169
        p = f"ru_net/featMapG/unet_up_{l}"
        skip = skips[l]
        v = act(deconv2d(u, w[p + "/deconv/weights"], w[p + "/deconv/bias"], skip.shape[:2], cfg.pool_size))
        inter[f"scale_0_unet_up_{l}_deconv"] = v
        c = np.concatenate([skip, v], axis=2)
        if cfg.inp4up:
            if _conv1_log is not None:
                _conv1_log.append((p + "/conv1", c, pyr[l]))
            c = np.concatenate([c, pyr[l]], axis=2)                 # RU_v2.py:143-144
        u = _res_block(c, w, p, cfg.res_depth, act)
        inter[f"scale_0_unet_up_{l}_conv"] = u
    logits = conv2d_same(u, w["ru_net/logit/class/weights"], w["ru_net/logit/class/biases"])
    inter["logits"] = logits
    out = softmax(logits, axis=2) if cfg.apply_softmax else logits
    return (out, inter) if return_intermediates else out
