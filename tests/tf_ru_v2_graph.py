"""TEST INFRASTRUCTURE: an RU_v2 inference graph (the reference's ``backbones/RU_v2.py``) laid out the way TensorFlow 1.x freezes it.

The layers are those of tests/tf_aru_graph.py; what RU_v2 adds is the input pyramid -- a chain of AvgPool ops on the page, one per level
(RU_v2.py:92-96) -- and its concats: ``ConcatV2[pool(d_{l-1}), I_l]`` in front of conv1 of the down blocks l >= 1 (RU_v2.py:101) and, with
``inp4up``, the nested ``ConcatV2[ConcatV2[skip, deconv], I_l]`` in front of conv1 of the up blocks (RU_v2.py:142-144).  Variable scopes are
``ru_net/...`` (RU_v2.py:48).

``image_last=False`` and ``pyramid_ksize=3`` write the two malformed graphs the importer must refuse: the pooled page as the FIRST operand of
the concats, and a pyramid that is not the 2x2 / stride 2 / SAME average pool.
"""
import numpy as np

import tf_graphdef_proto as tp
from tf_aru_graph import AruGraphBuilder, F32


class RuV2GraphBuilder(AruGraphBuilder):
    def __init__(self, ns, weights, cfg, image_last=True, pyramid_ksize=2, **kw):
        super().__init__(ns, weights, cfg, **kw)
        self.image_last, self.pyramid_ksize = image_last, pyramid_ksize

    def concat(self, name, parts):
        axis = self.const(self.fresh(name + "/axis"), np.array(3, np.int32))
        return self.add(name, "ConcatV2", list(parts) + [axis], N=len(parts), T=F32, Tidx=tp.DType(tp.DT_INT32))

    def with_image(self, name, x, image):
        return self.concat(name, [x, image] if self.image_last else [image, x])

    def build(self):
        cfg, ren = self.cfg, self.rename
        n, base = cfg.scale_space_num, "ru_net/featMapG"
        k = self.pyramid_ksize
        img = self.add("inImg", "Placeholder", dtype=F32, shape=tp.Shape(-1, -1, -1, cfg.channels))
        pyr = [img]
        for l in range(1, n):
            pyr.append(self.add(ren(f"{base}/AvgPool_{l}" if l > 1 else f"{base}/AvgPool"), "AvgPool", [pyr[-1]], T=F32, ksize=[1, k, k, 1],
                                strides=[1, 2, 2, 1], padding="SAME", data_format="NHWC"))
        x, skips = img, []
        for l in range(n):
            scope = f"{base}/unet_down_{l}"
            if l > 0:
                x = self.with_image(ren(f"{scope}/concat"), x, pyr[l])
            x = self.res_block(x, scope, "")
            skips.append(x)
            if l < n - 1:
                x = self.pool(x, ren(f"{scope}/pool"), "MaxPool")
        for l in range(n - 2, -1, -1):
            scope = f"{base}/unet_up_{l}"
            d = self.deconv(x, skips[l], f"{scope}/deconv", "", cfg.feat(l))
            cat = self.concat(ren(f"{scope}/concat"), [skips[l], d])
            if cfg.inp4up:
                cat = self.with_image(ren(f"{scope}/concat_1"), cat, pyr[l])
            x = self.res_block(cat, scope, "")
        logits = self.conv(x, "ru_net/logit/class", "", act=False)
        logits = self.add(ren("ru_net/logit/logits"), "Identity", [logits], T=F32)
        self.add("output", "Softmax" if self.output_softmax else "Identity", [logits], T=F32)
        return tp.graphdef(self.ns, self.nodes).SerializeToString()


def build_ru_v2_pb(weights, cfg, packed_repeated=True, **kw):
    return RuV2GraphBuilder(tp.build_messages(packed_repeated), weights, cfg, **kw).build()
