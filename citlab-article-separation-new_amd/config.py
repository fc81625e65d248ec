"""Model hyper-parameters of the two hot-path nets.

Defaults follow the reference's defaults:
  * ARU-Net: ``article_separation/backbones/ARU_v1.py:35-43`` (graph 'ARU' switches the
    attention branch on, ``ARU_v1.py:94-98``).
  * GNN: ``gnn/model/graph/graph_gnn.py:19-25``, ``message_fn_chunk.py:13-40``,
    ``update_fn_lstm.py:12-19``, ``gnn/trainer/trainer_rel.py:15-17``.
"""
from dataclasses import dataclass, field, asdict
from typing import List


@dataclass
class AruConfig:
    graph: str = "ARU"            # 'U' (plain conv1 + conv2 blocks), 'RU' (residual blocks) or 'ARU' (+ attention), ARU_v1.py:92-97;
                                  # 'RU_v2' (RU_v2.py): the RU-Net with the average-pooled page concatenated into conv1 of its blocks
    channels: int = 1             # image channels: 1 (gray) or, for the graphs without attention (RU / U), 3 (RGB, interleaved [H,W,3])
    n_classes: int = 2
    feat_root: int = 8
    scale_space_num: int = 5
    res_depth: int = 3
    num_scales_att: int = 3
    filter_size: int = 3
    pool_size: int = 2
    activation_name: str = "relu"  # ARU_v1.py:43,70-75: 'relu', 'elu' or 'leaky' (leak 0.1, layers.py:10-30)
    mvn: bool = False
    apply_softmax: bool = True    # export-time class softmax -> 'output:0'
    # The engine's arithmetic -- an engine option, not a property of the weights:
    #   'f32s' (default since round 5): fp32 tensors, fp32 accumulation, fp32 results; the products of the convolutions with >= 12 input
    #           channels as six bf16 x bf16 partial products of the exact three-way bfloat16 split of both factors (dropped terms
    #           <= 2^-23 |x w|); level 0, first / last layers and deconvolutions on the fp32 FMA / MFMA.  Held to the fp32 parity gates.
    #   'f32':  every product on the fp32 pipes (v_mfma_f32_16x16x4_f32, Winograd F(2x2,3x3) from 32 channels, v_pk_fma_f32 at level 0)
    #   'bf16': BASELINE configs[4] "bf16 convs": bf16 tensors and MFMA operands, fp32 accumulation (its own, wider gates)
    compute_dtype: str = "f32s"
    inp4up: bool = True           # graph 'RU_v2' only (RU_v2.py:13,143): the pooled page also goes into conv1 of the up blocks

    @property
    def use_attention(self) -> bool:
        return "ARU" in self.graph

    @property
    def input_pyramid(self) -> bool:
        return self.graph == "RU_v2"

    @property
    def root_scope(self) -> str:
        """the variable scope of the graph: RU_v2.py:48 'ru_net', ARU_v1.py 'aru_net'"""
        return "ru_net" if self.input_pyramid else "aru_net"

    @property
    def use_residual(self) -> bool:
        return "RU" in self.graph                 # ARU_v1.py:94-95 ('U' alone: conv1 + conv2 blocks)

    @property
    def activation_code(self) -> int:
        """asep_aru_cfg.activation"""
        try:
            return {"relu": 0, "elu": 1, "leaky": 2}[self.activation_name]
        except KeyError:
            raise ValueError(f"activation_name must be 'relu', 'elu' or 'leaky' (ARU_v1.py:43), got {self.activation_name!r}")

    def feat(self, level: int) -> int:
        return self.feat_root * (self.pool_size ** level)

    def check_channels(self):
        """the image channels the engine serves; raises ``ValueError`` with the reason otherwise (the same rule as ``asep_aru_load``)"""
        if self.channels not in (1, 3):
            raise ValueError(f"{self.channels} input channels: 1 (gray) and 3 (RGB) are supported")
        if self.channels == 3 and self.use_attention:
            raise ValueError("3-channel input needs a graph without attention (RU or U): the attention graph upsamples its attention "
                             "map to the input's shape with a one-channel filter (ARU_v1.py:115)")

    def check_graph(self):
        """what the engine serves of the graph 'RU_v2'; raises ``ValueError`` with the reason otherwise (the same rules as ``asep_aru_load``)"""
        if self.input_pyramid and self.compute_dtype == "bf16":
            raise ValueError("graph 'RU_v2' runs on the fp32 engines (compute_dtype 'f32s' or 'f32'): the bf16 engine's fused block tails round "
                             "conv1's result to bfloat16 before the pooled page's term could be added")

    def to_dict(self):
        return asdict(self)


@dataclass
class GnnConfig:
    node_feature_dim: int = 7         # after masking (vn7e2: 7 of 15, nets/README.md:24-27)
    edge_feature_dim: int = 2
    num_transition_steps: int = 3
    hidden_dim: int = 32              # hidden_node_feature_dim
    interaction_dim: int = 32         # interaction_feature_dim
    interaction_hidden: List[int] = field(default_factory=lambda: [32])
    classifier_hidden: List[int] = field(default_factory=lambda: [64, 32])
    num_classes: int = 2
    undirected_graph: bool = True
    # graph_gnn.py:20,102-109: > 0: the (concatenated) node features go through ff_layer(tanh) to this width before the GNN
    compress_node_feature_dim: int = 0
    # graph_gnn.py:23,158-166: 'hidden', 'add_final_hidden_and_input' (h += x W) or 'concat_final_hidden_and_input' ([h | x]); x = the
    # node features as fed
    output_type: str = "hidden"
    # message_fn_chunk.py:35-41: learned attention over the in-edges instead of the degree-normalised sum (the default, False)
    use_attention: bool = False
    num_attention_heads: int = 1
    multihead_attention_merge_type: str = "concat"        # 'concat' (x_dim = interaction_dim // heads) or 'average'
    attention_hidden: List[int] = field(default_factory=lambda: [16])   # num_hidden_units_attention_fct
    aggregation_type: str = "sum"     # message_fn_chunk.py:16,57-62: 'sum' (tf.sparse.reduce_sum) or 'max' (tf.sparse.reduce_max)
    # update_fn_lstm.py:13-16,43-50: which tensors the four gates read besides x
    incorporate_hidden_features_in_update: bool = True
    incorporate_node_input_features_in_update: bool = True
    # graph_relation.py:141-172 assign_visual_features_to_edges: ROI features of every interaction's region, compressed like the
    # nodes' (same layer_compressed_dim per feature map), appended to the fed edge features
    visual_edges: bool = False
    # visual branch (GraphRelation image_input); 0 maps -> disabled
    visual_dims: List[int] = field(default_factory=list)   # layer_compressed_dim per feature map
    # feature_map_generation_params from_layer (layer_depth -1): backbone end points, e.g. scale_0_unet_up_2_conv
    visual_layers: List[str] = field(default_factory=list)
    mvn: bool = False                 # GraphRelation flag: per-image standardisation of the fed image
    backbone: dict = field(default_factory=dict)            # AruConfig fields of the ARU_v1 backbone (graph 'RU')
    # feature_map_generation_params layer_depth per map (feature_map_generators.py:72-197); empty = all -1.  -1: the end point itself.
    # d > 0 with a from_layer: that end point through a 1x1 conv to d/2 channels and a 3x3 conv to d channels.  d > 0 with from_layer '':
    # the same two convs over the previous map, the 3x3 at stride 2 (an SSD-style pyramid below the backbone)
    visual_layer_depths: List[int] = field(default_factory=list)

    def backbone_cfg(self) -> "AruConfig":
        kw = dict(graph="RU", apply_softmax=False)
        kw.update(self.backbone)
        kw["mvn"] = bool(kw.get("mvn", False) or self.mvn)
        if kw["graph"] == "RU_v2":
            raise ValueError("graph 'RU_v2' cannot be the relation net's backbone: RU_v2_CNN.infer returns no end points (RU_v2.py:31), and the "
                             "visual branch picks its feature maps from the backbone's end points by name (graph_relation.py:96-105)")
        return AruConfig(**kw)

    MAX_LAYER_DEPTH = 256             # widest generated map the engine serves (asep_gnn_attach_backbone_maps)

    def layer_depths(self) -> List[int]:
        """``visual_layer_depths`` per map (empty = all -1), checked against what the reference can build (``ValueError`` with the reason)"""
        depths = [int(d) for d in self.visual_layer_depths] or [-1] * len(self.visual_layers)
        if len(depths) != len(self.visual_layers):
            raise ValueError(f"visual_layer_depths has {len(depths)} entries for {len(self.visual_layers)} visual_layers "
                             "(feature_map_generators.py:130: from_layer and layer_depth have the same length)")
        for i, (name, d) in enumerate(zip(self.visual_layers, depths)):
            if not name and i == 0:
                raise ValueError("visual_layers[0] is empty: an empty from_layer shrinks the previous feature map and there is none "
                                 "(feature_map_generators.py:154)")
            if not name and d == -1:
                raise ValueError(f"visual_layers[{i}] is empty and its layer_depth is -1: an empty from_layer builds a new map and needs "
                                 "its depth (feature_map_generators.py:145-155)")
            if d == -1:
                continue
            if d <= 0 or d % 2:
                raise ValueError(f"layer_depth {d} of map {i}: a positive even depth is needed, layer_depth / 2 is the width of the 1x1 "
                                 "convolution (feature_map_generators.py:159-160)")
            if d > self.MAX_LAYER_DEPTH:
                raise ValueError(f"layer_depth {d} of map {i}: the engine serves generated maps of up to {self.MAX_LAYER_DEPTH} channels")
        return depths

    def _endpoint_channels(self, name: str) -> int:
        import re
        bc = self.backbone_cfg()
        m = re.fullmatch(r"scale_\d+_unet_(down|up)_(\d+)_(conv|deconv)", name)
        if not m or int(m.group(2)) >= bc.scale_space_num:
            raise ValueError(f"'{name}' is not a feature-map end point of the ARU_v1 backbone")
        return bc.feat(int(m.group(2)))

    def visual_channels(self) -> List[int]:
        """Channels of the feature maps: feat_root * 2^level for an end point (ARU_v1.py:208-292), layer_depth for a generated map."""
        return [self._endpoint_channels(name) if d == -1 else d for name, d in zip(self.visual_layers, self.layer_depths())]

    def visual_generators(self) -> List[dict]:
        """The generated maps in order: index, the channels read (``cin``), ``depth``, ``stride`` and the variable scopes of the two
        convolutions as the reference spells them -- f'{base}_1_Conv2d_{index}_1x1_{layer_depth / 2}' with Python's true division (a
        float: '3.0') and f'{base}_2_Conv2d_{index}_3x3_s2_{layer_depth}', base = the last from_layer that had depth -1, '' before any
        (feature_map_generators.py:133,147,159,164)."""
        out, base, chans = [], "", self.visual_channels()
        for i, (name, d) in enumerate(zip(self.visual_layers, self.layer_depths())):
            if d == -1:
                base = name
                continue
            out.append({"index": i, "cin": self._endpoint_channels(name) if name else chans[i - 1], "depth": d, "stride": 1 if name else 2,
                        "conv1": f"{base}_1_Conv2d_{i}_1x1_{d / 2}", "conv2": f"{base}_2_Conv2d_{i}_3x3_s2_{d}"})
        return out

    @property
    def heads(self) -> int:
        """message_fn_chunk.py:167-169: one head without attention"""
        return self.num_attention_heads if self.use_attention else 1

    @property
    def head_interaction_dim(self) -> int:
        """message_fn_chunk.py:68-72: x_dim of one head"""
        if self.use_attention and self.multihead_attention_merge_type == "concat":
            return self.interaction_dim // self.num_attention_heads
        return self.interaction_dim

    @property
    def output_type_code(self) -> int:
        """asep_gnn_cfg.output_type"""
        try:
            return {"hidden": 0, "add_final_hidden_and_input": 1, "concat_final_hidden_and_input": 2}[self.output_type]
        except KeyError:
            raise ValueError(f"output_type {self.output_type!r} (graph_gnn.py:23: hidden, add_final_hidden_and_input, "
                             f"concat_final_hidden_and_input)")

    @property
    def classifier_node_dim(self) -> int:
        """width of the node vectors the pair classifier concatenates"""
        return self.hidden_dim + (self.u_in_dim if self.output_type_code == 2 else 0)

    @property
    def u_in_dim(self) -> int:
        """width of the node features as fed (geometric + compressed visual dims)"""
        return self.node_feature_dim + sum(self.visual_dims)

    @property
    def u_dim(self) -> int:
        """width of the node features the message / update functions see"""
        return self.compress_node_feature_dim if self.compress_node_feature_dim > 0 else self.u_in_dim

    @property
    def visual_edge_dim(self) -> int:
        return sum(self.visual_dims) if self.visual_edges else 0

    @property
    def edge_in_dim(self) -> int:
        """width of the edge features the message function sees: fed (geometric) + compressed visual edge dims"""
        return self.edge_feature_dim + self.visual_edge_dim

    @property
    def aggregation_code(self) -> int:
        """asep_gnn_cfg.aggregation_type"""
        try:
            return {"sum": 0, "max": 1}[self.aggregation_type]
        except KeyError:
            raise ValueError(f"aggregation_type {self.aggregation_type!r} (message_fn_chunk.py:57-62: 'sum' or 'max')")

    @property
    def message_in_dim(self) -> int:
        return 4 * self.u_dim + self.edge_in_dim + 4 * self.hidden_dim

    @property
    def update_in_dim(self) -> int:
        return (self.message_out_dim + (self.hidden_dim if self.incorporate_hidden_features_in_update else 0)
                + (self.u_dim if self.incorporate_node_input_features_in_update else 0))

    @property
    def message_out_dim(self) -> int:
        """width of x (message_fn_chunk.py:229-241): heads * x_dim for 'concat', x_dim for 'average' / no attention"""
        if self.use_attention and self.multihead_attention_merge_type == "concat":
            return self.heads * self.head_interaction_dim
        return self.interaction_dim

    def to_dict(self):
        return asdict(self)
