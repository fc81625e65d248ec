/* asep_hip.h -- C ABI of libasep_hip.so: the MI355X (gfx950) replacement for the two
 * TensorFlow session calls on the article-separation hot path.
 *
 * The reference has no FFI of its own; its seam is two Python call sites that hand numpy arrays
 * to tf.Session.run.  Each entry point below names the reference call it replaces:
 *
 *   ARU-Net   article_separation/image_segmentation/net_post_processing/net_post_processing_helper.py
 *             :36-53  load_graph(path_to_pb)                    -> asep_aru_load
 *             :56-72  get_net_output(image, pb_graph, gpu)      -> asep_aru_forward[_dev]
 *             :75-78  apply_threshold + separator_net_post_processor.py:147 (uint8 truncation)
 *                                                               -> fused u8 outputs of asep_aru_forward
 *   GNN       article_separation/gnn/io.py:12-25 load_graph     -> asep_gnn_load
 *             article_separation/gnn/run_gnn_clustering.py:259-269 sess.run(
 *                 'output_belong_to_same_instance:0', feed_dict) -> asep_gnn_forward[_dev]
 *             article_separation/gnn/model/graph_util/misc.py:7-151
 *                 check_and_correct_interacting_nodes           -> asep_gnn_correct_edges
 *
 * Conventions: plain pointers and sizes; caller-owned buffers; 0 = success, negative = error
 * (text via asep_last_error()); no exceptions cross the ABI; one handle per (process, device);
 * a handle is re-entrant but must not be used concurrently from two threads.
 * Pointers named d_* are device (HBM) pointers; all others are host pointers.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 */
#ifndef ASEP_HIP_H
#define ASEP_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "asep_host_jpeg.h" /* asep_jpeg_info */

#ifdef __cplusplus
extern "C" {
#endif

#define ASEP_OK 0
#define ASEP_ERR_ARG -1
#define ASEP_ERR_HIP -2
#define ASEP_ERR_WEIGHTS -3
#define ASEP_ERR_UNSUPPORTED -4

/* ---- runtime ------------------------------------------------------------------------------- */
int asep_device_count(void);
int asep_init(int device_id);                 /* hipSetDevice + arch check (gfx950) */
const char* asep_last_error(void);
const char* asep_version(void);
/* Version of THIS header's struct layouts and signatures (ASEP_ABI_VERSION of the build).  A binding checks it once after
 * dlopen; independently of it every configuration struct starts with its own size in bytes (`struct_size`), and the load
 * functions refuse a struct whose size is not the one the library was built with -- a caller written against an older or newer
 * header gets ASEP_ERR_ARG + a message instead of fields read from whatever follows its struct on the stack.
 * An added function moves the version too: a binding resolves every name it declares when it loads the library. */
#define ASEP_ABI_VERSION 12
int asep_abi_version(void);
/* ABI 6: the environment switches this build of the library reads when a model is loaded (one name per line).
 * Anything else in the environment is not a switch: a caller that records the switches a measurement ran under (bench.py) filters
 * against this list, and the library names a set-but-ignored switch of an earlier round once on stderr. */
const char* asep_engine_switches(void);

/* Page-locked host memory.  The host-pointer entry points (asep_aru_forward, asep_gnn_forward ...) copy with
 * asynchronous transfers on one stream: from / to page-locked buffers these are DMAs at link speed, from / to ordinary
 * (pageable) memory the runtime stages them.  asep_host_alloc returns page-locked memory; asep_host_register page-locks
 * a range the caller already owns (e.g. a shared-memory slot that decoded pages arrive in). */
void* asep_host_alloc(size_t nbytes);
void asep_host_free(void* p);
int asep_host_register(void* p, size_t nbytes);
int asep_host_unregister(void* p);

/* ---- ARU-Net (ARU_v1.py:35-43 hyper-parameters) ---------------------------------------------- */
typedef struct asep_aru_cfg {
    int32_t struct_size;       /* = sizeof(asep_aru_cfg) of the header the caller was compiled / written against */
    int32_t channels;          /* image channels: 1 (gray), or 3 (R, G, B) for the graphs without attention (use_attention 0: RU, U) */
    int32_t n_classes;
    int32_t feat_root;         /* 8 */
    int32_t scale_space_num;   /* 5 */
    int32_t res_depth;         /* 3 */
    int32_t num_scales_att;    /* 3; 0/1 with use_attention=0 */
    int32_t use_attention;     /* graph contains 'ARU' */
    int32_t mvn;               /* per-image standardisation of the input */
    int32_t apply_softmax;     /* export-time class softmax */
    int32_t compute_dtype;     /* 0 = fp32 (f32 MFMA), 1 = bf16 tensors + bf16 MFMA with fp32 accumulation, 2 = fp32 tensors and accumulation with
                                  SPLIT products: x = xh + xm + xl, w = wh + wm + wl (bfloat16 parts, exact), x w as the six largest of the nine
                                  bf16 products on the bf16 MFMA (dropped terms <= 2^-23 |x w|): fp32 results, the fp32 parity gates */
    int32_t activation;        /* ARU_v1.py:70-75 activation_name: 0 = relu, 1 = elu, 2 = leaky (leak 0.1, layers.py:10-30).  It is the
                                  activation of the convR / conv2 layers, of the block ends, the deconvolutions and the attention CNN; the
                                  ReLU between conv1 and convR_0 of a residual block is a ReLU in every variant (ARU_v1.py:214,268) */
    int32_t plain_u;           /* 1 = graph 'U' (ARU_v1.py:228-233,283-288): every block is conv1 + conv2 with the activation, no
                                  residual add, tensors <block>/conv2/{weights,biases} instead of convR_<i>; 0 = residual blocks (RU / ARU) */
    int32_t input_pyramid;     /* ABI 10: 1 = graph RU_v2 (RU_v2.py): the residual U-Net whose down blocks l >= 1 read concat[pool(d_{l-1}), I_l],
                                  I_l = the page average-pooled l times (2x2, stride 2, SAME).  The tensors carry the reference's names
                                  ru_net/featMapG/..., ru_net/logit/class/...; conv1 of those blocks is [3,3,f_{l-1} + channels,f_l], the image
                                  rows last.  Needs use_attention 0, plain_u 0 and compute_dtype 0 or 2; publishes the end point "logits" */
    int32_t inp4up;            /* with input_pyramid (RU_v2.py:13,143): 1 = the up blocks read concat[skip, deconv, I_l], conv1 [3,3,2 f_l + channels,f_l] */
} asep_aru_cfg;

typedef struct asep_aru asep_aru;

/* weight_blob: "ASEPW001" container (see citlab-article-separation-new_amd/weights.py) holding
 * the tensors of ARU_v1.py under the reference's variable-scope names. */
asep_aru* asep_aru_load(const void* weight_blob, size_t nbytes, const asep_aru_cfg* cfg);
void asep_aru_free(asep_aru* m);

/* Page layout of every asep_aru_forward* entry point: H*W*channels floats, row major, the channels of a pixel interleaved ([H,W] for a gray
 * net, [H,W,3] in R, G, B order for cfg.channels == 3), values as fed to 'inImg:0'.  With cfg.mvn the page is standardised with the mean and
 * the standard deviation of all H*W*channels values (layers.py:672-711).  asep_aru_load refuses cfg.channels == 3 together with
 * use_attention (ARU_v1.py:115 upsamples the attention map to the input's shape with a one-channel filter) and every other channel count.
 *
 * Host-buffer call == get_net_output(): img_hw is H*W*channels floats (row major, values as fed to
 * 'inImg:0'); out_hwc receives H*W*n_classes floats ('output:0'[0]).  The optional u8 outputs are
 * the two consumers that directly follow the net in the reference:
 *   out_u8   = uint8(prob*255)               (truncation, separator_net_post_processor.py:147)
 *   out_mask = (out_u8 > threshold*255)*255  (net_post_processing_helper.py:75-78)
 * Pass NULL to skip either. */
int asep_aru_forward(asep_aru* m, const float* img_hw, int H, int W,
                     float* out_hwc, uint8_t* out_u8, uint8_t* out_mask, float threshold);

/* Device-resident variant (input and outputs already in HBM); asynchronous on `stream`. */
int asep_aru_forward_dev(asep_aru* m, const float* d_img, int H, int W,
                         float* d_out, uint8_t* d_out_u8, uint8_t* d_out_mask, float threshold,
                         void* stream);

/* A batch of n_pages equally sized device-resident pages in one call (BASELINE configs[1]: "batch of
 * 3000x4500 px full pages").  Every layer is launched once for all pages and scale-space levels, which keeps
 * the coarse levels from under-filling the 256 CUs.  d_imgs / d_outs / d_out_u8 / d_out_mask are host arrays
 * of n_pages device pointers (the u8 arrays themselves may be NULL). */
int asep_aru_forward_batch_dev(asep_aru* m, int n_pages, const float* const* d_imgs, int H, int W,
                               float* const* d_outs, uint8_t* const* d_out_u8, uint8_t* const* d_out_mask,
                               float threshold, void* stream);
/* ABI 6: asep_aru_forward_batch_dev for pages of DIFFERENT sizes: H[b] x W[b] is page b's size, d_imgs[b] / d_outs[b] / d_out_u8[b] /
 * d_out_mask[b] its buffers ([H[b], W[b](, 3)] fp32 in; [H[b], W[b], n_classes] out).  Replaces the reference's page-by-page loop over scans of
 * arbitrary size (run_net_post_processing.py:61-82 -> get_net_output per scan, ARU_v1.py:64 `inImg` [1, None, None, 1]); results are those
 * of the single-page calls bit for bit.  The pages of a call share every layer's launches. */
int asep_aru_forward_batch_dev2(asep_aru* m, int n_pages, const float* const* d_imgs, const int32_t* H, const int32_t* W,
                                float* const* d_outs, uint8_t* const* d_out_u8, uint8_t* const* d_out_mask, float threshold,
                                void* stream);

/* Named intermediate tensors of the last forward (tests / GNN visual branch): copies the NHWC fp32
 * tensor `name` (e.g. "scale_0_unet_up_0_conv", ARU_v1.py:11-29 end-point names) to host.
 * Returns the number of floats written, or a negative error; dims receives {H, W, C}. */
long asep_aru_get_endpoint(asep_aru* m, const char* name, float* out, size_t max_floats, int32_t dims[3]);

/* ABI 6: release the handle's device arenas (intermediate tensors of the largest call served so far: ~6 GB per 3000 x 4500 fp32 page in flight);
 * the next forward call rebuilds them.  For a process that keeps a model loaded while another GPU process of its size runs beside it. */
int asep_aru_trim(asep_aru* m);

/* Per-launch timing with HIP events recorded on the launch stream (measurement aid for bench.py).
 * asep_aru_profile(m,1) clears the records and starts recording; (m,0) stops.  Mode 1 serialises the net on the
 * launch stream (isolated kernel times), mode 2 additionally names every layer, mode 3 keeps the attention side
 * stream running ("in situ": what rocprofv3 sees in the real schedule).  The report is a JSON array
 * [{"kernel","calls","total_ms","flops"}] aggregated per kernel, "kernel" being the rocprofv3 name without
 * "void ", "asep::", blanks and the argument list; returns its length. */
int asep_aru_profile(asep_aru* m, int enable);
long asep_aru_profile_report(asep_aru* m, char* buf, size_t buflen);

/* Algorithmic FLOPs (2*MAC of conv/deconv layers) of one forward at H x W. */
double asep_aru_flops(const asep_aru* m, int H, int W);

/* Blocks of the f32s level-0 strip walker (res8ws_kernel<up != 0>, one wave each) that the runtime keeps resident on a compute unit
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor); negative on error. */
int asep_aru_walker_occupancy(int up);

/* ---- GNN relation predictor ------------------------------------------------------------------ */
typedef struct asep_gnn_cfg {
    int32_t struct_size;           /* = sizeof(asep_gnn_cfg) of the header the caller was compiled / written against */
    int32_t node_feature_dim;      /* u (after masking), e.g. 7 */
    int32_t edge_feature_dim;      /* e, e.g. 2; counts the fed (geometric) + compressed visual edge dims (visual_edge_dims) */
    int32_t num_transition_steps;  /* 3 */
    int32_t hidden_dim;            /* 32 (any width; the fused MFMA kernels serve 32/32/32) */
    int32_t interaction_dim;       /* 32 */
    int32_t interaction_hidden;    /* first hidden layer of the interaction MLP (32); further layers: interaction_hidden2..4 below */
    int32_t cls_hidden1;           /* classifier num_hidden_units (graph_relation.py:196), first entry: 64 (64,32 -> 2 has a specialised kernel) */
    int32_t cls_hidden2;           /* 32; 0 = the classifier has ONE hidden layer */
    int32_t num_classes;           /* 2 (<= 16) */
    int32_t undirected_graph;      /* 1 */
    int32_t compress_input_dim;    /* graph_gnn.py:20,102-109 compress_node_feature_dim: 0 = off; > 0: node features are FED with this
                                      width and go through tanh(W x + b) (GraphLSTM1/compress_input/ff_compress_input/{weights,bias})
                                      to node_feature_dim before the message passing */
    int32_t output_type;           /* graph_gnn.py:23,158-166: 0 = 'hidden' (the classifier reads the final hidden states), 1 =
                                      'add_final_hidden_and_input' (h += x W, GraphLSTM1/dense/weights [fed width, hidden], no bias), 2 =
                                      'concat_final_hidden_and_input' (the classifier reads [h | x]: its first layer has 2 (hidden + fed
                                      width) rows); x = the node features AS FED (before compress_input) */
    int32_t attention_heads;       /* message_fn_chunk.py:35-41 use_attention: 0 = off (degree-normalised sum, the reference's default);
                                      k >= 1 = learned attention with k heads (head_<i>/calculation_interaction_features/... and
                                      head_<i>/calculation_unnormalized_attention_values/... MLPs); the reference's chunking of the
                                      interactions by target-node ranges (message_fn_chunk.py:76-110) is reproduced */
    int32_t attention_merge;       /* multihead_attention_merge_type: 0 = 'concat' (x_dim = interaction_dim / heads), 1 = 'average' */
    int32_t attention_hidden;      /* num_hidden_units_attention_fct, first entry (16); further layers: attention_hidden2..4 below */
    /* ---- ABI 5 ---- */
    int32_t aggregation_type;      /* message_fn_chunk.py:16,57-62: 0 = 'sum' (tf.sparse.reduce_sum, the default), 1 = 'max'
                                      (tf.sparse.reduce_max over the stored entries: a node without in-edges gets 0) */
    int32_t interaction_hidden2;   /* num_hidden_units_interaction_fct is a list (message_fn_chunk.py:24): entries 2..4, 0 = absent */
    int32_t interaction_hidden3;
    int32_t interaction_hidden4;
    int32_t attention_hidden2;     /* num_hidden_units_attention_fct entries 2..4 (message_fn_chunk.py:40), 0 = absent */
    int32_t attention_hidden3;
    int32_t attention_hidden4;
    int32_t cls_hidden3;           /* classifier hidden layers 3, 4; 0 = absent */
    int32_t cls_hidden4;
    int32_t lstm_use_hidden;       /* update_fn_lstm.py:13-16,43-50 incorporate_hidden_features_in_update (default 1): h is an input of the gates */
    int32_t lstm_use_input;        /* incorporate_node_input_features_in_update (default 1): the node features are an input of the gates */
    int32_t visual_edge_dims;      /* graph_relation.py:141-172 assign_visual_features_to_edges: total width of the compressed visual EDGE
                                      features (ROI max over the backbone end points of every interaction's region ->
                                      visual_edge_feature_compression_fm_<i>/dense) appended to the fed edge features; 0 = off */
} asep_gnn_cfg;

typedef struct asep_gnn asep_gnn;

asep_gnn* asep_gnn_load(const void* weight_blob, size_t nbytes, const asep_gnn_cfg* cfg);
void asep_gnn_free(asep_gnn* g);

/* misc.py:7-151 on the device: symmetrise (if undirected), de-duplicate, drop self loops, sort by
 * from*N+to, first-occurrence edge features.  out_edges must hold 2*E*2 ints, out_feat 2*E*e
 * floats (may be NULL).  Returns E' (>= 0) or a negative error. */
int asep_gnn_correct_edges(asep_gnn* g, int N, int E, const int32_t* edges, const float* edge_feat,
                           int32_t* out_edges, float* out_feat);

/* One page: == sess.run('output_belong_to_same_instance:0', feed_dict) at batch size 1.
 *   edges [E,2] (from,to), node_feat [N,u], edge_feat [E,e], relations [R,2] -> probs_out [R,num_classes].
 * relations == NULL means "all N*N ordered pairs, row major" (input_dataset.py:444-457). */
int asep_gnn_forward(asep_gnn* g, int N, int E, const int32_t* edges, const float* node_feat,
                     const float* edge_feat, int R, const int32_t* relations, float* probs_out);

int asep_gnn_forward_dev(asep_gnn* g, int N, int E, const int32_t* d_edges, const float* d_node_feat,
                         const float* d_edge_feat, int R, const int32_t* d_relations, float* d_probs_out,
                         void* stream);

/* Final hidden node states h [N, hidden_dim] of the last forward (tests). */
int asep_gnn_get_hidden(asep_gnn* g, float* out, size_t max_floats);

double asep_gnn_flops(const asep_gnn* g, int N, int E_corrected, int R);

/* Visual node features (graph_relation.py:84-139 with image_input; misc.py:272-381): `backbone` is an ARU-Net
 * handle loaded from the `aru_net/...` tensors of the same frozen graph (graph 'RU'/'ARU', mvn per the GNN's flag,
 * apply_softmax 0); endpoint_names are the `feature_map_generation_params from_layer` entries (layer_depth -1),
 * e.g. "scale_0_unet_up_2_conv".  The compression layers visual_node_feature_compression_fm_<i>/dense/{weights,bias} come from
 * the GNN's own weight blob.  cfg.node_feature_dim counts geometric + compressed visual dims (e.g. 7 + 3*16).
 * The backbone may be loaded with compute_dtype 1 (bf16, BASELINE configs[4]): the ROI kernel then reads its bf16 end points;
 * compression layers, graph and classifier stay fp32. */
int asep_gnn_attach_backbone(asep_gnn* g, asep_aru* backbone, int n_maps, const char* const* endpoint_names);

/* ABI 8: the same with the whole `feature_map_generation_params` layout (feature_map_generators.py:72-197): layer_depths[i] is the
 * `layer_depth` of map i (NULL = all -1 = asep_gnn_attach_backbone).  -1: the end point endpoint_names[i] itself.  d > 0 with a name: that end
 * point through a 1x1 convolution to d/2 channels and a 3x3 convolution to d channels, stride 1.  d > 0 with the EMPTY name "": the same two
 * convolutions over map i - 1, the 3x3 at stride 2 (TensorFlow's SAME: ceil(n/2) cells, an even side pads 0 in front and 1 behind).  All
 * convolutions have a bias and a ReLU; fp32 operands and accumulation.  Their variables come from the GNN's weight blob under the reference's
 * names, <base>_1_Conv2d_<i>_1x1_<d/2>.0/{weights,biases} and <base>_2_Conv2d_<i>_3x3_s2_<d>/{weights,biases}, <base> being the last name
 * with depth -1 in front of map i ("" before any).  Refused with the reason: "" in position 0, "" with depth -1, an odd or non-positive depth,
 * a depth above 256.  The generated maps live in the handle (sized at the first forward of a page size, freed by the next attach); the
 * compression layer of a generated map is [d, layer_compressed_dim]. */
int asep_gnn_attach_backbone_maps(asep_gnn* g, asep_aru* backbone, int n_maps, const char* const* endpoint_names,
                                  const int32_t* layer_depths);

/* Feature map `index` of the last asep_gnn_forward_visual* as fp32 [fh, fw, C] (a batch call: of its last page), generated or not; a
 * bf16 end point is widened.  dims receives {fh, fw, C}; out == NULL asks for the sizes only.  Waits for the forward's stream (tests). */
int asep_gnn_get_feature_map(asep_gnn* g, int index, float* out, size_t max_floats, int32_t dims[3]);

/* run_gnn_clustering.py:259-269 with the image feeds: node_feat [N, node_feature_dim - visual dims],
 * image float32 [h,w] -- [h,w,3] in R, G, B order when the attached backbone reads three channels (a net trained with load_mode=RGB,
 * input_dataset.py:42-49) -- (0..255 as fed, input_dataset.py:279-280), regions [N,2,P] relative coordinates (row 0 = x,
 * row 1 = y), num_points [N].  Backbone -> ROI max -> compression -> concat -> GNN -> probabilities [R, classes].
 * edge_regions [E,2,P] / edge_num_points [E] ('visual_regions_edges', 'num_points_visual_regions_edges'): the regions of the
 * interactions of a graph exported with assign_visual_features_to_edges (cfg.visual_edge_dims > 0; NULL otherwise): their
 * compressed ROI maxima are appended to edge_feat [E, edge_feature_dim - visual_edge_dims] BEFORE the edge correction, which
 * keeps the first occurrence's features like every other edge feature. */
int asep_gnn_forward_visual(asep_gnn* g, int N, int E, const int32_t* edges, const float* node_feat,
                            const float* edge_feat, const float* image, int h, int w, const float* regions, int P,
                            const int32_t* num_points, const float* edge_regions, const int32_t* edge_num_points,
                            int R, const int32_t* relations, float* probs_out);

/* The same with every array already in HBM (image [h,w] or [h,w,3] float32 included), launched on `stream` without any host
 * synchronisation: backbone, ROI kernels and the graph are queued back to back.  Index arrays are not validated here:
 * an edge that names a node outside 0..N-1 is ignored, a relation that does yields NaN probabilities. */
int asep_gnn_forward_visual_dev(asep_gnn* g, int N, int E, const int32_t* d_edges, const float* d_node_feat,
                                const float* d_edge_feat, const float* d_image, int h, int w, const float* d_regions,
                                int P, const int32_t* d_num_points, const float* d_edge_regions,
                                const int32_t* d_edge_num_points, int R, const int32_t* d_relations,
                                float* d_probs_out, void* stream);

/* A batch of pages through the visual net (bench.py's step; a GPU owner that holds several decoded pages): the backbones
 * of all pages run as ONE grouped forward (asep_aru_forward_batch_dev: every layer is one launch over the page list, so the
 * small 683 x 1024 images fill the chip together), then ROI kernels + graph per page, all queued on `stream`, no host
 * synchronisation.  Every image is [h,w] (colour backbone: [h,w,3]) float32 and every region array [N,2,P]; the other sizes are per page.
 * asep_gnn_get_node_features afterwards returns page 0's features. */
typedef struct asep_gnn_page {
    int32_t N, E, R;
    const int32_t* d_edges;        /* [E,2] */
    const float* d_node_feat;      /* [N, node_feature_dim - visual dims] */
    const float* d_edge_feat;      /* [E, edge_feature_dim] */
    const float* d_image;          /* [h,w], or [h,w,3] for a 3-channel backbone */
    const float* d_regions;        /* [N,2,P] */
    const int32_t* d_num_points;   /* [N] */
    const float* d_edge_regions;   /* [E,2,P] or NULL (cfg.visual_edge_dims == 0) */
    const int32_t* d_edge_num_points; /* [E] or NULL */
    const int32_t* d_relations;    /* [R,2] or NULL = all N*N ordered pairs (then R must be N*N) */
    float* d_probs_out;            /* [R, num_classes] */
} asep_gnn_page;
int asep_gnn_forward_visual_batch_dev(asep_gnn* g, int n_pages, const asep_gnn_page* pages, int h, int w, int P,
                                      void* stream);

/* ABI 9: asep_gnn_forward_visual_batch_dev for pages of DIFFERENT image sizes: h[b] x w[b] is page b's image size (pages[b].d_image is
 * [h[b], w[b]] or [h[b], w[b], 3]); everything else as above.  What the reference's input pipeline leaves after its ratio-preserving resize
 * (image_resizer.py: max side 1024, min side 256) differs from scan to scan, and the reference runs page by page (run_gnn_clustering.py:259-269).
 * The backbones run as ONE grouped forward over the page list (asep_aru_forward_batch_dev2's launches: nothing is padded to a common frame).
 * Each of the stages below then runs as ONE launch over a page table in device memory, whatever the pages' sizes; the graphs follow page by
 * page:
 *   - the two convolutions of every generated feature map;
 *   - ROI max + compression of all node and interaction regions.
 *   - the per-image moments of the backbone's standardisation (mean and variance over the page's own h[b] x w[b] values, sd floor 1e-4);
 *   - with the u8 entry below, the TF1 bilinear resize of all scans.
 * Per page the results are those of asep_gnn_forward_visual_dev bit for bit.  Refused with ASEP_ERR_ARG and a message that names the page,
 * before anything is queued: n_pages < 1, a NULL size array, a non-positive size, a page with a missing array, and -- where the entry can
 * know it, i.e. in the u8 entry -- a page whose image channels do not match the backbone.  An asep_gnn_page carries no channel count: as
 * in every float entry, d_image must hold h[b] * w[b] * (the backbone's channels) values.  (What depends on the queued backbone's end points --
 * an end point of another channel count than the attached layout -- is refused behind the backbone forward.)
 * Everything is queued on `stream`; the one host wait is on the table buffer a call reuses, whose readers were queued four calls back
 * (free unless the caller runs that far ahead of the device; it rules these two entries out of a stream capture).
 * The handle's arenas and table buffers keep the largest call served so far.  Like every entry of a handle, successive calls go to one
 * stream, or the caller orders them.  Afterwards asep_gnn_get_node_features / asep_gnn_get_feature_map behave as after the old entry;
 * the asep_gnn_get_page_* functions read any page of the call, until the handle's next forward (the addresses they read, backbone end
 * points included, belong to that call). */
int asep_gnn_forward_visual_batch_dev2(asep_gnn* g, int n_pages, const asep_gnn_page* pages, const int32_t* h, const int32_t* w, int P,
                                       void* stream);
/* The same fed with the scans as decoded: page.d_image is not read; d_scan is uint8 [src_h, src_w, src_c], src_c = 1 or 3 (R, G, B), and is
 * resized to h[b] x w[b] on the device (asep_prep_resize_tf1_dev's bytes, all pages in one launch): src_c equal to the backbone's channels
 * keeps every channel, src_c = 3 into a gray backbone takes Pillow's luma per tap, anything else is the channel mismatch above. */
typedef struct asep_gnn_page_u8 {
    asep_gnn_page page;
    const uint8_t* d_scan;
    int32_t src_h, src_w, src_c;
} asep_gnn_page_u8;
int asep_gnn_forward_visual_batch_u8_dev(asep_gnn* g, int n_pages, const asep_gnn_page_u8* pages, const int32_t* h, const int32_t* w, int P,
                                         void* stream);
/* Read-back of page `page` of the handle's last call of the two entries above (tests): the concatenated node features [N, node_feature_dim],
 * feature map `index` as fp32 [fh, fw, C] (dims receives the sizes, out == NULL asks for them only), and after the u8 entry the resized
 * image [h, w, C].  Each waits for the call's stream. */
int asep_gnn_get_page_node_features(asep_gnn* g, int page, float* out, size_t max_floats);
int asep_gnn_get_page_feature_map(asep_gnn* g, int page, int index, float* out, size_t max_floats, int32_t dims[3]);
int asep_gnn_get_page_image(asep_gnn* g, int page, float* out, size_t max_floats, int32_t dims[3]);

/* ABI 12: the GRAPH part (edge correction, message passing, LSTM update, pair classifier) of n_pages pages in one call, each stage one launch
 * over all pages, for graphs WITHOUT visual features (a handle with a backbone attached or with visual_edge_dims is refused with a message
 * that names asep_gnn_forward_visual_batch_dev2).  N / E / R [n_pages] are host arrays; the other inputs hold the pages one behind the other:
 * node features [sum N, node_feature_dim], edges [sum E, 2] with PAGE-LOCAL node numbers, edge features [sum E, edge_feature_dim],
 * relations [sum R, 2] page-local (NULL: R_b <= N_b^2 ordered pairs of page b row major).  probs_out receives the class-1 probability of
 * every relation, sum R floats in page order (max_floats: what the buffer holds); per page the values are those of asep_gnn_forward[_dev] on
 * the page alone bit for bit, whatever else shares the call.  Refused before anything is uploaded or launched, with "... in page %d" where a
 * page is at fault: NULL arrays, N_b < 1, E_b / R_b < 0, N_b^2 > 2^30 and a sum of N_b^2 over the call > 2^30 (ASEP_ERR_UNSUPPORTED: split
 * the call), a too-small output buffer, and in the host entry an edge or relation that names a node outside 0..N_b-1 (the device entry does
 * with those what asep_gnn_forward_dev does: the edge is ignored, the relation is NaN).  The calls of a handle go to one stream, or the
 * caller orders them.  Afterwards asep_gnn_get_hidden returns the hidden states of all pages [sum N, hidden_dim] in page order,
 * asep_gnn_get_page_hidden those of one page, asep_gnn_get_page_edges one page's corrected edge list as asep_gnn_correct_edges returns it
 * (out_first, optional: the index into the page's symmetrised list of every edge's first occurrence; returns the count), until the
 * handle's next forward.  asep_gnn_batch_launches: the kernels the handle's last batched call launched (0: it was refused). */
int asep_gnn_forward_batch(asep_gnn* g, int n_pages, const int32_t* N, const int32_t* E, const int32_t* R, const float* node_feat,
                           const int32_t* edges, const float* edge_feat, const int32_t* relations, float* probs_out, size_t max_floats);
int asep_gnn_forward_batch_dev(asep_gnn* g, int n_pages, const int32_t* N, const int32_t* E, const int32_t* R, const float* d_node_feat,
                               const int32_t* d_edges, const float* d_edge_feat, const int32_t* d_relations, float* d_probs_out,
                               size_t max_floats, void* stream);
int asep_gnn_get_page_hidden(asep_gnn* g, int page, float* out, size_t max_floats);
int asep_gnn_get_page_edges(asep_gnn* g, int page, int32_t* out_edges, int32_t* out_first, int max_edges);
long asep_gnn_batch_launches(const asep_gnn* g);

/* Which message-passing kernel the handle uses: 0 = generic FMA kernels (any widths), 1 = fused MFMA step with the
 * edge-MLP filter in registers (widths 32, node_feature_dim <= 8), 2 = fused MFMA step with the filter in LDS (widths 32,
 * node_feature_dim <= 120: the visual nets), 3 (ABI 6, the default wherever 1 or 2 would serve) = the FACTORED fused step: the per-node
 * terms of the edge MLP's first layer once per node, its step-independent per-edge term once per page, K = 32 per edge and step
 * (ASEP_GNN_FACTOR=0 keeps 1 / 2). */
int asep_gnn_step_mode(const asep_gnn* g);

/* Concatenated node features [N, node_feature_dim] of the last asep_gnn_forward_visual[_dev] (tests). */
int asep_gnn_get_node_features(asep_gnn* g, float* out, size_t max_floats);

/* ---- classical image stages around the ARU-Net ---------------------
 * The reference runs these on the host with OpenCV; here they are byte / bit kernels next to the nets so that a
 * page never leaves HBM between decode and polygon extraction.  Binary images: 0 = background, non-zero =
 * foreground on input; 0 / 255 on output.  One workspace handle per (process, device); buffers grow on demand. */
typedef struct asep_post asep_post;
asep_post* asep_post_create(void);
void asep_post_free(asep_post* p);

/* net_post_processing_helper.py:14-33 (scale_image + cvtColor(BGR2GRAY)/255.0) without the file decode.
 * img: uint8 [H,W,C] with C = 3 (BGR) or 1 (gray).  sc < 1: cv2 INTER_AREA, sc > 1: INTER_CUBIC, sc == 1: copy.
 * Output size (round-half-even of H*sc, W*sc) is returned by asep_prep_scaled_size.
 * out_image (optional): uint8 [h,w,C]; out_gray: float32 [h,w] = gray/255 (the net input). */
int asep_prep_scaled_size(int H, int W, double sc, int32_t* out_h, int32_t* out_w);
int asep_prep_scale_gray(asep_post* p, const uint8_t* img, int H, int W, int C, double sc,
                         uint8_t* out_image, float* out_gray);
int asep_prep_scale_gray_dev(asep_post* p, const uint8_t* d_img, int H, int W, int C, double sc,
                             uint8_t* d_out_image, float* d_out_gray, void* stream);

/* ABI 7: gnn_input.resize_bilinear_tf1 (image_resizer.py:111-223: tf.image.resize BILINEAR of TF 1.x, align_corners False) from the uint8
 * scan, for the relation net's page image (input_dataset.py:279-283): src = dst * (in / out) in float32 with the factors
 * float32(H / h), float32(W / w), no half-pixel offset, taps clamped at the border, every product and sum rounded on its own --
 * the host function's result bit for bit.  img: uint8 [H,W,C], C = 1 or 3; h, w: the target size, which the caller computes
 * (gnn_input.compute_new_size).  mode ASEP_RESIZE_KEEP: every channel on its own -> out float32 [h,w] or [h,w,3], interleaved order
 * kept.  ASEP_RESIZE_LUMA (C = 3 in R, G, B order only): each tap first becomes Pillow's convert('L') value
 * (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 -> out float32 [h,w]: a colour scan for a gray backbone.  Values 0..255 as fed to
 * 'image:0'.  The _dev form takes device pointers and queues one kernel on `stream`, nothing is synchronised. */
#define ASEP_RESIZE_KEEP 0
#define ASEP_RESIZE_LUMA 1
int asep_prep_resize_tf1(asep_post* p, const uint8_t* img, int H, int W, int C, int mode, int h, int w, float* out);
int asep_prep_resize_tf1_dev(asep_post* p, const uint8_t* d_img, int H, int W, int C, int mode, int h, int w, float* d_out,
                             void* stream);

/* region_net_post_processor_base.py:230-251 apply_cc_analysis: drop 8-connected components whose pixel count is
 * below min_size (the caller evaluates int(size * threshold) in double like the reference).
 * mask: uint8 [H,W,pix_stride], channel `channel` is used. */
int asep_post_cc_filter(asep_post* p, const uint8_t* mask, int H, int W, int pix_stride, int channel,
                        int min_size, uint8_t* out);

/* cv2.erode / dilate / morphologyEx(MORPH_OPEN | MORPH_CLOSE) with a kw x kh rectangle, default anchor
 * (kw/2, kh/2), default constant border; op: 0 erode, 1 dilate, 2 open, 3 close. */
int asep_post_morph_rect(asep_post* p, int op, const uint8_t* mask, int H, int W, int kw, int kh, uint8_t* out);

/* separator_net_post_processor.py:26-97 post_process: CC filter, horizontal opening (k_h x 1), vertical opening
 * (1 x k_v), horizontal minus vertical, clean-up opening (k_clean x 1).  mask: uint8 [H,W,pix_stride] (the
 * thresholded net output, channel 0 is the separator class).  Outputs uint8 [H,W] each. */
int asep_post_separator(asep_post* p, const uint8_t* mask, int H, int W, int pix_stride, int channel,
                        int min_size, int k_h, int k_v, int k_clean, uint8_t* out_horizontal,
                        uint8_t* out_vertical);
int asep_post_separator_dev(asep_post* p, const uint8_t* d_mask, int H, int W, int pix_stride, int channel,
                            int min_size, int k_h, int k_v, int k_clean, uint8_t* d_out_horizontal,
                            uint8_t* d_out_vertical, void* stream);

/* Device half of region_net_post_processor_base.py:186-197 (rasterio.features.shapes): the boundary of the pixels
 * equal to `value` as maximal straight segments, each directed with the foreground on its right (heading 0 = +x top
 * sides, 1 = +y right sides, 2 = -x bottom sides, 3 = -y left sides).  out_starts / out_ends receive the keys
 * ((vy*(W+1)+vx)*4 + heading) of the start / end vertices in arbitrary order; segments of one heading on one grid
 * line are disjoint, so after sorting both arrays per heading the k-th start pairs with the k-th end.  Returns the
 * number of segments (may exceed `capacity`: call again with larger buffers) or a negative error.  The host chains
 * the segments into exterior / interior rings (polygonize.py). */
long asep_post_boundary_segments(asep_post* p, const uint8_t* mask, int H, int W, int value, int32_t* out_starts,
                                 int32_t* out_ends, long capacity);
long asep_post_boundary_segments_dev(asep_post* p, const uint8_t* d_mask, int H, int W, int value, int32_t* d_starts,
                                     int32_t* d_ends, long capacity, void* stream);
/* The same without the host round trip, for a caller that keeps more than one page in flight: the kernel is
 * enqueued on `stream` and the two counts (starts, ends; equal on success, either may exceed `capacity`) are left in
 * d_totals[0..1] (device memory, caller-owned).  Nothing is synchronised: the caller copies d_totals and the first
 * min(total, capacity) keys back in stream order and falls back to asep_post_boundary_segments_dev with larger
 * buffers when total > capacity. */
int asep_post_boundary_segments_enqueue_dev(asep_post* p, const uint8_t* d_mask, int H, int W, int value,
                                            int32_t* d_starts, int32_t* d_ends, long capacity,
                                            unsigned long long* d_totals, void* stream);

/* cv2.imread(path, IMREAD_GRAYSCALE) of an image that is already decoded and on the device (swt_dist_trafo.py:19):
 * d_bgr uint8 [H,W,3] in B,G,R order -> d_out uint8 [H,W] with OpenCV's fixed-point weights
 * (B*3735 + G*19235 + R*9798 + 16384) >> 15.  Enqueued on `stream`, nothing is synchronised. */
int asep_prep_gray_u8_dev(asep_post* p, const uint8_t* d_bgr, int H, int W, uint8_t* d_out, void* stream);

/* heading_net_post_processor.py:247-270 (get_net_prob_for_text_line) without the net output leaving the device:
 * out_sums[i] = sum of d_img[y0:y1, x0:x1, channel] over box i = {x0, y0, x1, y1} (clipped to the image like a numpy
 * slice with non-negative bounds), d_img uint8 [H,W,pix_stride].  Exact integers; the caller divides by 255 and by
 * the nominal box size.  boxes and out_sums are host pointers; returns after the sums have arrived. */
int asep_post_box_sums_dev(asep_post* p, const uint8_t* d_img, int H, int W, int pix_stride, int channel, int n_boxes,
                           const int32_t* boxes, int64_t* out_sums, void* stream);

/* swt_dist_trafo.py:18-29 distance_transform without the file decode: gray uint8 [H,W] -> 255-gray ->
 * GaussianBlur 5x5 -> Otsu -> exact Euclidean distance to the nearest zero pixel -> astype(uint8).
 * out_otsu (optional) receives the Otsu threshold; out_d2 (optional) the exact squared distances (int32). */
int asep_swt_distance_transform(asep_post* p, const uint8_t* gray, int H, int W, uint8_t* out,
                                int32_t* out_otsu, int32_t* out_d2);
int asep_swt_distance_transform_dev(asep_post* p, const uint8_t* d_gray, int H, int W, uint8_t* d_out,
                                    void* stream);

/* heading_net_post_processor.py:218-245 / feature_generation.py:106-159 for all text lines of a page at once.
 * swt: the uint8 distance-transform image [H,W]; boxes: n_lines x {x0, y0, x1, y1} = the crop swt[y0:y1, x0:x1]
 * the reference takes per line (numpy slicing: bounds are clipped to the image).  Per line: 8-connected components
 * of the non-zero crop pixels (connected_components_cv), size / aspect cleaning (clean_connected_components),
 * the crop's maximum over each surviving component's bounding box; out_stroke_width = median of those maxima
 * (0.0 if none), out_height = largest surviving component height.  out_flag[i] = 1 marks a line with more than
 * 1024 components whose results were not computed (the caller evaluates that line on the host).
 * boxes and the three outputs are host pointers in both variants. */
int asep_swt_line_features(asep_post* p, const uint8_t* swt, int H, int W, int n_lines, const int32_t* boxes,
                           float* out_stroke_width, int32_t* out_height, int32_t* out_flag);
int asep_swt_line_features_dev(asep_post* p, const uint8_t* d_swt, int H, int W, int n_lines, const int32_t* boxes,
                               float* out_stroke_width, int32_t* out_height, int32_t* out_flag, void* stream);

/* ---- text block detection (baseline DBSCAN and alpha-shape regions, SURVEY.md "text block detection") ----------------
 * Batched over pages on the asep_post handle.  Polygons are concatenated page after page: page k holds the polygons
 * page_off[k] .. page_off[k+1]-1 (page_off[0] = 0).  Host pointers in and out; each call returns after its results
 * have arrived.
 *
 * dbscan_baselines.py:35-110 get_list_of_interline_distances (use_java_code=False) on NORMED baselines, bit for bit:
 * polygon i holds the points points[2*poly_off[i] ..] as (x, y) int32 pairs up to poly_off[i+1] (at least one point);
 * boxes [n_polys][4] = {x, y, w, h} of its bounding box with w = max-min+1 (polygon.py:91); orient [n_polys][2] =
 * (cos, sin) of the calc_reg_line_stats angle, computed by the caller.  Every polygon is compared with the polygons of
 * its own page.  out_dist [n_polys] = the distance, max_d where it is not below max_d. */
int asep_textblock_interline_dists(asep_post* p, int n_pages, const int32_t* page_off, const int32_t* poly_off,
                                   const int32_t* points, const int32_t* boxes, const double* orient, double des_dist,
                                   double max_d, double* out_dist);
/* dbscan_baselines.py:253-307 region_query for every ordered pair of every page as a bit matrix: page k with
 * n = page_off[k+1]-page_off[k] polygons owns n rows of (n+31)/32 uint32 words, the pages one after the other; bit j
 * of row i is set when polygon j is a neighbour of polygon i.  boxes as above, dists [n_polys] the interline
 * distances, avg [n_pages] the page's average interline distance, fac the rectangle_interline_factor.
 * asep_textblock_neighbour_words gives the words the matrix needs; capacity_words is the size of out_bits. */
long long asep_textblock_neighbour_words(int n_pages, const int32_t* page_off);
int asep_textblock_neighbours(asep_post* p, int n_pages, const int32_t* page_off, const int32_t* boxes,
                              const double* dists, const double* avg, double fac, uint32_t* out_bits,
                              long long capacity_words);
/* Device time in microseconds of the kernel of the calling thread's last asep_textblock_interline_dists (which = 0)
 * or asep_textblock_neighbours (which = 1) call; -1 for another `which`. */
double asep_textblock_last_kernel_us(int which);

/* ---- text regions (python_util/geometry/util.py:568-697 alpha_shape behind the Delaunay triangulation) -----------------
 * One call for all articles of a group of pages on the asep_post handle; host pointers in and out, the call returns after
 * its results have arrived.  Page k holds the articles art_off[k] .. art_off[k+1]-1, article a the points
 * pt_off[a] .. pt_off[a+1]-1 of `points` ((x, y) int32 pairs) and the triangles tri_off[a] .. tri_off[a+1]-1 of
 * `simplices` and `neighbors` ([.][3] int32, scipy.spatial.Delaunay's tables of the article's points: indices local to
 * the article, neighbors[t][j] = the triangle opposite corner j or -1).  alpha0 [n_articles] is the first alpha of each
 * article; a refused alpha becomes alpha + alpha * 0.2, at most max_retries (>= 1) times.
 *
 * Out, per article a: out_ring[pt_off[a] ..] the point indices of the boundary in the reference's order (without the
 * repeated first point), out_len[a] their number, out_retries[a] the increases of alpha taken, out_failed[a] = 1 when
 * max_retries increases gave no single boundary (out_len[a] = 0 then).  Optional (NULL to skip), for tests:
 * out_circum_r [sum T] the circumradii as the reference computes them, bit for bit; out_edge_mask [sum T] bit k set when
 * the edge k = (corner k, corner (k+1) % 3) of the triangle is on the boundary in the article's last round.
 * The offset tables and every corner / neighbour index are checked before anything is allocated or launched;
 * ASEP_ERR_ARG names the page, the article and the reason.  A ring does not depend on what else shares the call. */
int asep_alpha_shapes(asep_post* p, int n_pages, const int32_t* art_off, const int32_t* pt_off, const int32_t* tri_off,
                      const int32_t* points, const int32_t* simplices, const int32_t* neighbors, const double* alpha0,
                      int max_retries, int32_t* out_ring, int32_t* out_len, int32_t* out_retries, int32_t* out_failed,
                      double* out_circum_r, uint8_t* out_edge_mask);
/* Device time in microseconds of the circumradius (which = 0) or boundary (which = 1) kernel of the calling thread's last
 * asep_alpha_shapes call; -1 for another `which`. */
double asep_alpha_shapes_last_kernel_us(int which);
/* The largest article (in points) whose vertex tables the boundary kernel keeps in LDS; larger ones use global scratch. */
int asep_alpha_shapes_lds_points(void);

/* The triangulation itself on the device: one workgroup per article builds the Delaunay triangulation of the article's
 * points (incremental Bowyer-Watson in (x, y) order, exact integer predicates) in scipy's two tables: out_simplices[t] the
 * corners, counter-clockwise, out_neighbors[t][j] the triangle opposite corner j or -1, indices local to the article.
 * Article a holds the points pt_off[a] .. pt_off[a+1]-1 and owns the triangles tri_off_cap[a] .. tri_off_cap[a+1]-1 of the
 * two output tables, which must have room for 2n - 5 triangles of its n >= 3 points; out_ntri[a] of them are filled, the rest
 * are zeros.  Exact duplicates of a point are in no triangle (the first of them is); cocircular points get one of their valid
 * triangulations, which depends on the article's points alone; collinear points of the hull are corners of proper triangles.
 * out_status[a]: 0 triangulated; 1 fewer than 3 distinct points; 2 all points on one line; 3 the bounding box is wider or
 * taller than asep_delaunay_max_extent() (the predicates are exact in int64 up to there); 4 / 5 an inconsistent table / no room
 * (neither is reachable through this interface).  A status other than 0 leaves out_ntri[a] = 0: the caller triangulates such an
 * article itself.  Offsets and room are checked before anything is allocated or launched; ASEP_ERR_ARG names the article and the
 * reason.  A result does not depend on what else shares the call. */
int asep_delaunay(asep_post* p, int n_articles, const int32_t* pt_off, const int32_t* points, const int32_t* tri_off_cap,
                  int32_t* out_simplices, int32_t* out_neighbors, int32_t* out_ntri, int32_t* out_status);
/* asep_alpha_shapes without tri_off / simplices / neighbors: the articles are triangulated on the device as by asep_delaunay
 * and the circumradius and boundary kernels read those tables where they are.  Same outputs (the ring starts at the first
 * boundary edge of the DEVICE's triangle order, so it is the reference's cycle, not its start or direction), plus
 * out_status[a] as above.  An article with a status other than 0 has no triangles: the boundary kernel, which this call leaves
 * as it is, finds no edge in any of its max_retries rounds, so it comes back with out_failed[a] = 1, out_len[a] = 0 and
 * out_retries[a] = max_retries, after max_retries short rounds of device time (they run beside the other articles' workgroups).
 * The call's triangle count never comes to the host: the stream is synchronised once, at the end. */
int asep_alpha_shapes_points(asep_post* p, int n_pages, const int32_t* art_off, const int32_t* pt_off, const int32_t* points,
                             const double* alpha0, int max_retries, int32_t* out_ring, int32_t* out_len, int32_t* out_retries,
                             int32_t* out_failed, int32_t* out_status);
/* Device time in microseconds of the triangulation kernel of the calling thread's last asep_delaunay or
 * asep_alpha_shapes_points call (the latter also sets asep_alpha_shapes_last_kernel_us). */
double asep_delaunay_last_kernel_us(void);
/* The largest article (in points) whose working tables the triangulation keeps in LDS; larger ones use global scratch. */
int asep_delaunay_lds_points(void);
/* The largest bounding-box extent (max - min, per axis) of an article the device triangulates. */
int asep_delaunay_max_extent(void);

/* ---- article separation measure (eval_measure.py count_rel_hits / count_rel_hits_list, Python path) -------------------
 * Batched over file pairs on the asep_post handle.  Truth and reco (hypothesis) polygons are NORMED baselines in the
 * layout of asep_textblock_interline_dists (points as (x, y) int32 pairs, poly_off, boxes {x, y, w, h}); file k holds
 * the truth polygons t_file_off[k] .. t_file_off[k+1]-1, the reco polygons r_file_off[k] .. and the reco articles
 * art_file_off[k] ..  The reco polygons of a file are grouped by article: article a holds the reco polygons
 * art_off[a] .. art_off[a+1]-1 (art_off [n_arts + 1], tiling each file); art_has_id[a] = 0 marks the group of lines
 * without an article id.  tols [n_truth][n_tols]: the tolerances of each truth polygon (ticks, or one value per truth
 * subset it is scored in); a value <= 0 yields 0.  dmax = floor(3 * largest tolerance), at most 4094; a truth polygon
 * holds at most 4096 points.
 *
 * A (reco i, truth j) pair, or a (truth j, article a) record, is a candidate when the bounding boxes are at most dmax
 * apart in x and in y; everything else has no distance <= dmax and contributes nothing.  Memory and output are bounded
 * by the candidates.  Per candidate pair: count_rel_hits(reco i, truth j, tols[j]) -- sum_p h(d_p) / n_points over the
 * points p of i with d_p the minimum L1 distance to the points of j.  Per record: count_rel_hits_list(truth j, polygons
 * of article a, tols[j]).  Per truth polygon: the same against all reco polygons of the file (slot 0) and against those
 * of the articles with an id (slot 1).  Every value is evaluated from the histogram of the integer distances over
 * ascending distance, so it depends on the multiset of distances, the point count and the tolerance only.
 *
 * asep_measure_run computes everything and returns the number of candidate pairs (out_counts = {pairs, records});
 * asep_measure_fetch, called next on the same thread and handle, copies the results to host arrays sized from those
 * counts (any pointer may be null): pair_ij [pairs][2] = (i, j) ordered by i then j, pair_hits [pairs][n_tols],
 * rec_ja [records][2] = (j, article index within the file) ordered by j then a, rec_hits [records][n_tols],
 * truth_hits [n_truth][2][n_tols]; with want_hist the distance histograms behind them ([..][dmax + 2] uint32, last
 * bin = distances above dmax).  Host pointers in and out; each call returns after its results have arrived. */
long long asep_measure_run(asep_post* p, int n_files, const int32_t* t_file_off, const int32_t* r_file_off,
                           const int32_t* t_poly_off, const int32_t* t_points, const int32_t* t_boxes,
                           const int32_t* r_poly_off, const int32_t* r_points, const int32_t* r_boxes,
                           const int32_t* art_file_off, const int32_t* art_off, const int32_t* art_has_id, int n_tols,
                           const double* tols, int dmax, int want_hist, long long* out_counts);
int asep_measure_fetch(asep_post* p, int32_t* pair_ij, double* pair_hits, int32_t* rec_ja, double* rec_hits,
                       double* truth_hits, uint32_t* pair_hist, uint32_t* rec_hist, uint32_t* truth_hist);
/* Device time in microseconds of the kernels of the calling thread's last asep_measure_run: which = 0 candidate count,
 * 1 pair (precision) kernel, 2 recall kernel; -1 for another `which`. */
double asep_measure_last_kernel_us(int which);

/* ---- heading detection evaluation (heading_evaluation.py / heading_evaluation_grid_search.py) --------------------------
 * Scores many settings of the heading fusion rule (heading_net_post_processor.py:110-195) at once on the asep_post
 * handle.  Page k holds the lines line_off[k] .. line_off[k+1]-1 and the text regions reg_off[k] .. reg_off[k+1]-1;
 * region r lists the lines reg_lines[reg_line_off[r] .. reg_line_off[r+1]-1] as indices within its page.  Per line the
 * normalised confidences sw_conf, th_conf, net_conf (doubles) and line_tagged (may be null: a line that already carries
 * the heading tag counts as a heading line under every setting); per page use_swt (0: the confidence is net_conf); per
 * region gt_heading (the ground truth label).  settings [n_settings][9] are numbers of tenths in 0..10: threshold,
 * net_w, sw_w, th_w, net_thresh, sw_thresh, th_thresh, sw_th_thresh, text_line_percentage, each turned into k / 10.0.
 * A line is a heading when (conf > threshold), conf = 1.0 if sw >= sw_thresh, th >= th_thresh, (sw + th) / 2 >=
 * sw_th_thresh or net >= net_thresh, else net_w * net + sw_w * sw + th_w * th; with net_w = 0 every net confidence is 0.
 * A region is a heading when it has lines and (double)headings / lines >= text_line_percentage.
 * out_counts [n_settings][n_pages][4] = TP, FP, FN, TN of the region labels.  Bad offsets, indices or settings return a
 * negative code (asep_last_error) and launch nothing.  Host pointers in and out; returns after the counts have arrived. */
int asep_heading_grid_eval(asep_post* p, int n_pages, const int32_t* line_off, const double* sw_conf, const double* th_conf,
                           const double* net_conf, const uint8_t* line_tagged, const uint8_t* use_swt, const int32_t* reg_off,
                           const int32_t* reg_line_off, const int32_t* reg_lines, const uint8_t* gt_heading, int n_settings,
                           const int32_t* settings, int32_t* out_counts);
/* Device time in microseconds of the kernel of the calling thread's last asep_heading_grid_eval (0 if nothing ran). */
double asep_heading_grid_last_kernel_us(void);

/* ---- clustering grid (clustering/dbscan.py for many pages and settings; the counts of as_eval.py) ---------------------------
 * Runs DBScanRelation.cluster_relations for every (page, setting) pair in one launch on the asep_post handle, one wavefront per
 * pair; the labels equal the host class's, integer for integer.  Page k has the nodes node_off[k] .. node_off[k+1]-1 (N_k of
 * them, at most asep_cluster_grid_max_nodes()); `conf` holds the pages' N_k x N_k matrices, row-major, one after the other, as
 * float (conf_is_f64 0) or double (1), prepared as DBScanRelation.confidences holds them (clamped, symmetric).  The thresholds
 * are compared in the matrix dtype: conf > (T)conf_thr for a neighbour, np.mean(conf[cand, members]) > (T)agree_thr to join.
 * A page of two nodes follows TextblockClustering.calc instead: labels 1, 1 when conf[0][1] >= (T)conf_thr, else 1, 2; only that
 * entry is read, so the caller passes the matrix calc tests (TextblockClustering._conf_mat, which need not be symmetric).
 * out_labels [n_settings][node_off[n_pages]]: labels from 1, -1 for noise nodes when assign_noise is 0.
 * The comparison tables are optional (all NULL: labels only).  Page k has the hypothesis lines line_off[k] .. line_off[k+1]-1:
 * line_node = the node of the page the line hangs in, line_gt = the line's dense ground truth article index (below the page's
 * number of lines) or -1 when the ground truth lacks the line; and the ground truth blocks gtblk_off[k] .. gtblk_off[k+1]-1,
 * block b listing the lines gtblk_lines[gtblk_line_off[b] .. gtblk_line_off[b+1]-1] as indices within the page.
 * out_counts [n_settings][n_pages][4] = hypNIs (distinct labels over the lines), n_inf (distinct (ground truth article, label)
 * pairs over the lines with line_gt >= 0), corrects (listed blocks whose lines share one label that no other line carries), 0.
 * With the tables given out_labels may be NULL.  Bad offsets, indices or a page above the limit return ASEP_ERR_ARG
 * (asep_last_error) and launch nothing.  Host pointers in and out; returns after the results have arrived. */
typedef struct asep_cluster_setting {
    int32_t min_neighbors; /* min_neighbors_for_cluster */
    int32_t assign_noise;  /* assign_noise_clusters */
    double conf_thr;       /* confidence_threshold */
    double agree_thr;      /* cluster_agreement_threshold */
} asep_cluster_setting;
int asep_cluster_grid_run(asep_post* p, int n_pages, const int32_t* node_off, const void* conf, int conf_is_f64, int n_settings,
                          const asep_cluster_setting* settings, const int32_t* line_off, const int32_t* line_node,
                          const int32_t* line_gt, const int32_t* gtblk_off, const int32_t* gtblk_line_off,
                          const int32_t* gtblk_lines, int32_t* out_labels, int32_t* out_counts);
/* Device time in microseconds of the kernels of the calling thread's last asep_cluster_grid_run (0 if nothing ran). */
double asep_cluster_grid_last_kernel_us(void);
/* Largest N_k asep_cluster_grid_run and asep_cluster_grid_run_methods accept. */
int asep_cluster_grid_max_nodes(void);

/* The same call over settings of three clustering methods of TextblockClustering, mixed freely; row s of every output belongs to
 * settings[s].  The pages' matrices come in up to three sets of the layout of `conf` above, all float (mats_are_f64 0) or all
 * double (1), each as the host class holds it after set_confs:
 *   conf   DBScanRelation.confidences, and _conf_mat for a page of two nodes (as above): needed by a dbscan setting, and by any
 *          setting when a page has two nodes (calc's rule for two nodes does not depend on the method; it reads conf_thr)
 *   dist   _dist_mat (diagonal 0): needed by a dbscan_std setting
 *   delta  _delta_mat (diagonal -inf, every other entry finite): needed by a greedy setting and by out_llh
 * A set that is not needed may be NULL; a needed one that is NULL is ASEP_ERR_ARG.
 * ASEP_CLUSTER_DBSCAN: as asep_cluster_grid_run (count = min_neighbors_for_cluster, param = cluster_agreement_threshold).
 * ASEP_CLUSTER_DBSCAN_STD: sklearn.cluster.dbscan(dist, metric='precomputed', eps = param, min_samples = count): node i is a core
 *   point when row i holds at least `count` entries <= (T)eps (the diagonal counts); clusters are numbered from 0 by their seed,
 *   the lowest core point without a label, and hold whatever is reachable from it along row entries <= (T)eps out of core
 *   points; other nodes are -1.  Rows, not columns: the matrix may be asymmetric.  assign_noise is not read.
 * ASEP_CLUSTER_GREEDY: TextblockClustering._greedy with max_iteration = count: while the budget lasts, (i, j) = the first
 *   maximum of the working matrix in row-major order; stop unless it is > 0; class i absorbs class j, for every other idx
 *   m[idx][i] = m[idx][i] + m[idx][j] (one addition in T) and m[i][idx] = m[idx][i], row and column j leave.  Labels from 0: the
 *   rank of the node's class among the classes left.  The working matrices live in the handle's pool (N_k^2 values per greedy
 *   setting and page).  assign_noise and param are not read.
 * out_llh (optional) [n_settings][n_pages]: TextblockClustering.rel_LLH of the labels, the sum of (delta[i][k] + delta[k][i]) / 2
 * over the pairs k < i with equal labels >= 0; each term is formed in T, the sum is taken in double (the host adds in T, so the
 * two agree to rounding, not bit for bit).  out_labels may be NULL when out_counts or out_llh is asked for.
 * An unknown method, a missing set, bad tables, more (page, setting) pairs than one launch holds or a page above the limit
 * return ASEP_ERR_ARG and launch nothing.  asep_cluster_grid_last_kernel_us covers all kernels of this call as well. */
#define ASEP_CLUSTER_DBSCAN 0
#define ASEP_CLUSTER_DBSCAN_STD 1
#define ASEP_CLUSTER_GREEDY 2
typedef struct asep_cluster_method_setting {
    int32_t method;        /* ASEP_CLUSTER_* */
    int32_t count;         /* min_neighbors_for_cluster | min_samples | max_iteration */
    int32_t assign_noise;  /* assign_noise_clusters (dbscan) */
    int32_t reserved;      /* 0 */
    double conf_thr;       /* confidence_threshold: dbscan's neighbourhood, and the rule for a page of two nodes */
    double param;          /* cluster_agreement_threshold | epsilon */
} asep_cluster_method_setting;
int asep_cluster_grid_run_methods(asep_post* p, int n_pages, const int32_t* node_off, int mats_are_f64, const void* conf,
                                  const void* dist, const void* delta, int n_settings,
                                  const asep_cluster_method_setting* settings, const int32_t* line_off, const int32_t* line_node,
                                  const int32_t* line_gt, const int32_t* gtblk_off, const int32_t* gtblk_line_off,
                                  const int32_t* gtblk_lines, int32_t* out_labels, int32_t* out_counts, double* out_llh);

/* ---- edge features (article_separation/gnn/input/feature_generation.py, the per-edge and per-pair part) ------------------------
 * For all pages of a call at once, on the asep_post handle: the separator flags of every edge, the convex hull of every edge's two
 * regions, and the pair bits the confidence masking reads.  Everything is integer geometry, so the results equal the host
 * functions' bit for bit.  No floating point is used.
 * Tables (offsets over pages; every *_off starts at 0 and never decreases):
 *   page k has the text regions node_off[k] .. node_off[k+1]-1; region r has the points node_pts[node_pt_off[r] .. node_pt_off[r+1]-1]
 *   ([x, y] int32, as np.asarray(points, dtype=np.int32) gives them) and node_heading[r] = 1 for a heading, else 0;
 *   page k has the separator regions sep_off[k] .. sep_off[k+1]-1 with sep_pt_off / sep_pts in the same form and sep_orient[s] =
 *   SeparatorRegion.get_orientation(): ASEP_SEP_NONE (no tag), ASEP_SEP_HORIZONTAL, ASEP_SEP_VERTICAL, ASEP_SEP_OTHER (any other text);
 *   page k has the edges edge_off[k] .. edge_off[k+1]-1, edges[e] = {a, b} as region indices WITHIN the page.
 * Every coordinate lies in [-ASEP_EDGE_COORD_MAX, ASEP_EDGE_COORD_MAX] = [-2^20, 2^20]: the centre of a box is a half-integer, so the
 * kernels work in doubled coordinates, and with this bound every cross product fits an int64 (and is exact in the host's doubles,
 * which is why the two agree).  Every region and every separator has at least one point.
 * Outputs, each optional (NULL = not computed):
 *   out_flags [E][2] uint8 = (horizontally_separated, vertically_separated) of get_edge_separator_feature_bb (rule ASEP_EDGE_RULE_BB;
 *     a separator without tag is horizontal when height < 5 * width, both clamped to >= 1) or of get_edge_separator_feature_line
 *     (ASEP_EDGE_RULE_LINE: the segment between the two box centres against the separator's box corners in the order (min,min),
 *     (max,min), (min,max), (max,max), closed on the fly, or line_in_bounding_box; then against the separator's own polygon; a
 *     separator tagged horizontal, or one with height < 5 * width, sets the first flag, any other the second).
 *   out_hull [E][hull_cap][2] int32 and out_hull_n [E] (both or none): convex_hull(points of a + points of b) as the host returns it:
 *     lexicographically smallest point first, strict left turns, collinear points dropped; all points collinear give [first, last],
 *     all points equal give [p, p].  Entries behind out_hull_n[e] are 0.  hull_cap must hold the points of the two regions of every
 *     edge, and E * hull_cap * 8 bytes must not exceed hull_budget_bytes (> 0; the device holds twice that as scratch): the caller
 *     splits its edges over several calls.  An edge whose own row exceeds the budget cannot be computed and is refused as such.
 *   out_pairs: one N_k x N_k uint8 matrix per page, one after the other: bit 0 = is_aligned_heading_separated(i, j), bit 1 =
 *     is_aligned_horizontally_separated(i, j, separators) is true, computed for i < j and mirrored; the diagonal is 0.
 * Bad or decreasing offsets, an edge index outside its page, a region or separator without points, a coordinate outside the bound,
 * an unknown rule, a hull_cap or budget that does not fit: ASEP_ERR_ARG (asep_last_error), nothing is launched.  Zero pages, edges
 * or separators are valid.  Host pointers in and out; returns after the results have arrived. */
#define ASEP_EDGE_COORD_MAX (1 << 20)
#define ASEP_EDGE_RULE_BB 0
#define ASEP_EDGE_RULE_LINE 1
#define ASEP_SEP_NONE 0
#define ASEP_SEP_HORIZONTAL 1
#define ASEP_SEP_VERTICAL 2
#define ASEP_SEP_OTHER 3
int asep_edge_features_run(asep_post* p, int n_pages, const int32_t* node_off, const int32_t* node_pt_off, const int32_t* node_pts,
                           const uint8_t* node_heading, const int32_t* sep_off, const int32_t* sep_pt_off, const int32_t* sep_pts,
                           const uint8_t* sep_orient, const int32_t* edge_off, const int32_t* edges, int rule, uint8_t* out_flags,
                           int32_t* out_hull, int32_t* out_hull_n, int hull_cap, long long hull_budget_bytes, uint8_t* out_pairs);
/* Device time in microseconds of the kernels of the calling thread's last asep_edge_features_run (0 if nothing ran). */
double asep_edge_features_last_kernel_us(void);
/* The kernels the calling thread's last asep_edge_features_run launched, as JSON text [{"kernel": name, "blocks": grid size}, ...]
 * in launch order ("[]" if nothing ran).  Returns the text's length, or ASEP_ERR_ARG if buf is too small. */
long asep_edge_features_last_launches(char* buf, size_t buflen);

/* ---- relation net evaluation (article_separation/gnn/trainer/lav_rel.py) ----------------------------------------------
 * An accumulator of (score, label) pairs in HBM and sklearn's _binary_clf_curve over them: what precision_recall_curve,
 * roc_auc_score and accuracy_score of lav_rel.py:190-229 are computed from, without a probability leaving the device.
 * A pair is one 32-bit key (float_bits(p) << 1) | label; asep_releval_finish sorts the keys (radix sort, 8 bits x 4 stable
 * passes of three launches each: digit histograms per tile, a scan of the digit x tile table, the scatter) and writes, per
 * distinct score in DESCENDING order, the score (thresholds), tps and fps = the number of pairs of label 1 / label 0 whose
 * score is >= it.  All of it is integer work: the results are exact and do not depend on the launch geometry.
 * One accumulator holds fewer than 2^31 pairs (every count is a 32-bit number on the device); more is refused with
 * ASEP_ERR_UNSUPPORTED.  The calls of one accumulator go to one stream, or the caller orders them. */
typedef struct asep_releval asep_releval;
asep_releval* asep_releval_create(void);
void asep_releval_free(asep_releval* h);
/* forget the pairs and the counters; buffers are kept */
int asep_releval_reset(asep_releval* h, void* stream);
/* room for total_pairs pairs.  Optional: the key buffer doubles when it is full (that synchronises `stream` once). */
int asep_releval_reserve(asep_releval* h, long long total_pairs, void* stream);
long long asep_releval_count(const asep_releval* h);
/* One page behind its forward, queued on `stream`, no host synchronisation (unless the buffer has to grow): d_probs
 * [R, num_classes] is the net's output, the LAST class column is the score (lav_rel.py:183); R must be N * N, pair (i, j) at
 * row i * N + j (input_dataset.py:444-457).  d_gt_relations [G, 3]: a row (., i, j) gives pair (i, j) label 1, duplicates are
 * harmless.  The call also counts what the host refuses at the end: scores that are NaN, negative or above 1, and rows of
 * d_gt_relations that name a node outside 0..N-1; and the positives and the pairs with (p > 0.5) == label. */
int asep_releval_append_dev(asep_releval* h, const float* d_probs, int num_classes, long long R, const int32_t* d_gt_relations,
                            int G, int N, void* stream);
/* The same from host arrays: probs [n] are the scores, labels [n] their labels (0 / non-zero).  Returns after the copy. */
int asep_releval_append_host(asep_releval* h, const float* probs, const uint8_t* labels, long long n, void* stream);
/* Sort and curve; *out_thresholds = T, the number of distinct scores (0 for an empty accumulator).  Synchronises `stream`. */
int asep_releval_finish(asep_releval* h, void* stream, long long* out_thresholds);
/* After finish: thresholds [T] float32, tps [T], fps [T] int64 (any may be null) and counters [8] = {pairs, refused scores,
 * positives counted by the appends, pairs with (p > 0.5) == label, refused ground truth rows,
 * A2 = sum_k (fps_k - fps_{k-1}) (tps_k + tps_{k-1}) with tps_{-1} = fps_{-1} = 0, T, positives counted in the sorted keys}.
 * AUC-ROC = A2 / (2 P (pairs - P)): one division of exact integers. */
int asep_releval_fetch(asep_releval* h, void* stream, float* thresholds, int64_t* tps, int64_t* fps, uint64_t* counters);
/* Device time in microseconds of stage `which` of the last finish: 3 * pass + {0 histogram, 1 scan, 2 scatter} for the
 * passes 0..3, 12 / 13 / 14 = curve count / scan / write, 15 = A2; -1 for another `which`. */
double asep_releval_stage_us(const asep_releval* h, int which);

/* ---- segmentation net evaluation (article_separation/plot_net_output.py) ---------------------------------------------
 * What plot_net_output computes from a pixel labeller's output, on the probabilities where asep_aru_forward_batch_dev2 left
 * them: the count of unsure values, the arg-max class counts, the per-class agreement with the ground truth channel images
 * and the per-class output masks.  Only integer counts leave the device; shares and accuracies are host divisions.
 * (The entry points of this block were added under ABI 12: the number is pinned by the suite and stays.) */
#define ASEP_SEG_EVAL_MAX_CLASSES 8
/* one page's counter block: ASEP_SEG_EVAL_SLOTS numbers; the per-class groups hold C entries each */
#define ASEP_SEG_EVAL_SLOTS 48
#define ASEP_SEG_EVAL_UNSURE 0   /* values with 0 < p < 1, before any threshold (:198-199) */
#define ASEP_SEG_EVAL_PIXELS 1   /* H * W */
#define ASEP_SEG_EVAL_HAS_GT 2   /* 1 if the page came with ground truth planes; the groups from EQUAL on are 0 without */
#define ASEP_SEG_EVAL_CLASS 8    /* [c] pixels whose arg max (first maximum) is c (:216-226) */
#define ASEP_SEG_EVAL_EQUAL 16   /* [c] pixels where the one-hot arg max equals gt_c / 255 (:109-117,241): (gt == 255 and arg max
                                    == c) or (gt == 0 and arg max != c); any other ground truth byte never matches */
#define ASEP_SEG_EVAL_TP 24      /* [c] arg max == c and gt_c == 255.  TP / FP / FN are an addition to the reference */
#define ASEP_SEG_EVAL_FP 32      /* [c] arg max == c and gt_c != 255 */
#define ASEP_SEG_EVAL_FN 40      /* [c] arg max != c and gt_c == 255 */
typedef struct asep_seg_eval asep_seg_eval;
asep_seg_eval* asep_seg_eval_create(void);
void asep_seg_eval_free(asep_seg_eval* h);
/* The pages of a call, of any sizes, in one launch per 12 pages.  Host arrays: d_probs[b] = page b's float32 [H[b], W[b], C];
 * d_gt (or NULL) [n_pages * C]: d_gt[b * C + c] = uint8 [H[b], W[b]] plane of class c, a page's C entries all set or all NULL;
 * d_masks (or NULL) [n_pages]: d_masks[b] (or NULL) receives the planar uint8 [C][H[b], W[b]] masks, uint8(p * 255) by
 * truncation.  mask_threshold != 0: the values become p > 0.6 before the arg max and the masks 0 / 255 -- 0.6 whatever the
 * flag's value, as :201-202 have it; the unsure count is taken first.  out_counters [n_pages * ASEP_SEG_EVAL_SLOTS] is host
 * memory.  The counters are zeroed by the call; the call synchronises `stream`.
 * Refused: C < 1 (ASEP_ERR_ARG), C > ASEP_SEG_EVAL_MAX_CLASSES or a page of H * W * C >= 2^40 values (ASEP_ERR_UNSUPPORTED), a
 * page without probabilities or with some but not all of its ground truth planes (ASEP_ERR_ARG). */
int asep_seg_eval_pages_dev(asep_seg_eval* h, int n_pages, const float* const* d_probs, const uint8_t* const* d_gt,
                            uint8_t* const* d_masks, const int32_t* H, const int32_t* W, int C, int mask_threshold,
                            unsigned long long* out_counters, void* stream);
/* apply_mask(image, mask, (r, g, b), alpha 0.5) of :57-93: d_out [H, W, 3] = where d_mask [H, W] is 255 the truncated mean of the
 * d_scan [H, W, 3] byte and the colour, else the scan's byte.  Queued on `stream`; d_out may be d_scan. */
int asep_seg_eval_blend_dev(asep_seg_eval* h, const uint8_t* d_scan, const uint8_t* d_mask, int H, int W, int r, int g, int b,
                            uint8_t* d_out, void* stream);
/* Device time in microseconds of the scoring launches of the last asep_seg_eval_pages_dev. */
double asep_seg_eval_last_kernel_us(const asep_seg_eval* h);
/* The kernels launched through the handle since the start of its last asep_seg_eval_pages_dev, one name per line
 * ("seg_eval_kernel<C,thr>", "seg_blend_kernel").  Copies at most max_bytes - 1 characters; returns the text's length. */
long asep_seg_eval_last_launches(const asep_seg_eval* h, char* buf, size_t max_bytes);

/* ---- JPEG pixels (added under ABI 12; csrc/jpeg_engine.hip, a code object of its own) ------------------------------------------
 * The parallel half of a JPEG decode: asep_jpeg_probe / asep_jpeg_entropy_decode of asep_host.h give the frame description, the quantised
 * coefficients (per component int16 [blocks_h][blocks_w][64], natural order) and the quantisation tables (uint16 [4][64], natural order,
 * HOST memory in both forms); here they become the bytes libjpeg-turbo's defaults produce: dequantisation and the accurate integer
 * inverse DCT, "fancy" chroma upsampling over the real downsampled size, YCbCr -> RGB in 16-bit fixed point, cropped to width x height.
 * A one-component page gives [H, W] whatever the order.  A three-component page gives [H, W, 3] B, G, R (what load_image_bgr returns),
 * [H, W, 3] R, G, B (the relation net's page_u8), or for ASEP_JPEG_ORDER_GRAY [H, W] with the BGR2GRAY weights of load_image_gray.
 * Refused with ASEP_ERR_ARG: a description whose block grid, sampling or coefficient size does not follow from its width and height.
 * asep_jpeg_pixels_dev queues on `stream` (scratch: p's arena, so one handle serves one stream); asep_jpeg_pixels uploads `coef`,
 * runs on p's stream, copies `out` back and synchronises. */
#define ASEP_JPEG_ORDER_GRAY 0
#define ASEP_JPEG_ORDER_BGR 1
#define ASEP_JPEG_ORDER_RGB 2
int asep_jpeg_pixels_dev(asep_post* p, const asep_jpeg_info* info, const int16_t* d_coef, const uint16_t* qt, int order, uint8_t* d_out,
                         void* stream);
int asep_jpeg_pixels(asep_post* p, const asep_jpeg_info* info, const int16_t* coef, const uint16_t* qt, int order, uint8_t* out);
/* The kernels the calling thread's last call of the two above launched, one name per line ("jpeg_idct_kernel", "jpeg_colour_kernel").
 * Copies at most max_bytes - 1 characters and returns the text's length. */
long asep_jpeg_last_launches(char* buf, size_t max_bytes);

/* ---- JPEG entropy decode (added under ABI 12 as well; csrc/jpeg_huffman_kernels.h, entry points in csrc/jpeg_engine.hip) ------------
 * The Huffman decode of a scan that asep_jpeg_scan_prepare (asep_host_jpeg.h) unstuffed, by self-synchronising subsequences: every
 * segment is cut into subsequences of subseq_bits bits (a multiple of 32, >= 64; 0 = ASEP_JPEG_SUBSEQ_BITS_DEFAULT), one thread each.
 *   speculate   decode from a guessed state (block 0 of the MCU, first AC position); an invalid code skips one bit, nothing is reported
 *   synchronise entry[s + 1] = exit[s], decode again where the entry changed, until a launch changes nothing.  A launch is
 *               ASEP_JPEG_SYNC_INNER rounds (doubled per launch up to _MAX) with workgroup barriers between them; no workgroup waits for another.  The host reads one
 *               "changed" word back after every launch (so this call blocks on `stream` once or a few times) and stops at the cap.
 *               The cap follows from the subsequences: a launch sees all that earlier launches stored, and inside a launch
 *               correctness moves one subsequence forward per round within a workgroup, so with n the subsequences of the longest
 *               segment n - 1 rounds suffice where one workgroup holds the scan, and otherwise ceil(n / _MAX) + 1 launches of _MAX
 *               rounds, one per workgroup the segment touches, behind the five shorter ones; one more launch of one round has to
 *               confirm.  Self-synchronisation ends the loop long before wherever blocks end in end-of-block codes.
 *               asep_jpeg_entropy_set_max_rounds (for tests) lowers the cap.
 *   place       exclusive sum of the completed blocks per segment -> every subsequence's first block
 *   write       d_coef zeroed, then decoded once more from the now correct entries: de-zigzagged, at the block's place in its
 *               component's plane, the DC as its difference; real errors go to the status
 *   DC, energy  inclusive sum of the DC differences per component and segment with the host's range rule, then the energy bound
 * d_coef (info->coef_bytes) gets exactly what asep_jpeg_entropy_decode writes; *d_status (device) is 0 then.  Otherwise it is an OR of
 * ASEP_JPEG_STATUS_*, and d_coef holds no promise except that nothing outside it was written.  d_scan: scan_bytes bytes in an allocation
 * of scan_bytes rounded up to 4; tables and segments are HOST memory and are copied before the call returns.  Scratch: p's arena.
 * asep_jpeg_entropy is the blocking form with host pointers throughout; *status is the host's copy. */
#define ASEP_JPEG_SUBSEQ_BITS_DEFAULT 128
#define ASEP_JPEG_SYNC_INNER 8
#define ASEP_JPEG_SYNC_INNER_MAX 256
#define ASEP_JPEG_STATUS_DAMAGED 1       /* invalid code, index past 63, refused category, segment length or block count off, DC out of range */
#define ASEP_JPEG_STATUS_REFUSED 2       /* a block above the energy bound (ASEP_JPEG_REFUSED on the host) */
#define ASEP_JPEG_STATUS_NOT_CONVERGED 4 /* the cap of rounds was reached */
int asep_jpeg_entropy_dev(asep_post* p, const asep_jpeg_info* info, const uint8_t* d_scan, size_t scan_bytes,
                          const asep_jpeg_scan_tables* tables, const asep_jpeg_segment* segments, int n_segments, int subseq_bits,
                          int16_t* d_coef, int32_t* d_status, void* stream);
int asep_jpeg_entropy(asep_post* p, const asep_jpeg_info* info, const uint8_t* scan, size_t scan_bytes,
                      const asep_jpeg_scan_tables* tables, const asep_jpeg_segment* segments, int n_segments, int subseq_bits,
                      int16_t* coef, int32_t* status);
/* Rounds of the calling thread's last entropy call until a launch changed nothing (a sum of whole launches), and its
 * subsequence count; for measurements. */
int asep_jpeg_entropy_last_rounds(int* n_subsequences);
/* For tests: the calling thread's later entropy calls stop after at most max_rounds rounds (status "not converged" where that is too
 * few); 0 = the cap above alone. */
void asep_jpeg_entropy_set_max_rounds(int max_rounds);

#ifdef __cplusplus
}
#endif
#endif /* ASEP_HIP_H */
