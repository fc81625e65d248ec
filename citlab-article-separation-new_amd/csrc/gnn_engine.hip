// GNN relation-predictor engine (host side).  Entry points: include/asep_hip.h.
// Schedule of one page (batch size 1, graph_gnn.py:46-167 + graph_relation.py:194-203):
//   [visual branch: backbone -> ROI max -> compression -> concat]
//   edge correction -> T x (message, LSTM update) -> per-node first classifier layer -> per-pair classifier.
// Three step kernels, chosen at load time:
//   STEP_SMALL  gnn_step_kernel      widths 32/32/32, U <= 8, Ed <= 4: W1 fragments in registers (the 7-feature nets)
//   STEP_BIG    gnn_step_big_kernel  widths 32/32/32, U <= 120, Ed <= 4: W1 fragments in LDS (visual nets, U = 55)
//   STEP_GENERIC  gnn_message_generic_kernel + gnn_lstm_generic_kernel: any widths (plain FMA loops)
// Round 6: for the widths of STEP_SMALL / STEP_BIG the default is the FACTORED step (gnn_fact_pre_kernel once per page +
// gnn_step_fact_kernel per step: per-node terms of the edge MLP's first layer per node, K = 32 per edge and step); ASEP_GNN_FACTOR=0
// keeps the unfactored kernels (the tests compare the two).
#include <algorithm>
#include <memory>

#include "asep_common.h"
#include "fmap_kernels.h"
#include "gnn_batch_kernels.h"
#include "gnn_kernels.h"

using namespace asep;

enum { STEP_GENERIC = 0, STEP_SMALL = 1, STEP_BIG = 2, STEP_FACT = 3 };

struct asep_gnn {
    asep_gnn_cfg cfg{};
    int U = 0, Ed = 0, H = 0, I = 0, Hm = 0;   // node / edge feature widths, hidden, interaction, MLP hidden
    int K = 0, V = 0;                 // message-MLP input width, LSTM input width
    float *b1 = nullptr, *b2 = nullptr;          // biases of the default one-hidden-layer edge MLP (fused step kernels)
    MlpW msg{};                       // the interaction MLP (no attention): [K] -> hidden ... -> [I]
    int msg_maxh = 0;                 // widest hidden layer of the interaction / attention MLPs
    float* Wg[4] = {nullptr, nullptr, nullptr, nullptr};
    float* bg[4] = {nullptr, nullptr, nullptr, nullptr};
    float *C1 = nullptr, *cb1 = nullptr, *C2 = nullptr, *cb2 = nullptr, *C3 = nullptr, *cb3 = nullptr;
    MlpW cls_rest{};                  // classifier layers behind the first hidden one: [cls_hidden1] -> ... -> [num_classes]
    int cls_maxw = 0;
    bool cls_fast = false;            // 64, 32 -> 2: gnn_pair_cls_kernel<64,32,2>
    int Iout = 0;                     // width of x (message_fn_chunk.py:229-241): heads * x_dim for 'concat', interaction_dim otherwise
    int Ed_fed = 0;                   // width of the edge features as FED (Ed minus the visual edge dims)
    // fused MFMA step kernels: permuted W1 / W2 fragments + quad descriptors
    float *A1 = nullptr, *A2 = nullptr;
    unsigned char* qdesc = nullptr;
    int nch = 0, Upad = 0;
    int mode = STEP_GENERIC;
    size_t big_lds = 0;
    bool use_step = true;             // ASEP_GNN_STEP=0 selects the separate (generic) message / LSTM kernels
    bool use_fact = true;             // ASEP_GNN_FACTOR=0: the unfactored fused step kernels (STEP_SMALL / STEP_BIG)
    float *Wuu = nullptr, *Wde = nullptr, *Whh = nullptr, *A1f = nullptr;   // factored first layer (gnn_kernels.h, "The FACTORED step")
    size_t fact_pre_lds = 0, fact_lds = 0;
    std::vector<void*> owned;
    BufferPool pool;                  // buffers of one forward (requested in a fixed order)
    BufferPool vis_pool;              // buffers of the visual stage in front of it
    BufferPool host_stage;            // device staging of the host-pointer entry points (grow-only)
    // state of the last forward
    int N = 0;
    float* d_h = nullptr;
    int* d_rowptr = nullptr;
    hipStream_t stream = nullptr;
    // visual branch (graph_relation.py:84-139): backbone + per-map compression layers
    // graph_gnn.py:102-109 compress_node_feature_dim: fed features [N, Uin] -> tanh(Wc x + bc) [N, U]; Uin == U when off
    int Uin = 0;
    float* Wc = nullptr;
    float* bc = nullptr;
    std::map<std::string, HostTensor> vis_blob;      // visual_node_feature_compression_fm_<i>/dense/{weights,bias}
    asep_aru* backbone = nullptr;                    // not owned
    std::vector<std::string> vis_names;
    std::vector<float*> vis_W, vis_b;                // owned through vis_owned
    std::vector<void*> vis_owned;
    std::vector<int> vis_C, vis_d;
    int vis_total = 0;
    // generated feature maps (feature_map_generators.py:72-197; fmap_kernels.h): per map its layer_depth (-1 = the end point itself) and,
    // for a generated one, the two convolutions.  All empty / -1 for the default layout: nothing below is then touched by a forward.
    struct FmapGen {
        int depth = -1;                              // layer_depth d: 1x1 to d / 2 channels, 3x3 to d
        int Cin = 0, stride = 1;                     // channels of the map it reads; 2 = from_layer '' (reads map i - 1)
        float *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr;   // owned through vis_owned
    };
    struct FmapRef { const float* p = nullptr; int fh = 0, fw = 0, C = 0, bf = 0; };
    std::vector<FmapGen> vis_gen;
    int n_generated = 0;
    BufferPool fmap_pool;                            // intermediates and generated maps of the last page (sized at its first forward)
    std::vector<FmapRef> fmap_last;                  // every map of the last page, generated or not (asep_gnn_get_feature_map)
    std::string fmap_last_prefix;
    // asep_gnn_forward_visual_batch_dev2: the page tables of a call in device memory.  A ring of page-locked host buffers with their device
    // copies: a call fills the next two slots (the tables in front of the backbone, the tables behind it), copies them on the call's stream
    // (asynchronous, no host wait) and records the slot's event behind the last kernel that reads the table; a slot is refilled only once that
    // event -- four calls back -- has passed.  Buffers grow and are kept.  Like the handle's arenas the ring assumes that the calls of a handle
    // go to one stream, or that the caller orders them.
    struct TableSlot { char* h = nullptr; char* d = nullptr; size_t cap = 0; hipEvent_t done = nullptr; };
    TableSlot tab_ring[8];
    unsigned tab_next = 0;
    // what the asep_gnn_get_page_* functions read: per page of the last dev2 call its node count, its rows of d_u_cat and its maps
    struct PageRec { int N = 0; size_t u_off = 0; std::vector<FmapRef> maps; };
    std::vector<PageRec> batch_pages;
    unsigned long long fwd_serial = 0, batch_serial = ~0ull;   // forwards queued so far / the count right after the last dev2 call
    std::vector<FmapRef> batch_images;               // the resized images of the last u8 call ([h, w, C] fp32)
    float* Wout = nullptr;                           // output_type 1: GraphLSTM1/dense/weights [Uin, H]
    AttHeadW att_w[GNN_MAX_HEADS] = {};              // attention_heads > 0: per-head interaction + attention MLPs
    AttHeadW* d_att_w = nullptr;                     // the same in device memory (kernel argument of gnn_msg_att_kernel)
    int att_xd = 0;                                  // interaction width per head
    // visual EDGE features (graph_relation.py:141-172): compression layers per feature map, concatenated behind the fed edge features
    std::vector<float*> vise_W, vise_b;
    std::vector<int> vise_d;
    int vise_total = 0;
    float* d_ef_cat = nullptr;                       // [E, Ed] per page of the last visual forward (own buffer)
    size_t ef_cat_cap = 0;
    float* d_u_cat = nullptr;                        // concatenated node features of the last visual forward (own buffer)
    size_t u_cat_cap = 0;
    // asep_gnn_forward_batch[_dev] (the graph part of the pages of one call; the section at the end of this file): its own buffers, so that
    // the single-page forwards keep theirs; the page rows and the corrected lists of the last call for asep_gnn_get_page_hidden / _edges
    BufferPool batch_pool;
    std::vector<GnnPageRow> graph_pages;
    unsigned long long graph_serial = ~0ull;         // fwd_serial right after the last batched graph call
    const int32_t* gb_sorted = nullptr;
    const int* gb_sfirst = nullptr;
    const int* gb_rowptr = nullptr;
    long batch_launches = 0;                         // kernels the last asep_gnn_forward_batch[_dev] launched (0: it was refused)
    void free_visual() {
        for (void* p : vis_owned)
            if (p) (void)hipFree(p);
        vis_owned.clear(); vis_W.clear(); vis_b.clear(); vis_names.clear(); vis_C.clear(); vis_d.clear();
        vise_W.clear(); vise_b.clear(); vise_d.clear();
        vis_total = 0; vise_total = 0;
        vis_gen.clear(); fmap_last.clear(); n_generated = 0;
        fmap_pool.release();                         // (hipFree waits for the device: no forward still reads the maps)
        backbone = nullptr;
    }
    ~asep_gnn() {
        free_visual();
        for (TableSlot& t : tab_ring) {
            if (t.done) (void)hipEventDestroy(t.done);
            if (t.h) (void)hipHostFree(t.h);
            if (t.d) (void)hipFree(t.d);
        }
        if (d_u_cat) (void)hipFree(d_u_cat);
        if (d_ef_cat) (void)hipFree(d_ef_cat);
        for (void* p : owned)
            if (p) (void)hipFree(p);
    }
};

namespace {

const char* MSG = "GraphLSTM1/message_fn_default/head_0/calculation_interaction_features/concat_u_and_h/interaction_features";
const char* UPD = "GraphLSTM1/update_function_LSTM";
const char* CLS = "Classification/logits";

int upload_named(std::vector<void*>& owner, const std::map<std::string, HostTensor>& blob, const std::string& name,
                 std::vector<int> dims, float** d) {
    auto it = blob.find(name);
    if (it == blob.end()) { set_error("weights: missing tensor %s", name.c_str()); return ASEP_ERR_WEIGHTS; }
    if (it->second.dims != dims) {
        std::string want, got;
        for (int v : dims) want += std::to_string(v) + ",";
        for (int v : it->second.dims) got += std::to_string(v) + ",";
        set_error("weights: %s has shape [%s] expected [%s]", name.c_str(), got.c_str(), want.c_str());
        return ASEP_ERR_WEIGHTS;
    }
    const auto& h = it->second.data;
    ASEP_HIP_CHECK(hipMalloc((void**)d, std::max<size_t>(h.size(), 4) * sizeof(float)));
    owner.push_back(*d);
    ASEP_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return ASEP_OK;
}

template <typename T>
int upload_vec(asep_gnn* g, const std::vector<T>& v, T** d) {
    ASEP_HIP_CHECK(hipMalloc((void**)d, std::max<size_t>(v.size(), 4) * sizeof(T)));
    g->owned.push_back(*d);
    ASEP_HIP_CHECK(hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return ASEP_OK;
}

// An MLP of layers.py:468-490 under `scope`: fully_connected_layer_h<i> for the hidden widths, fully_connected_logit_layer_out
int upload_mlp(asep_gnn* g, const std::map<std::string, HostTensor>& blob, const std::string& scope, int d_in,
               const std::vector<int>& hidden, int d_out, MlpW* m, int first_layer = 0) {
    // first_layer = 1: the first hidden layer is held elsewhere (classifier: evaluated per node); dims[0] = its width
    if ((int)hidden.size() > GNN_MLP_MAX) { set_error("%s: %zu hidden layers, at most %d are served", scope.c_str(), hidden.size(), GNN_MLP_MAX); return ASEP_ERR_UNSUPPORTED; }
    *m = MlpW{};
    int cur = d_in, l = 0;
    for (size_t i = 0; i < hidden.size(); ++i) {
        if ((int)i >= first_layer) {
            const std::string ly = scope + "/fully_connected_layer_h" + std::to_string(i + 1);
            float *W = nullptr, *b = nullptr;
            int rc = upload_named(g->owned, blob, ly + "/weights", {cur, hidden[i]}, &W);
            if (!rc) rc = upload_named(g->owned, blob, ly + "/bias", {hidden[i]}, &b);
            if (rc) return rc;
            m->W[l] = W; m->b[l] = b; m->dims[l] = cur; ++l;
        }
        cur = hidden[i];
    }
    float *W = nullptr, *b = nullptr;
    int rc = upload_named(g->owned, blob, scope + "/fully_connected_logit_layer_out/weights", {cur, d_out}, &W);
    if (!rc) rc = upload_named(g->owned, blob, scope + "/fully_connected_logit_layer_out/bias", {d_out}, &b);
    if (rc) return rc;
    m->W[l] = W; m->b[l] = b; m->dims[l] = cur; ++l;
    m->dims[l] = d_out;
    m->nl = l;
    return ASEP_OK;
}

std::vector<int> hidden_list(std::initializer_list<int> v) {      // the non-zero prefix of a cfg's hidden-width fields
    std::vector<int> out;
    for (int x : v) {
        if (x <= 0) break;
        out.push_back(x);
    }
    return out;
}

// K axis of the edge MLP permuted into quads of four consecutive features (gnn_kernels.h): fragments + descriptors
struct Quad { int type, off; };

int pack_step_fragments(asep_gnn* g, const std::map<std::string, HostTensor>& blob, bool big) {
    const int U = g->U, Ed = g->Ed;
    const std::string m = MSG;
    std::vector<Quad> quads;
    const int uq = (U + 3) / 4;
    for (int t : {GQ_UI, GQ_UJ, GQ_DU, GQ_DU2})
        for (int q = 0; q < uq; ++q) quads.push_back({t, 4 * q});
    if (Ed > 0) quads.push_back({GQ_EF, 0});
    while (quads.size() % 4) quads.push_back({GQ_ZERO, 0});
    // H-type quads come as whole chunks: lane group k4 owns h[16c' + 4 k4 ..]
    for (int t : {GQ_HI, GQ_HJ, GQ_DH, GQ_DH2})
        for (int c = 0; c < 2; ++c)
            for (int k4 = 0; k4 < 4; ++k4) quads.push_back({t, big ? 16 * c + 4 * k4 : 16 * c});
    g->nch = (int)quads.size() / 4;
    const HostTensor& W1h = blob.find(m + "/fully_connected_layer_h1/weights")->second;            // [K,32]
    const HostTensor& W2h = blob.find(m + "/fully_connected_logit_layer_out/weights")->second;     // [32,32]
    auto w1row = [&](const Quad& q, int k4, int r) -> int {              // original row of W1 or -1 (zero)
        const int hoff = big ? q.off + r : q.off + 4 * k4 + r;
        switch (q.type) {
            case GQ_UI: return q.off + r < U ? 0 * U + q.off + r : -1;
            case GQ_UJ: return q.off + r < U ? 1 * U + q.off + r : -1;
            case GQ_DU: return q.off + r < U ? 2 * U + q.off + r : -1;
            case GQ_DU2: return q.off + r < U ? 3 * U + q.off + r : -1;
            case GQ_EF: return r < Ed ? 4 * U + r : -1;
            case GQ_HI: return 4 * U + Ed + 0 * 32 + hoff;
            case GQ_HJ: return 4 * U + Ed + 1 * 32 + hoff;
            case GQ_DH: return 4 * U + Ed + 2 * 32 + hoff;
            case GQ_DH2: return 4 * U + Ed + 3 * 32 + hoff;
            default: return -1;
        }
    };
    std::vector<float> a1((size_t)g->nch * 2 * 64 * 4), a2((size_t)2 * 2 * 64 * 4);
    const int dstride = big ? 4 : 2;
    std::vector<unsigned char> qd((size_t)g->nch * 4 * dstride, 0);
    for (int c = 0; c < g->nch; ++c)
        for (int k4 = 0; k4 < 4; ++k4) {
            const Quad& q = quads[c * 4 + k4];
            qd[(c * 4 + k4) * dstride] = (unsigned char)q.type;
            qd[(c * 4 + k4) * dstride + 1] = (unsigned char)(big ? q.off / 4 : q.off);
            for (int mt = 0; mt < 2; ++mt)
                for (int i = 0; i < 16; ++i)
                    for (int r = 0; r < 4; ++r) {
                        const int row = w1row(q, k4, r), lane = k4 * 16 + i;
                        a1[(((size_t)c * 2 + mt) * 64 + lane) * 4 + r] = row < 0 ? 0.f : W1h.data[(size_t)row * GNN_H + 16 * mt + i];
                    }
        }
    for (int c = 0; c < 2; ++c)
        for (int mt = 0; mt < 2; ++mt)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    a2[(((size_t)c * 2 + mt) * 64 + lane) * 4 + r] = W2h.data[(size_t)(16 * c + 4 * (lane >> 4) + r) * GNN_H + 16 * mt + (lane & 15)];
    int rc = upload_vec(g, a1, &g->A1);
    if (!rc) rc = upload_vec(g, a2, &g->A2);
    if (!rc) rc = upload_vec(g, qd, &g->qdesc);
    return rc;
}

// The factored first layer of the edge MLP (gnn_kernels.h): W1's row blocks [Wa Wb Wc Wd | We | Wf Wg Wh Wi] combined in double
int pack_fact(asep_gnn* g, const std::map<std::string, HostTensor>& blob) {
    const int U = g->U, Ed = g->Ed;
    const std::string m = MSG;
    const HostTensor& W1 = blob.find(m + "/fully_connected_layer_h1/weights")->second;            // [K,32]
    auto w = [&](int row, int o) -> double { return (double)W1.data[(size_t)row * GNN_H + o]; };
    const int ha = 4 * U + Ed;                                   // first row of Wf
    std::vector<float> wuu((size_t)std::max(U, 1) * 64), wde((size_t)std::max(U + Ed, 1) * 32), whh((size_t)32 * 64), a1((size_t)2 * 2 * 64 * 4);
    for (int k = 0; k < U; ++k)
        for (int o = 0; o < 32; ++o) {
            wuu[(size_t)k * 64 + o] = (float)(w(k, o) - w(2 * U + k, o));                  // Wa - Wc
            wuu[(size_t)k * 64 + 32 + o] = (float)(w(U + k, o) + w(2 * U + k, o));         // Wb + Wc
            wde[(size_t)k * 32 + o] = (float)w(3 * U + k, o);                              // Wd
        }
    for (int k = 0; k < Ed; ++k)
        for (int o = 0; o < 32; ++o) wde[(size_t)(U + k) * 32 + o] = (float)w(4 * U + k, o);   // We
    for (int k = 0; k < 32; ++k)
        for (int o = 0; o < 32; ++o) {
            whh[(size_t)k * 64 + o] = (float)(w(ha + k, o) - w(ha + 64 + k, o));           // Wf - Wh
            whh[(size_t)k * 64 + 32 + o] = (float)(w(ha + 32 + k, o) + w(ha + 64 + k, o)); // Wg + Wh
        }
    for (int c = 0; c < 2; ++c)                                   // Wi as A fragments: slot 16 c + 4 kk + r, unit 16 mt + i
        for (int mt = 0; mt < 2; ++mt)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r)
                    a1[(((size_t)c * 2 + mt) * 64 + lane) * 4 + r] = (float)w(ha + 96 + 16 * c + 4 * (lane >> 4) + r, 16 * mt + (lane & 15));
    int rc = upload_vec(g, wuu, &g->Wuu);
    if (!rc) rc = upload_vec(g, wde, &g->Wde);
    if (!rc) rc = upload_vec(g, whh, &g->Whh);
    if (!rc) rc = upload_vec(g, a1, &g->A1f);
    return rc;
}

struct EdgeBufs {
    int* table; int* rowcnt; int* colcnt; int* rowptr; int* colptr;
    int32_t* sorted; int* sfirst; int* tsrc; int* tfirst;
};

// the buffers of an edge correction over `nodes` nodes: dense tables of `cells` cells in all (queued here: every cell "no edge"), lists of maxE
int edge_bufs(BufferPool& pool, size_t cells, size_t nodes, size_t maxE, EdgeBufs& eb, hipStream_t s) {
    eb.table = (int*)pool.get(cells * sizeof(int));
    eb.rowcnt = (int*)pool.get(nodes * sizeof(int));
    eb.colcnt = (int*)pool.get(nodes * sizeof(int));
    eb.rowptr = (int*)pool.get((nodes + 1) * sizeof(int));
    eb.colptr = (int*)pool.get((nodes + 1) * sizeof(int));
    eb.sorted = (int32_t*)pool.get(maxE * 2 * sizeof(int32_t));
    eb.sfirst = (int*)pool.get(maxE * sizeof(int));
    eb.tsrc = (int*)pool.get(maxE * sizeof(int));
    eb.tfirst = (int*)pool.get(maxE * sizeof(int));
    ASEP_HIP_CHECK(hipMemsetAsync(eb.table, 0x7f, cells * sizeof(int), s));
    return ASEP_OK;
}

// misc.py:7-151 on the device; fills the CSR-by-target used by the message kernel
int correct_edges_dev(asep_gnn* g, BufferPool& pool, int N, int E, const int32_t* d_edges, EdgeBufs& eb, hipStream_t s) {
    const int und = g->cfg.undirected_graph ? 1 : 0;
    if (int rc = edge_bufs(pool, (size_t)N * N, (size_t)N, (size_t)(und ? 2 : 1) * std::max(E, 1), eb, s)) return rc;
    if (E > 0) {
        const int total = und ? 2 * E : E;
        hipLaunchKernelGGL(edge_table_kernel, dim3(std::min(cdiv(total, 256), 2048)), dim3(256), 0, s, d_edges, E, N, und,
                           eb.table);
    }
    hipLaunchKernelGGL(edge_count_kernel, dim3(N), dim3(64), 0, s, eb.table, N, eb.rowcnt, eb.colcnt);
    hipLaunchKernelGGL(edge_scan_kernel, dim3(1), dim3(1024), 0, s, eb.rowcnt, eb.colcnt, N, eb.rowptr, eb.colptr);
    hipLaunchKernelGGL(edge_emit_kernel, dim3(N), dim3(64), 0, s, eb.table, N, eb.rowptr, eb.colptr, eb.sorted,
                       eb.sfirst, eb.tsrc, eb.tfirst);
    ASEP_HIP_CHECK(hipGetLastError());
    g->d_rowptr = eb.rowptr;
    return ASEP_OK;
}

// the step kernel of this model under the switches: the factored form wherever a fused step kernel serves the widths
inline int step_mode_of(const asep_gnn* g) {
    if (!g->use_step || g->mode == STEP_GENERIC) return STEP_GENERIC;
    return g->use_fact && g->A1f ? STEP_FACT : g->mode;
}

// a launch that its caller counts (asep_gnn_batch_launches)
#define COUNTED_LAUNCH(count, ...) do { hipLaunchKernelGGL(__VA_ARGS__); ++(count); } while (0)

struct GraphOut { const float* hcls = nullptr; int Hc = 0; long launches = 0; };   // what the pair classifier reads, its width; kernels launched

// The ONE step schedule of the relation net, from the compress_node_feature_dim layer to the output_type layer: T x (message, aggregation /
// attention soft-max, LSTM update) over the N nodes of a launch -- a page (forward_impl) or all pages of a call (forward_batch_impl; one
// CSR-by-target over them: no kernel in here knows of pages).  Erows = rows of the fed edge features (`tfirst % Erows` is the row), maxE = the
// capacity of the corrected lists.  The one page-dependent launch of the span, the attention pairing's chunk rank, is the caller's:
// chunk_rank(widx, launches) queues it.  Sets g->d_h.  Buffers come from `pool` in an order that depends on the handle alone.
template <class ChunkRank>
int graph_steps(asep_gnn* g, BufferPool& pool, int N, int Erows, size_t maxE, const EdgeBufs& eb, const float* d_u, const float* d_ef,
                hipStream_t s, ChunkRank chunk_rank, GraphOut& out) {
    const asep_gnn_cfg& c = g->cfg;
    long& nl = out.launches;
    const int H = g->H, I = g->I;
    const size_t nh = (size_t)N * H;
    float* h[2] = {(float*)pool.get(nh * 4), (float*)pool.get(nh * 4)};
    float* cs[2] = {(float*)pool.get(nh * 4), (float*)pool.get(nh * 4)};
    float* x = (float*)pool.get((size_t)N * std::max(I, g->Iout) * 4);
    const float* d_fed = d_u;                                // node features as fed (output_type add / concat read these)
    if (g->Wc) {                                             // compress_node_feature_dim: the fed features -> tanh(Wc x + bc)
        float* uc = (float*)pool.get((size_t)N * g->U * 4);
        COUNTED_LAUNCH(nl, gnn_compress_kernel, dim3(cdiv(N * g->U, 256)), dim3(256), 0, s, d_u, N, g->Uin, g->Wc, g->bc, g->U, uc);
        d_u = uc;
    }
    // attention-weighted aggregation: edge index of every csr entry + per-edge interaction features / attention values
    int* att_eidx = nullptr;
    int* att_widx = nullptr;
    float *att_M = nullptr, *att_A = nullptr, *att_S = nullptr;
    if (c.attention_heads > 0) {
        att_eidx = (int*)pool.get(maxE * sizeof(int));
        att_M = (float*)pool.get(maxE * c.attention_heads * g->att_xd * sizeof(float));
        att_A = (float*)pool.get(maxE * c.attention_heads * sizeof(float));
        att_S = (float*)pool.get(maxE * c.attention_heads * sizeof(float));
        att_widx = (int*)pool.get(maxE * sizeof(int));
        COUNTED_LAUNCH(nl, edge_rank_kernel, dim3(N), dim3(64), 0, s, eb.colptr, eb.tsrc, eb.rowptr, eb.sorted, N, att_eidx);
        chunk_rank(att_widx, nl);
    }
    float* upad = nullptr;
    const int mode = step_mode_of(g);
    if (mode == STEP_BIG) {
        upad = (float*)pool.get((size_t)N * g->Upad * 4);
        COUNTED_LAUNCH(nl, gnn_pad_rows_kernel, dim3(cdiv(N * g->Upad, 256)), dim3(256), 0, s, d_u, N, g->U, upad, g->Upad);
    }
    float *fPu = nullptr, *fP[2] = {nullptr, nullptr}, *fC = nullptr;
    if (mode == STEP_FACT && c.num_transition_steps > 0) {     // the step-independent parts of the edge MLP's first layer, once per launch
        fPu = (float*)pool.get((size_t)N * 64 * 4);
        fP[0] = (float*)pool.get((size_t)N * 64 * 4);
        fP[1] = (float*)pool.get((size_t)N * 64 * 4);
        fC = (float*)pool.get(maxE * 32 * 4);
        FactPreArgs fa{};
        fa.u = d_u; fa.ef = d_ef; fa.tptr = eb.colptr; fa.tsrc = eb.tsrc; fa.tfirst = eb.tfirst;
        fa.Wuu = g->Wuu; fa.Wde = g->Wde; fa.b1 = g->b1; fa.Pu = fPu; fa.C = fC;
        fa.N = N; fa.U = g->U; fa.Ed = g->Ed; fa.E = Erows;
        COUNTED_LAUNCH(nl, gnn_fact_pre_kernel, dim3(N), dim3(256), g->fact_pre_lds, s, fa);
    }
    if (mode != STEP_FACT || c.num_transition_steps == 0) {  // (the factored step's first launch does not read h / c: no memsets)
        ASEP_HIP_CHECK(hipMemsetAsync(h[0], 0, nh * 4, s));
        ASEP_HIP_CHECK(hipMemsetAsync(cs[0], 0, nh * 4, s));
    }
    int cur = 0;
    for (int t = 0; t < c.num_transition_steps; ++t) {
        if (mode == STEP_FACT) {
            StepFactArgs sa{};
            sa.u = d_u; sa.h_in = h[cur]; sa.c_in = cs[cur]; sa.tptr = eb.colptr; sa.tsrc = eb.tsrc;
            sa.P_in = t == 0 ? fPu : fP[t & 1];                // h = 0 in front of the first step: the rows are their u halves
            sa.Pu = fPu; sa.C = fC;
            sa.A1 = (const gf32x4*)g->A1f; sa.A2 = (const gf32x4*)g->A2; sa.b2 = g->b2; sa.Whh = g->Whh;
            for (int q = 0; q < 4; ++q) { sa.Wg[q] = g->Wg[q]; sa.bg[q] = g->bg[q]; }
            sa.h_out = h[cur ^ 1]; sa.c_out = cs[cur ^ 1];
            sa.P_out = t + 1 < c.num_transition_steps ? fP[(t + 1) & 1] : nullptr;
            sa.N = N; sa.U = g->U; sa.first = t == 0;
            COUNTED_LAUNCH(nl, gnn_step_fact_kernel, dim3(N), dim3(256), g->fact_lds, s, sa);
        } else if (mode == STEP_SMALL) {
            StepArgs sa{};
            sa.u = d_u; sa.h_in = h[cur]; sa.c_in = cs[cur]; sa.ef = d_ef;
            sa.tptr = eb.colptr; sa.tsrc = eb.tsrc; sa.tfirst = eb.tfirst;
            sa.A1 = (const gf32x4*)g->A1; sa.A2 = (const gf32x4*)g->A2; sa.b1 = g->b1; sa.b2 = g->b2;
            for (int q = 0; q < 4; ++q) { sa.Wg[q] = g->Wg[q]; sa.bg[q] = g->bg[q]; }
            sa.h_out = h[cur ^ 1]; sa.c_out = cs[cur ^ 1];
            sa.N = N; sa.U = g->U; sa.Ed = g->Ed; sa.E = Erows; sa.nch = g->nch;
            sa.qdesc = g->qdesc;
            COUNTED_LAUNCH(nl, gnn_step_kernel, dim3(N), dim3(256), 0, s, sa);
        } else if (mode == STEP_BIG) {
            StepBigArgs sa{};
            sa.u = upad; sa.h_in = h[cur]; sa.c_in = cs[cur]; sa.ef = d_ef;
            sa.tptr = eb.colptr; sa.tsrc = eb.tsrc; sa.tfirst = eb.tfirst;
            sa.A1 = (const gf32x4*)g->A1; sa.A2 = (const gf32x4*)g->A2; sa.b1 = g->b1; sa.b2 = g->b2;
            for (int q = 0; q < 4; ++q) { sa.Wg[q] = g->Wg[q]; sa.bg[q] = g->bg[q]; }
            sa.h_out = h[cur ^ 1]; sa.c_out = cs[cur ^ 1];
            sa.N = N; sa.U = g->U; sa.Upad = g->Upad; sa.Ed = g->Ed; sa.E = Erows; sa.nch = g->nch;
            sa.qdesc = g->qdesc;
            COUNTED_LAUNCH(nl, gnn_step_big_kernel, dim3(N), dim3(256), g->big_lds, s, sa);
        } else if (c.attention_heads > 0) {
            MsgAttArgs aa{};
            aa.u = d_u; aa.h = h[cur]; aa.ef = d_ef; aa.tptr = eb.colptr; aa.tsrc = eb.tsrc; aa.tfirst = eb.tfirst; aa.eidx = att_eidx;
            aa.hd = g->d_att_w;
            aa.M = att_M; aa.A = att_A;
            aa.N = N; aa.U = g->U; aa.Ed = g->Ed; aa.E = Erows; aa.H = H;
            aa.xd = g->att_xd; aa.heads = c.attention_heads; aa.Etot = (int)maxE; aa.maxh = g->msg_maxh;
            const size_t lds = ((size_t)g->K + 2 * (size_t)g->msg_maxh) * sizeof(float);
            COUNTED_LAUNCH(nl, gnn_msg_att_kernel, dim3(N), dim3(256), lds, s, aa);
            COUNTED_LAUNCH(nl, gnn_att_softmax_kernel, dim3(N), dim3(64), 0, s, eb.colptr, att_eidx, att_A, c.attention_heads, (int)maxE, att_S);
            COUNTED_LAUNCH(nl, gnn_att_aggregate_kernel, dim3(N), dim3(64), 0, s, eb.colptr, att_eidx, att_widx, att_S, att_M, c.attention_heads,
                           g->att_xd, (int)maxE, c.attention_merge, c.aggregation_type, x);
        } else {
            MsgGenArgs ma{};
            ma.u = d_u; ma.h = h[cur]; ma.ef = d_ef; ma.tptr = eb.colptr; ma.tsrc = eb.tsrc; ma.tfirst = eb.tfirst;
            ma.mlp = g->msg; ma.x = x;
            ma.N = N; ma.U = g->U; ma.Ed = g->Ed; ma.E = Erows; ma.H = H; ma.I = I; ma.maxh = g->msg_maxh;
            ma.agg_max = c.aggregation_type;
            const size_t lds = ((size_t)g->K + 2 * (size_t)g->msg_maxh + I) * sizeof(float);
            COUNTED_LAUNCH(nl, gnn_message_generic_kernel, dim3(N), dim3(256), lds, s, ma);
        }
        if (mode == STEP_GENERIC) {                          // (the fused step kernels contain the LSTM update)
            LstmGenArgs la{};
            la.x = x; la.h_in = h[cur]; la.c_in = cs[cur]; la.u = d_u;
            for (int q = 0; q < 4; ++q) { la.Wg[q] = g->Wg[q]; la.bg[q] = g->bg[q]; }
            la.h_out = h[cur ^ 1]; la.c_out = cs[cur ^ 1]; la.N = N; la.U = g->U; la.H = H; la.I = g->Iout;
            la.use_h = c.lstm_use_hidden; la.use_u = c.lstm_use_input;
            COUNTED_LAUNCH(nl, gnn_lstm_generic_kernel, dim3(cdiv(N * H, 256)), dim3(256), 0, s, la);
        }
        cur ^= 1;
    }
    g->d_h = h[cur];
    out.hcls = h[cur];
    out.Hc = H;
    if (c.output_type != 0) {                                // graph_gnn.py:158-166
        out.Hc = c.output_type == 2 ? H + g->Uin : H;
        float* y = (float*)pool.get((size_t)N * out.Hc * 4);
        COUNTED_LAUNCH(nl, gnn_output_type_kernel, dim3(cdiv(N * out.Hc, 256)), dim3(256), 0, s, h[cur], d_fed, N, H, g->Uin, g->Wout,
                       c.output_type, y);
        out.hcls = y;
    }
    return ASEP_OK;
}

// the pair classifier's arguments in both forms (cls_fast says which kernel runs); N and R stay 0: only the single-page kernels read them
void pair_args(const asep_gnn* g, const float* Pt, const float* Qt, const int32_t* rel, float* out, PairArgs& pa, PairGenArgs& pg) {
    pa.Pt = Pt; pa.Qt = Qt; pa.b1 = g->cb1; pa.W2 = g->C2; pa.b2 = g->cb2; pa.W3 = g->C3; pa.b3 = g->cb3;
    pa.rel = rel; pa.out = out;
    pg.Pt = Pt; pg.Qt = Qt; pg.b1 = g->cb1; pg.rest = g->cls_rest; pg.rel = rel; pg.out = out;
    pg.maxw = g->cls_maxw;
}

int forward_impl(asep_gnn* g, BufferPool& pool, int N, int E, const int32_t* d_edges, const float* d_u, const float* d_ef, int R,
                 const int32_t* d_rel, float* d_out, hipStream_t s) {
    const asep_gnn_cfg& c = g->cfg;
    if (N < 1 || E < 0 || R < 0) { set_error("asep_gnn_forward: bad sizes N=%d E=%d R=%d", N, E, R); return ASEP_ERR_ARG; }
    if ((size_t)N * N > (size_t)1 << 30) { set_error("asep_gnn_forward: N=%d too large for the dense edge table", N); return ASEP_ERR_UNSUPPORTED; }
    g->stream = s;
    g->N = N;
    ++g->fwd_serial;
    pool.begin();
    EdgeBufs eb{};
    int rc = correct_edges_dev(g, pool, N, E, d_edges, eb, s);
    if (rc) return rc;
    GraphOut go;
    auto chunk_rank = [&](int* widx, long& nl) {
        const int chunk_nodes = std::max(1, 100000 / N);      // message_fn_chunk.py:77-78
        COUNTED_LAUNCH(nl, edge_chunk_rank_kernel, dim3(cdiv(N, chunk_nodes)), dim3(256), 0, s, eb.sorted, eb.rowptr, eb.colptr, N, chunk_nodes, widx);
    };
    rc = graph_steps(g, pool, N, std::max(E, 1), (size_t)(c.undirected_graph ? 2 : 1) * std::max(E, 1), eb, d_u, d_ef, s, chunk_rank, go);
    if (rc) return rc;
    float* Pt = (float*)pool.get((size_t)N * c.cls_hidden1 * 4);
    float* Qt = (float*)pool.get((size_t)N * c.cls_hidden1 * 4);
    if (R > 0) {
        hipLaunchKernelGGL(gnn_pair_pre_kernel, dim3(std::min(cdiv(N * c.cls_hidden1, 256), 1024)), dim3(256), 0, s,
                           go.hcls, N, go.Hc, g->C1, c.cls_hidden1, Pt, Qt);
        PairArgs pa{};
        PairGenArgs pg{};
        pair_args(g, Pt, Qt, d_rel, d_out, pa, pg);
        pa.N = pg.N = N; pa.R = pg.R = R;
        if (g->cls_fast)
            hipLaunchKernelGGL((gnn_pair_cls_kernel<64, 32, 2>), dim3(cdiv(R, 256)), dim3(256), 0, s, pa);
        else
            hipLaunchKernelGGL(gnn_pair_cls_generic_kernel, dim3(cdiv(R, PAIRG_P)), dim3(256), 2 * (size_t)PAIRG_P * g->cls_maxw * sizeof(float), s, pg);
    }
    ASEP_HIP_CHECK(hipGetLastError());
    return ASEP_OK;
}

// The inputs of a host-pointer graph entry (one page or the pages of a call; the totals) in the handle's grow-only device staging, queued for
// upload on the null stream, and room for `outs` output floats: hipMalloc / hipFree pairs per call would cost more than the GNN.  A pointer is
// null where its array is absent or empty.  Throws HipError.
struct StagedGraph { int32_t* e; float* u; float* f; int32_t* r; float* o; };
StagedGraph stage_graph(asep_gnn* g, size_t nodes, size_t edges, size_t rels, size_t outs, const int32_t* h_edges, const float* node_feat,
                        const float* edge_feat, const int32_t* relations) {
    BufferPool& p = g->host_stage;
    p.begin();
    auto up = [&p](auto* src, size_t n) { auto* d = upload(p, nullptr, src, n); return n ? d : nullptr; };   // (a slot per array, present or not)
    StagedGraph st{};
    st.e = up(h_edges, edges * 2);
    st.u = upload(p, nullptr, node_feat, nodes * g->Uin);        // (features as fed: width Uin; never null)
    st.f = up(edge_feat, edge_feat ? edges * g->Ed : 0);
    st.r = up(relations, relations ? rels * 2 : 0);
    st.o = (float*)p.get(std::max<size_t>(outs, 1) * sizeof(float));
    return st;
}

// ---- the visual branch in front of the graph (graph_relation.py:84-172): what its three entries share --------------------------------------

asep_gnn::FmapRef map_ref(const float* p, const FmapShape& m) { return asep_gnn::FmapRef{p, m.fh, m.fw, m.C, m.bf}; }

// the per-page arguments of the single (b < 0: its message names no page), the uniform and the table entries
int check_visual_page(const asep_gnn* g, const char* fn, int b, const asep_gnn_page& q, bool need_image) {
    const int ug = g->Uin - g->vis_total;
    if (q.N < 1 || q.E < 0 || q.R < 0 || (need_image && !q.d_image) || !q.d_regions || !q.d_num_points || (ug > 0 && !q.d_node_feat) ||
        (q.E > 0 && !q.d_edges) || (q.R > 0 && !q.d_probs_out) || (g->Ed_fed > 0 && q.E > 0 && !q.d_edge_feat) ||
        (g->vise_total > 0 && q.E > 0 && (!q.d_edge_regions || !q.d_edge_num_points))) {
        if (b < 0) set_error("%s: bad argument", fn);
        else set_error("%s: bad argument in page %d", fn, b);
        return ASEP_ERR_ARG;
    }
    return ASEP_OK;
}

// the compression layer "<scope>weights" [C, d] / "<scope>bias" [d] of a map of C channels (nodes' or interactions' side), owned through vis_owned
int upload_compression(asep_gnn* g, const std::string& scope, int C, float** dW, float** db, int* d) {
    auto w = g->vis_blob.find(scope + "weights"), b = g->vis_blob.find(scope + "bias");
    if (w == g->vis_blob.end() || b == g->vis_blob.end()) { set_error("weights: missing tensor %sweights|bias", scope.c_str()); return ASEP_ERR_WEIGHTS; }
    if (w->second.dims.size() != 2 || w->second.dims[0] != C || b->second.dims.size() != 1 || b->second.dims[0] != w->second.dims[1]) {
        set_error("weights: %sweights must be [%d, d] with a matching bias", scope.c_str(), C);
        return ASEP_ERR_WEIGHTS;
    }
    *d = w->second.dims[1];
    int rc = upload_named(g->vis_owned, g->vis_blob, scope + "weights", w->second.dims, dW);
    if (!rc) rc = upload_named(g->vis_owned, g->vis_blob, scope + "bias", b->second.dims, db);
    return rc;
}

int reserve_floats(float** p, size_t* cap, size_t n) {         // a grow-only buffer of the handle (d_u_cat, d_ef_cat)
    if (*cap < n) {
        if (*p) (void)hipFree(*p);
        *p = nullptr; *cap = 0;
        ASEP_HIP_CHECK(hipMalloc((void**)p, n * sizeof(float)));
        *cap = n;
    }
    return ASEP_OK;
}

int endpoint_ref(asep_gnn* g, const std::string& name, asep_gnn::FmapRef* m) {
    int dims[3];
    int rc = aru_endpoint_dev(g->backbone, name.c_str(), &m->p, dims, &m->bf);
    if (rc) return rc;
    m->fh = dims[0]; m->fw = dims[1]; m->C = dims[2];
    return ASEP_OK;
}

// The maps of the page whose backbone end points are "<prefix><name>" of the forward that is queued: the plan of launch_plan.h over the handle's
// layout, with the end points' addresses (end_p[i] where map i is or reads one), and its channel verdicts as errors.
int page_map_plan(asep_gnn* g, const std::string& prefix, std::vector<FmapStep>& plan, std::vector<const float*>& end_p) {
    const size_t n = g->vis_names.size();
    std::vector<FmapSpec> spec(n);
    std::vector<FmapShape> ends(n, FmapShape{});
    end_p.assign(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        const asep_gnn::FmapGen& G = g->vis_gen[i];
        spec[i] = FmapSpec{G.depth, G.stride, G.Cin};
        if (G.depth >= 0 && G.stride != 1) continue;        // (reads map i - 1)
        asep_gnn::FmapRef m{};
        int rc = endpoint_ref(g, prefix + g->vis_names[i], &m);
        if (rc) return rc;
        end_p[i] = m.p;
        ends[i] = FmapShape{m.fh, m.fw, m.C, m.bf};
    }
    plan = fmap_plan(spec.data(), ends.data(), g->vis_C.data(), (int)n);
    for (size_t i = 0; i < n; ++i) {
        if (!plan[i].bad_channels) continue;
        if (plan[i].generated) set_error("feature map %zu reads %d channels, its 1x1 filter was loaded for %d", i, plan[i].in.C, spec[i].Cin);
        else set_error("end point %s has %d channels, expected %d", g->vis_names[i].c_str(), plan[i].out.C, g->vis_C[i]);
        return ASEP_ERR_ARG;
    }
    return ASEP_OK;
}

// One record of the backbone's launch profile (aru_prof_begin / aru_prof_end) around the launches that follow it in its block: the visual
// stage's kernels are timed in the backbone's report.  Closed on every way out of the block.
struct ProfiledLaunch {
    void* scope;
    ProfiledLaunch(asep_gnn* g, const char* name, const std::string& detail, double flops, double bytes)
        : scope(aru_prof_begin(g->backbone, name, detail.c_str(), flops, bytes)) {}
    ~ProfiledLaunch() { aru_prof_end(scope); }
};

// feature_map_generators.py:140-194 for the page whose backbone end points are "<prefix><name>" of the forward queued on s: every generated
// map into the handle's arena (two launches each, fmap_kernels.h), every map's address into g->fmap_last.  A layout without generated
// maps returns at once: it allocates and launches nothing.
int generate_maps_dev(asep_gnn* g, const std::string& prefix, hipStream_t s) {
    if (g->n_generated == 0) return ASEP_OK;
    std::vector<FmapStep> plan;
    std::vector<const float*> end_p;
    int rc = page_map_plan(g, prefix, plan, end_p);
    if (rc) return rc;
    g->fmap_last.assign(plan.size(), asep_gnn::FmapRef{});
    g->fmap_last_prefix = prefix;
    for (size_t i = 0; i < plan.size(); ++i) {
        const FmapStep& k = plan[i];
        if (!k.generated) { g->fmap_last[i] = map_ref(end_p[i], k.out); continue; }
        const asep_gnn::FmapGen& G = g->vis_gen[i];
        const int half = G.depth / 2;
        FmapConvArgs a{};
        a.in = k.src < 0 ? end_p[i] : g->fmap_last[k.src].p; a.W = G.W1; a.b = G.b1; a.ih = k.d.ih; a.iw = k.d.iw; a.Ci = k.in.C; a.Co = half;
        a.oh = k.d.ih; a.ow = k.d.iw; a.stride = 1;
        float* mid = (float*)g->fmap_pool.get(k.n1 * sizeof(float));
        a.out = mid;
        FmapConvArgs c{};
        c.in = mid; c.W = G.W2; c.b = G.b2; c.ih = k.d.ih; c.iw = k.d.iw; c.Ci = half; c.Co = G.depth; c.stride = G.stride;
        c.oh = k.d.oh; c.ow = k.d.ow; c.pad_t = k.d.pad_t; c.pad_l = k.d.pad_l;
        c.out = (float*)g->fmap_pool.get(k.n2 * sizeof(float));
        if (k.n1 + 255 > ((size_t)1 << 31) * 256 || k.n2 + 255 > ((size_t)1 << 31) * 256) { set_error("feature map %zu is too large for one launch", i); return ASEP_ERR_UNSUPPORTED; }
        const std::string where = "fm_" + std::to_string(i) + " " + std::to_string(k.d.ih) + "x" + std::to_string(k.d.iw);
        {
            ProfiledLaunch pl(g, k.in.bf ? "fmap_conv1x1_kernel<true>" : "fmap_conv1x1_kernel<false>", where + " " + std::to_string(k.in.C) + "->" + std::to_string(half), k.fl1, k.io1 + k.w1);
            if (k.in.bf) hipLaunchKernelGGL(fmap_conv1x1_kernel<true>, dim3((unsigned)((k.n1 + 255) / 256)), dim3(256), 0, s, a);
            else hipLaunchKernelGGL(fmap_conv1x1_kernel<false>, dim3((unsigned)((k.n1 + 255) / 256)), dim3(256), 0, s, a);
        }
        {
            ProfiledLaunch pl(g, "fmap_conv3x3_kernel", where + " " + std::to_string(half) + "->" + std::to_string(G.depth) + " s" + std::to_string(G.stride), k.fl3, k.io3 + k.w3);
            hipLaunchKernelGGL(fmap_conv3x3_kernel, dim3((unsigned)((k.n2 + 255) / 256)), dim3(256), 0, s, c);
        }
        g->fmap_last[i] = map_ref(c.out, k.out);
    }
    ASEP_HIP_CHECK(hipGetLastError());
    return ASEP_OK;
}

// map i of the page "<prefix>": the backbone's end point (the default layout: exactly the lookup the ROI launchers always made) or, in a
// layout with generated maps, what generate_maps_dev left for this page
int visual_map_dev(asep_gnn* g, const std::string& prefix, size_t i, asep_gnn::FmapRef* m) {
    if (g->n_generated == 0) return endpoint_ref(g, prefix + g->vis_names[i], m);
    if (i >= g->fmap_last.size() || !g->fmap_last[i].p || g->fmap_last_prefix != prefix) { set_error("feature map %zu of this page was not generated", i); return ASEP_ERR_ARG; }
    *m = g->fmap_last[i];
    return ASEP_OK;
}

// ROI max + compression (graph_relation.py:84-172, misc.py:384-470) has two sides, the nodes' regions and the interactions': per map a
// compression layer d[i] wide whose output goes behind the `fed` columns of the features as fed, in rows `stride` wide.  want_C: the maps'
// channels where the side checks them (the nodes' side)
struct RoiSide { const std::vector<float*>& W; const std::vector<float*>& b; const std::vector<int>& d; int fed, stride; const int* want_C; };
RoiSide node_side(const asep_gnn* g) { return RoiSide{g->vis_W, g->vis_b, g->vis_d, g->Uin - g->vis_total, g->Uin, g->vis_C.data()}; }
RoiSide edge_side(const asep_gnn* g) { return RoiSide{g->vise_W, g->vise_b, g->vise_d, g->Ed_fed, g->Ed, nullptr}; }

// one launch's (or one table entry's) arguments: the regions of one page on map i -> columns col .. col + d[i] - 1 of out
RoiArgs roi_entry(const asep_gnn::FmapRef& m, const float* regions, int P, const int32_t* npts, const RoiSide& sd, size_t i, float* out, int col) {
    RoiArgs a{};
    a.fm = m.p; a.fh = m.fh; a.fw = m.fw; a.C = m.C;
    a.regions = regions; a.P = P; a.npts = npts; a.Wc = sd.W[i]; a.bc = sd.b[i]; a.d = sd.d[i];
    a.u_out = out; a.ustride = sd.stride; a.col0 = col; a.vmax_out = nullptr;
    return a;
}

// the fed columns of a side: d_fed [rows, fed] -> the first columns of d_out [rows, stride].  The per-page schedule queues this in front of the
// page's ROI kernels, the table schedule behind its ROI launch (disjoint columns: the results do not depend on the order)
void copy_fed_cols(const RoiSide& sd, int rows, const float* d_fed, float* d_out, hipStream_t s) {
    if (sd.fed > 0) hipLaunchKernelGGL(gnn_copy_cols_kernel, dim3(cdiv(rows * sd.fed, 256)), dim3(256), 0, s, d_fed, rows, sd.fed, d_out, sd.stride);
}

// one side of one page from the maps "<prefix>..." of the forward that is queued on s: d_fed [rows, fed] -> d_out [rows, stride]
int visual_rois_dev(asep_gnn* g, const RoiSide& sd, int rows, const float* d_fed, const std::string& prefix, const float* d_reg, int P,
                    const int32_t* d_np, float* d_out, hipStream_t s) {
    if (rows < 1) return ASEP_OK;
    copy_fed_cols(sd, rows, d_fed, d_out, s);
    int col = sd.fed;
    for (size_t i = 0; i < g->vis_names.size(); ++i) {
        asep_gnn::FmapRef m{};                              // (a bf16 backbone, compute_dtype 1, hands over bf16 maps)
        int rc = visual_map_dev(g, prefix, i, &m);
        if (rc) return rc;
        if (sd.want_C && m.C != sd.want_C[i]) { set_error("end point %s has %d channels, expected %d", g->vis_names[i].c_str(), m.C, sd.want_C[i]); return ASEP_ERR_ARG; }
        const RoiArgs a = roi_entry(m, d_reg, P, d_np, sd, i, d_out, col);
        if (m.bf) hipLaunchKernelGGL(gnn_roi_compress_kernel<true>, dim3(rows), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(gnn_roi_compress_kernel<false>, dim3(rows), dim3(256), 0, s, a);
        col += sd.d[i];
    }
    ASEP_HIP_CHECK(hipGetLastError());
    return ASEP_OK;
}

// The graph of one page whose features are in place: its node rows at *d_u and, where the model has interaction visual features and the page
// interactions, its edge rows at *d_efc (the fed edge features otherwise).  Both cursors move on to the next page's rows.
int visual_graph_dev(asep_gnn* g, const asep_gnn_page& q, float** d_u, float** d_efc, hipStream_t s) {
    const float* d_ef = q.d_edge_feat;
    if (g->vise_total > 0 && q.E > 0) {
        d_ef = *d_efc;
        *d_efc += (size_t)q.E * g->Ed;
    }
    int rc = forward_impl(g, g->pool, q.N, q.E, q.d_edges, *d_u, d_ef, q.R, q.d_relations, q.d_probs_out, s);
    if (rc) return rc;
    *d_u += (size_t)q.N * g->Uin;
    return ASEP_OK;
}

// Everything of one page behind its backbone forward, queued on s: generated maps, ROI max + compression of nodes and interactions, the graph.
// The page's rows go to *d_u (and *d_efc), which move on to the next page's.
int visual_page_dev(asep_gnn* g, const asep_gnn_page& q, const std::string& prefix, int P, float** d_u, float** d_efc, hipStream_t s) {
    g->fmap_pool.begin();                                   // the pages of a call share the arena's buffers: page b + 1's generator is ordered behind page b's ROI kernels
    int rc = generate_maps_dev(g, prefix, s);
    if (rc) return rc;
    rc = visual_rois_dev(g, node_side(g), q.N, q.d_node_feat, prefix, q.d_regions, P, q.d_num_points, *d_u, s);
    if (rc) return rc;
    if (g->vise_total > 0 && q.E > 0) {
        rc = visual_rois_dev(g, edge_side(g), q.E, q.d_edge_feat, prefix, q.d_edge_regions, P, q.d_edge_num_points, *d_efc, s);
        if (rc) return rc;
    }
    return visual_graph_dev(g, q, d_u, d_efc, s);
}

// The body of asep_gnn_forward_visual_dev (one page; name_pages = false: its messages name no page) and asep_gnn_forward_visual_batch_dev
// (pages of ONE size): ONE grouped backbone forward for all pages (every layer is one launch over the page list), then per page the generated
// maps, the ROI kernels and the graph, queued back to back on the same stream.  h, w and P are checked in front of the pages, and the buffers
// are reserved in front of the backbone forward.
int visual_uniform_impl(asep_gnn* g, const char* fn, int n_pages, const asep_gnn_page* pages, int h, int w, int P, hipStream_t s, bool name_pages) {
    if (!g || !g->backbone) { set_error("%s: no backbone attached", fn); return ASEP_ERR_ARG; }
    if (n_pages < 1 || !pages || h < 1 || w < 1 || P < 1) { set_error("%s: bad argument", fn); return ASEP_ERR_ARG; }
    size_t nu = 0, nef = 0;
    for (int b = 0; b < n_pages; ++b) {
        if (int rc = check_visual_page(g, fn, name_pages ? b : -1, pages[b], true)) return rc;
        nu += (size_t)pages[b].N * g->Uin;
        if (g->vise_total > 0) nef += (size_t)pages[b].E * g->Ed;
    }
    g->vis_pool.begin();
    const int ncls = std::max(1, aru_num_classes(g->backbone));
    std::vector<const float*> imgs(n_pages); std::vector<float*> outs(n_pages);
    for (int b = 0; b < n_pages; ++b) {
        imgs[b] = pages[b].d_image;
        outs[b] = (float*)g->vis_pool.get((size_t)h * w * ncls * sizeof(float));      // backbone logits (not used by the graph)
    }
    int rc = reserve_floats(&g->d_u_cat, &g->u_cat_cap, nu);
    if (!rc && nef) rc = reserve_floats(&g->d_ef_cat, &g->ef_cat_cap, nef);
    if (rc) return rc;
    // (one page through the batch entry is the single entry's forward: both hand the same one-page list to the backbone's forward_lanes)
    rc = asep_aru_forward_batch_dev(g->backbone, n_pages, imgs.data(), h, w, outs.data(), nullptr, nullptr, 0.f, s);
    if (rc) return rc;
    float *d_u = g->d_u_cat, *d_efc = g->d_ef_cat;
    for (int b = 0; b < n_pages; ++b)
        if ((rc = visual_page_dev(g, pages[b], page_prefix(b), P, &d_u, &d_efc, s))) return rc;
    return ASEP_OK;
}

// read-backs (tests): a map as fp32 [fh, fw, C] (out == nullptr: the sizes only), and N rows of the concatenated node features from row offset off
int copy_map_out(asep_gnn* g, const char* fn, const asep_gnn::FmapRef& r, float* out, size_t max_floats, int32_t dims[3]) {
    dims[0] = r.fh; dims[1] = r.fw; dims[2] = r.C;
    const size_t n = (size_t)r.fh * r.fw * r.C;
    if (!out) return ASEP_OK;
    if (max_floats < n) { set_error("%s: buffer too small (%zu floats needed)", fn, n); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipStreamSynchronize(g->stream));
    if (r.bf) {                                             // a bf16 end point widens exactly
        std::vector<uint16_t> hb(n);
        ASEP_HIP_CHECK(hipMemcpy(hb.data(), r.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) { const uint32_t u = (uint32_t)hb[i] << 16; memcpy(out + i, &u, 4); }
    } else {
        ASEP_HIP_CHECK(hipMemcpy(out, r.p, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return ASEP_OK;
}

int copy_node_features_out(asep_gnn* g, const char* fn, size_t off, int N, float* out, size_t max_floats) {
    const size_t n = (size_t)N * g->Uin;
    if (max_floats < n) { set_error("%s: buffer too small", fn); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipStreamSynchronize(g->stream));
    ASEP_HIP_CHECK(hipMemcpy(out, g->d_u_cat + off, n * sizeof(float), hipMemcpyDeviceToHost));
    return ASEP_OK;
}

// host-side checks of the index arrays (the reference's tf.gather would raise on them)
int check_indices(const char* what, const int32_t* idx, size_t n_pairs, int N) {
    for (size_t i = 0; i < 2 * n_pairs; ++i)
        if (idx[i] < 0 || idx[i] >= N) {
            set_error("%s[%zu] = (%d, %d) names a node outside 0..%d", what, i / 2, idx[i & ~(size_t)1], idx[i | 1], N - 1);
            return ASEP_ERR_ARG;
        }
    return ASEP_OK;
}

}  // namespace

extern "C" {

asep_gnn* asep_gnn_load(const void* weight_blob, size_t nbytes, const asep_gnn_cfg* cfg) {
    ASEP_GUARD_BEGIN
    if (!cfg || !weight_blob) { set_error("asep_gnn_load: null argument"); return nullptr; }
    if (cfg->struct_size != (int32_t)sizeof(asep_gnn_cfg)) {
        set_error("asep_gnn_load: cfg.struct_size is %d, this library's asep_gnn_cfg has %zu bytes (ABI version %d): the binding was "
                  "written against another include/asep_hip.h", cfg->struct_size, sizeof(asep_gnn_cfg), ASEP_ABI_VERSION);
        return nullptr;
    }
    if (cfg->node_feature_dim < 1 || cfg->edge_feature_dim < 0 || cfg->num_transition_steps < 0 || cfg->hidden_dim < 1 ||
        cfg->interaction_dim < 1 || cfg->interaction_hidden < 1 || cfg->cls_hidden1 < 1 || cfg->cls_hidden2 < 0 ||
        cfg->num_classes < 1 || cfg->num_classes > 16 || cfg->visual_edge_dims < 0 || cfg->visual_edge_dims > cfg->edge_feature_dim) {
        set_error("asep_gnn_load: bad cfg");
        return nullptr;
    }
    if (cfg->aggregation_type != 0 && cfg->aggregation_type != 1) {
        set_error("asep_gnn_load: aggregation_type %d unknown (0 = 'sum', 1 = 'max'; message_fn_chunk.py:57-62)", cfg->aggregation_type);
        return nullptr;
    }
    std::map<std::string, HostTensor> blob;
    if (!parse_blob(weight_blob, nbytes, blob)) return nullptr;
    std::unique_ptr<asep_gnn> g(new asep_gnn());
    g->cfg = *cfg;
    g->cfg.lstm_use_hidden = cfg->lstm_use_hidden != 0;
    g->cfg.lstm_use_input = cfg->lstm_use_input != 0;
    const int U = g->U = cfg->node_feature_dim, Ed = g->Ed = cfg->edge_feature_dim;
    const int H = g->H = cfg->hidden_dim, I = g->I = cfg->interaction_dim, Hm = g->Hm = cfg->interaction_hidden;
    g->Ed_fed = Ed - cfg->visual_edge_dims;
    g->K = 4 * U + Ed + 4 * H;
    g->Uin = cfg->compress_input_dim > 0 ? cfg->compress_input_dim : U;
    const std::vector<int> ih = hidden_list({cfg->interaction_hidden, cfg->interaction_hidden2, cfg->interaction_hidden3, cfg->interaction_hidden4});
    const std::vector<int> ah = hidden_list({cfg->attention_hidden, cfg->attention_hidden2, cfg->attention_hidden3, cfg->attention_hidden4});
    const std::vector<int> ch = hidden_list({cfg->cls_hidden1, cfg->cls_hidden2, cfg->cls_hidden3, cfg->cls_hidden4});
    const std::string m = MSG, u = UPD, c = CLS;
    const int heads = cfg->attention_heads;
    int rc = ASEP_OK;
    if (heads < 0 || heads > GNN_MAX_HEADS || (heads > 0 && (cfg->attention_hidden < 1 || (cfg->attention_merge != 0 && cfg->attention_merge != 1)))) {
        set_error("asep_gnn_load: bad attention configuration (heads %d of at most %d, hidden %d, merge %d)", heads, GNN_MAX_HEADS,
                  cfg->attention_hidden, cfg->attention_merge);
        return nullptr;
    }
    g->msg_maxh = *std::max_element(ih.begin(), ih.end());
    if (heads > 0) g->msg_maxh = std::max(g->msg_maxh, *std::max_element(ah.begin(), ah.end()));
    // LDS of the generic message kernels: z + two scratch vectors (+ the accumulators); refused here, not at the first forward
    if (((size_t)g->K + 2 * (size_t)g->msg_maxh + I) * sizeof(float) > 60 * 1024) {
        set_error("asep_gnn_load: edge-MLP input width %d with hidden layers up to %d needs more LDS than a workgroup may use", g->K, g->msg_maxh);
        return nullptr;
    }
    g->Iout = I;
    if (heads > 0) {
        // message_fn_chunk.py:69-72: x_dim = interaction_dim // heads for 'concat' (the LSTM then reads heads * x_dim columns)
        if (cfg->attention_merge == 0 && I % heads != 0) {
            set_error("asep_gnn_load: interaction_dim %d is not a multiple of %d attention heads (merge 'concat')", I, heads);
            return nullptr;
        }
        g->att_xd = cfg->attention_merge == 0 ? I / heads : I;
        g->Iout = cfg->attention_merge == 0 ? heads * g->att_xd : I;
        for (int k = 0; k < heads && !rc; ++k) {
            const std::string hk = "GraphLSTM1/message_fn_default/head_" + std::to_string(k) + "/";
            const std::string mi = hk + "calculation_interaction_features/concat_u_and_h/interaction_features";
            const std::string ma = hk + "calculation_unnormalized_attention_values/calculation_interaction_features/concat_u_and_h/interaction_features";
            rc = upload_mlp(g.get(), blob, mi, g->K, ih, g->att_xd, &g->att_w[k].inter);
            if (!rc) rc = upload_mlp(g.get(), blob, ma, g->K, ah, 1, &g->att_w[k].att);
        }
        if (!rc) {
            std::vector<AttHeadW> hw(g->att_w, g->att_w + heads);
            rc = upload_vec(g.get(), hw, &g->d_att_w);
        }
    } else {
        rc = upload_mlp(g.get(), blob, m, g->K, ih, I, &g->msg);
        if (!rc && ih.size() == 1) { g->b1 = const_cast<float*>(g->msg.b[0]); g->b2 = const_cast<float*>(g->msg.b[1]); }
    }
    g->V = g->Iout + (g->cfg.lstm_use_hidden ? H : 0) + (g->cfg.lstm_use_input ? U : 0);      // update_fn_lstm.py:41-50
    const char* gates[4] = {"ingate", "outgate", "forgetgate", "cellinput"};
    for (int q = 0; q < 4 && !rc; ++q) {
        rc = upload_named(g->owned, blob, u + "/" + gates[q] + "_activation/dense/weights", {g->V, H}, &g->Wg[q]);
        if (!rc) rc = upload_named(g->owned, blob, u + "/" + gates[q] + "_activation/dense/bias", {H}, &g->bg[q]);
    }
    if (cfg->output_type < 0 || cfg->output_type > 2) { set_error("asep_gnn_load: output_type %d unknown (0 hidden, 1 add, 2 concat)", cfg->output_type); return nullptr; }
    const int Hc = cfg->output_type == 2 ? H + g->Uin : H;   // width of the node vectors the classifier pairs up
    if (!rc) rc = upload_named(g->owned, blob, c + "/fully_connected_layer_h1/weights", {2 * Hc, cfg->cls_hidden1}, &g->C1);
    if (!rc && cfg->output_type == 1) rc = upload_named(g->owned, blob, "GraphLSTM1/dense/weights", {g->Uin, H}, &g->Wout);
    if (!rc) rc = upload_named(g->owned, blob, c + "/fully_connected_layer_h1/bias", {cfg->cls_hidden1}, &g->cb1);
    if (!rc) rc = upload_mlp(g.get(), blob, c, 2 * Hc, ch, cfg->num_classes, &g->cls_rest, /*first_layer=*/1);
    if (!rc) {
        g->cls_maxw = std::max(cfg->num_classes, *std::max_element(ch.begin(), ch.end()));
        g->cls_fast = ch.size() == 2 && ch[0] == 64 && ch[1] == 32 && cfg->num_classes == 2;
        if (g->cls_fast) {                                   // the specialised kernel's operand names
            g->C2 = const_cast<float*>(g->cls_rest.W[0]); g->cb2 = const_cast<float*>(g->cls_rest.b[0]);
            g->C3 = const_cast<float*>(g->cls_rest.W[1]); g->cb3 = const_cast<float*>(g->cls_rest.b[1]);
        }
        if (2 * (size_t)PAIRG_P * g->cls_maxw * sizeof(float) > 60 * 1024) {
            set_error("asep_gnn_load: classifier layers up to %d wide need more LDS than a workgroup may use", g->cls_maxw);
            return nullptr;
        }
    }
    if (!rc && cfg->compress_input_dim > 0) {
        rc = upload_named(g->owned, blob, "GraphLSTM1/compress_input/ff_compress_input/weights", {g->Uin, U}, &g->Wc);
        if (!rc) rc = upload_named(g->owned, blob, "GraphLSTM1/compress_input/ff_compress_input/bias", {U}, &g->bc);
    }
    if (rc) return nullptr;
    for (auto& kv : blob)
        if (kv.first.rfind("visual_node_feature_compression_fm_", 0) == 0 || kv.first.rfind("visual_edge_feature_compression_fm_", 0) == 0 ||
            kv.first.find("_Conv2d_") != std::string::npos)       // (the feature-map generator's convolutions, asep_gnn_attach_backbone_maps)
            g->vis_blob[kv.first] = kv.second;
    warn_ignored_switches();
    if (const char* ev = getenv("ASEP_GNN_STEP")) g->use_step = atoi(ev) != 0;
    if (const char* ev = getenv("ASEP_GNN_FACTOR")) g->use_fact = atoi(ev) != 0;
    // the fused MFMA step kernels serve the reference's defaults: widths 32 / [32] / 32, degree-normalised SUM, both LSTM inputs
    const bool default_widths = H == GNN_H && I == GNN_H && Hm == GNN_H && ih.size() == 1 && heads == 0 && cfg->aggregation_type == 0 &&
                                g->cfg.lstm_use_hidden && g->cfg.lstm_use_input;
    g->mode = STEP_GENERIC;
    if (default_widths && Ed <= 4) {
        if (U <= 8) {
            if (pack_step_fragments(g.get(), blob, false)) return nullptr;
            if (g->nch <= GNN_MAXCH) g->mode = STEP_SMALL;
        }
        if (g->mode == STEP_GENERIC && U <= 120) {
            g->Upad = (U + 3) & ~3;
            if (pack_step_fragments(g.get(), blob, true)) return nullptr;
            g->big_lds = ((size_t)g->nch * 512 + g->Upad + 32) * sizeof(float);
            if (g->big_lds <= 150 * 1024 &&
                hipFuncSetAttribute((const void*)gnn_step_big_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->big_lds) == hipSuccess)
                g->mode = STEP_BIG;
        }
    }
    if (g->mode != STEP_GENERIC) {                          // the factored step for the same widths (any U whose filters fit the pre kernel's LDS)
        g->fact_pre_lds = ((size_t)(U + Ed) * 32 + U) * sizeof(float);
        g->fact_lds = (size_t)(64 + U) * sizeof(float);
        if (g->fact_pre_lds <= 60 * 1024) {
            if (pack_fact(g.get(), blob)) return nullptr;
        }
    }
    const size_t lds = ((size_t)g->K + 2 * (size_t)g->msg_maxh + I) * sizeof(float);
    if (hipFuncSetAttribute((const void*)gnn_message_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipFuncSetAttribute((const void*)gnn_msg_att_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipFuncSetAttribute((const void*)gnn_pair_cls_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(2 * (size_t)PAIRG_P * g->cls_maxw * sizeof(float))) != hipSuccess) {
        set_error("asep_gnn_load: cannot reserve %zu bytes of LDS", lds);
        return nullptr;
    }
    return g.release();
    ASEP_GUARD_END_PTR
}

void asep_gnn_free(asep_gnn* g) { delete g; }

int asep_gnn_forward_dev(asep_gnn* g, int N, int E, const int32_t* d_edges, const float* d_node_feat,
                         const float* d_edge_feat, int R, const int32_t* d_relations, float* d_probs_out, void* stream) {
    ASEP_GUARD_BEGIN
    if (!g || !d_node_feat || (E > 0 && !d_edges) || (R > 0 && !d_probs_out)) { set_error("asep_gnn_forward_dev: null argument"); return ASEP_ERR_ARG; }
    if (g->cfg.edge_feature_dim > 0 && E > 0 && !d_edge_feat) { set_error("asep_gnn_forward_dev: edge features required"); return ASEP_ERR_ARG; }
    if (g->cfg.visual_edge_dims > 0) { set_error("asep_gnn_forward_dev: this graph assigns visual features to edges: use asep_gnn_forward_visual*"); return ASEP_ERR_ARG; }
    return forward_impl(g, g->pool, N, E, d_edges, d_node_feat, d_edge_feat, R, d_relations, d_probs_out, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_gnn_forward(asep_gnn* g, int N, int E, const int32_t* edges, const float* node_feat, const float* edge_feat,
                     int R, const int32_t* relations, float* probs_out) {
    ASEP_GUARD_BEGIN
    if (!g || !node_feat || (E > 0 && !edges) || (R > 0 && !probs_out)) { set_error("asep_gnn_forward: null argument"); return ASEP_ERR_ARG; }
    if (g->cfg.visual_edge_dims > 0) { set_error("asep_gnn_forward: this graph assigns visual features to edges: use asep_gnn_forward_visual*"); return ASEP_ERR_ARG; }
    if (N < 1 || E < 0 || R < 0) { set_error("asep_gnn_forward: bad sizes N=%d E=%d R=%d", N, E, R); return ASEP_ERR_ARG; }
    int rc;
    if (E > 0 && (rc = check_indices("interacting_nodes", edges, (size_t)E, N))) return rc;
    if (relations && R > 0 && (rc = check_indices("relations", relations, (size_t)R, N))) return rc;
    const size_t no = (size_t)R * g->cfg.num_classes;
    const StagedGraph st = stage_graph(g, (size_t)N, (size_t)E, (size_t)R, no, edges, node_feat, edge_feat, relations);
    rc = asep_gnn_forward_dev(g, N, E, st.e, st.u, st.f, R, st.r, st.o, nullptr);
    if (rc) return rc;
    if (R > 0) ASEP_HIP_CHECK(hipMemcpyAsync(probs_out, st.o, no * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    ASEP_HIP_CHECK(hipStreamSynchronize(nullptr));
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_gnn_correct_edges(asep_gnn* g, int N, int E, const int32_t* edges, const float* edge_feat, int32_t* out_edges,
                           float* out_feat) {
    ASEP_GUARD_BEGIN
    if (!g || N < 1 || E < 0 || (E > 0 && !edges) || !out_edges) { set_error("asep_gnn_correct_edges: bad argument"); return ASEP_ERR_ARG; }
    if ((size_t)N * N > (size_t)1 << 30) { set_error("asep_gnn_correct_edges: N too large"); return ASEP_ERR_UNSUPPORTED; }
    const int Ed = g->Ed;
    const bool feats = out_feat && Ed > 0 && edge_feat;
    g->host_stage.begin();
    int32_t* d_e = (int32_t*)g->host_stage.get(std::max<size_t>((size_t)E * 2, 1) * sizeof(int32_t));
    float* d_f = (float*)g->host_stage.get(std::max<size_t>(feats ? (size_t)E * Ed : 0, 1) * sizeof(float));
    float* d_of = (float*)g->host_stage.get(std::max<size_t>(feats ? (size_t)E * 2 * Ed : 0, 1) * sizeof(float));
    if (E > 0) ASEP_HIP_CHECK(hipMemcpy(d_e, edges, (size_t)E * 2 * sizeof(int32_t), hipMemcpyHostToDevice));
    if (feats && E > 0) ASEP_HIP_CHECK(hipMemcpy(d_f, edge_feat, (size_t)E * Ed * sizeof(float), hipMemcpyHostToDevice));
    g->pool.begin();
    EdgeBufs eb{};
    int rc = correct_edges_dev(g, g->pool, N, E, d_e, eb, nullptr);
    if (rc) return rc;
    int ecorr = 0;
    ASEP_HIP_CHECK(hipStreamSynchronize(nullptr));
    ASEP_HIP_CHECK(hipMemcpy(&ecorr, eb.rowptr + N, sizeof(int), hipMemcpyDeviceToHost));
    if (ecorr > 0) {
        ASEP_HIP_CHECK(hipMemcpy(out_edges, eb.sorted, (size_t)ecorr * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (feats) {
            hipLaunchKernelGGL(edge_feat_gather_kernel, dim3(std::min(cdiv(ecorr * Ed, 256), 1024)), dim3(256), 0, nullptr,
                               d_f, E, Ed, eb.sfirst, ecorr, d_of);
            ASEP_HIP_CHECK(hipMemcpy(out_feat, d_of, (size_t)ecorr * Ed * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return ecorr;
    ASEP_GUARD_END
}

int asep_gnn_get_hidden(asep_gnn* g, float* out, size_t max_floats) {
    ASEP_GUARD_BEGIN
    if (!g || !out || !g->d_h) { set_error("asep_gnn_get_hidden: no forward has run"); return ASEP_ERR_ARG; }
    const size_t n = (size_t)g->N * g->H;
    if (max_floats < n) { set_error("asep_gnn_get_hidden: buffer too small"); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipStreamSynchronize(g->stream));
    ASEP_HIP_CHECK(hipMemcpy(out, g->d_h, n * sizeof(float), hipMemcpyDeviceToHost));
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_gnn_step_mode(const asep_gnn* g) { return g ? step_mode_of(g) : ASEP_ERR_ARG; }

int asep_gnn_attach_backbone(asep_gnn* g, asep_aru* backbone, int n_maps, const char* const* endpoint_names) {
    return asep_gnn_attach_backbone_maps(g, backbone, n_maps, endpoint_names, nullptr);
}

int asep_gnn_attach_backbone_maps(asep_gnn* g, asep_aru* backbone, int n_maps, const char* const* endpoint_names, const int32_t* layer_depths) {
    ASEP_GUARD_BEGIN
    if (!g || !backbone || n_maps < 1 || !endpoint_names) { set_error("asep_gnn_attach_backbone: bad argument"); return ASEP_ERR_ARG; }
    g->free_visual();                                   // a second attach replaces (and frees) the first one's uploads
    struct Undo { asep_gnn* g; ~Undo() { if (g) g->free_visual(); } } undo{g};   // every refusal below frees what was uploaded so far
    std::string base;                                   // feature_map_generators.py:133,147: the last from_layer that had depth -1
    for (int i = 0; i < n_maps; ++i) {
        if (!endpoint_names[i]) { set_error("asep_gnn_attach_backbone: null end-point name"); return ASEP_ERR_ARG; }
        const int depth = layer_depths ? layer_depths[i] : -1;
        const bool named = endpoint_names[i][0] != 0;
        int C = named ? aru_endpoint_channels(backbone, endpoint_names[i]) : 0;
        if (named && (C < 1 || C > 256)) {
            set_error("asep_gnn_attach_backbone: '%s' is not a feature map of this backbone (only unet conv/deconv "
                      "end points are supported)", endpoint_names[i]);
            return ASEP_ERR_UNSUPPORTED;
        }
        asep_gnn::FmapGen G{};
        if (depth == -1) {
            if (!named) {
                set_error("asep_gnn_attach_backbone_maps: map %d has an empty from_layer and layer_depth -1: an empty from_layer builds a new map "
                          "and needs its depth (feature_map_generators.py:145-155)", i);
                return ASEP_ERR_ARG;
            }
            base = endpoint_names[i];
        } else {
            if (!named && i == 0) {
                set_error("asep_gnn_attach_backbone_maps: map 0 has an empty from_layer: there is no previous feature map to shrink "
                          "(feature_map_generators.py:154)");
                return ASEP_ERR_ARG;
            }
            if (depth < 2 || depth % 2 != 0 || depth > 256) {
                set_error("asep_gnn_attach_backbone_maps: map %d has layer_depth %d: an even depth from 2 to 256 is served (layer_depth / 2 is the "
                          "width of the 1x1 convolution, feature_map_generators.py:159-160)", i, depth);
                return depth > 256 ? ASEP_ERR_UNSUPPORTED : ASEP_ERR_ARG;
            }
            G.depth = depth;
            G.stride = named ? 1 : 2;
            G.Cin = named ? C : g->vis_C[i - 1];
            // the reference formats layer_depth / 2 as a Python float: "<d/2>.0" (feature_map_generators.py:159,164)
            const std::string n1 = base + "_1_Conv2d_" + std::to_string(i) + "_1x1_" + std::to_string(depth / 2) + ".0/";
            const std::string n2 = base + "_2_Conv2d_" + std::to_string(i) + "_3x3_s2_" + std::to_string(depth) + "/";
            int rc = upload_named(g->vis_owned, g->vis_blob, n1 + "weights", {1, 1, G.Cin, depth / 2}, &G.W1);
            if (!rc) rc = upload_named(g->vis_owned, g->vis_blob, n1 + "biases", {depth / 2}, &G.b1);
            if (!rc) rc = upload_named(g->vis_owned, g->vis_blob, n2 + "weights", {3, 3, depth / 2, depth}, &G.W2);
            if (!rc) rc = upload_named(g->vis_owned, g->vis_blob, n2 + "biases", {depth}, &G.b2);
            if (rc) { return rc; }
            C = depth;
            ++g->n_generated;
        }
        g->vis_gen.push_back(G);
        float *dW = nullptr, *db = nullptr; int d = 0;
        if (int rc = upload_compression(g, "visual_node_feature_compression_fm_" + std::to_string(i) + "/dense/", C, &dW, &db, &d)) { return rc; }
        g->vis_names.push_back(endpoint_names[i]);
        g->vis_W.push_back(dW); g->vis_b.push_back(db);
        g->vis_C.push_back(C); g->vis_d.push_back(d);
        g->vis_total += d;
    }
    if (g->cfg.visual_edge_dims > 0) {                     // assign_visual_features_to_edges: one compression layer per feature map
        for (int i = 0; i < n_maps; ++i) {
            float *dW = nullptr, *db = nullptr; int d = 0;
            if (int rc = upload_compression(g, "visual_edge_feature_compression_fm_" + std::to_string(i) + "/dense/", g->vis_C[i], &dW, &db, &d)) { return rc; }
            g->vise_W.push_back(dW); g->vise_b.push_back(db); g->vise_d.push_back(d);
            g->vise_total += d;
        }
        if (g->vise_total != g->cfg.visual_edge_dims) {
            set_error("asep_gnn_attach_backbone: the visual edge compression layers are %d wide in all, cfg.visual_edge_dims says %d", g->vise_total,
                      g->cfg.visual_edge_dims);
            return ASEP_ERR_ARG;
        }
    }
    if (g->vis_total >= g->Uin + 1) {
        set_error("asep_gnn_attach_backbone: %d visual dims exceed the fed node feature width %d", g->vis_total, g->Uin);
        return ASEP_ERR_ARG;
    }
    undo.g = nullptr;
    g->backbone = backbone;
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_gnn_get_feature_map(asep_gnn* g, int index, float* out, size_t max_floats, int32_t dims[3]) {
    ASEP_GUARD_BEGIN
    if (!g || !g->backbone || !dims || index < 0 || index >= (int)g->vis_names.size()) { set_error("asep_gnn_get_feature_map: bad argument"); return ASEP_ERR_ARG; }
    asep_gnn::FmapRef m{};
    // the maps of the page the last forward served last (a batch: its last page)
    int rc = visual_map_dev(g, g->n_generated ? g->fmap_last_prefix : std::string(), (size_t)index, &m);
    if (rc) return rc;
    return copy_map_out(g, "asep_gnn_get_feature_map", m, out, max_floats, dims);
    ASEP_GUARD_END
}

int asep_gnn_forward_visual_dev(asep_gnn* g, int N, int E, const int32_t* d_edges, const float* d_node_feat,
                                const float* d_edge_feat, const float* d_image, int h, int w, const float* d_regions, int P,
                                const int32_t* d_num_points, const float* d_edge_regions, const int32_t* d_edge_num_points,
                                int R, const int32_t* d_relations, float* d_probs_out, void* stream) {
    ASEP_GUARD_BEGIN
    const asep_gnn_page q{N, E, R, d_edges, d_node_feat, d_edge_feat, d_image, d_regions, d_num_points, d_edge_regions, d_edge_num_points,
                          d_relations, d_probs_out};
    return visual_uniform_impl(g, "asep_gnn_forward_visual_dev", 1, &q, h, w, P, (hipStream_t)stream, /*name_pages=*/false);
    ASEP_GUARD_END
}

int asep_gnn_forward_visual_batch_dev(asep_gnn* g, int n_pages, const asep_gnn_page* pages, int h, int w, int P, void* stream) {
    ASEP_GUARD_BEGIN
    return visual_uniform_impl(g, "asep_gnn_forward_visual_batch_dev", n_pages, pages, h, w, P, (hipStream_t)stream, /*name_pages=*/true);
    ASEP_GUARD_END
}

}  // extern "C"

namespace {

// one blob of tables, built on the host and copied once: add() returns the offset of a 16-byte aligned section
struct TableBlob {
    std::vector<char> bytes;
    template <class T>
    size_t add(const T* src, size_t n) {
        const size_t off = (bytes.size() + 15) & ~(size_t)15;
        bytes.resize(off + n * sizeof(T));
        if (n) memcpy(bytes.data() + off, src, n * sizeof(T));
        return off;
    }
};

// the blob into the next slot of the handle's ring, copied on s; returns the slot: its device address, and its event, which the caller records
// behind the last launch that reads the table (tables_read)
int put_tables(asep_gnn* g, const TableBlob& blob, hipStream_t s, asep_gnn::TableSlot** slot) {
    asep_gnn::TableSlot& t = g->tab_ring[g->tab_next++ % 8];
    if (!t.done) ASEP_HIP_CHECK(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
    else ASEP_HIP_CHECK(hipEventSynchronize(t.done));              // (the readers of four calls back: long done unless the caller runs that far ahead)
    const size_t need = std::max<size_t>(blob.bytes.size(), 16);
    if (t.cap < need) {
        const size_t cap = std::max(need, 2 * t.cap);
        if (t.h) (void)hipHostFree(t.h);
        if (t.d) (void)hipFree(t.d);
        t.h = nullptr; t.d = nullptr; t.cap = 0;
        ASEP_HIP_CHECK(hipHostMalloc((void**)&t.h, cap, hipHostMallocDefault));
        ASEP_HIP_CHECK(hipMalloc((void**)&t.d, cap));
        t.cap = cap;
    }
    if (!blob.bytes.empty()) memcpy(t.h, blob.bytes.data(), blob.bytes.size());
    ASEP_HIP_CHECK(hipMemcpyAsync(t.d, t.h, need, hipMemcpyHostToDevice, s));
    ASEP_HIP_CHECK(hipEventRecord(t.done, s));                     // (at least the copy; tables_read moves it behind the readers)
    *slot = &t;
    return ASEP_OK;
}
int tables_read(asep_gnn::TableSlot* t, hipStream_t s) {
    ASEP_HIP_CHECK(hipEventRecord(t->done, s));
    return ASEP_OK;
}

struct ScanIn { const uint8_t* d_scan; int H, W, C; };

// ---- the table schedule (asep_gnn_forward_visual_batch_dev2 / _u8_dev) as stages.  Each stage below reads and fills the call's plan: the
//      page list, the sizes and the addresses carved so far.  visual_batch2_impl runs them in order and stops at the first that fails ----
struct GenMap { int page; size_t map; const float* src; float* mid; };   // a generated (page, map) pair: the end point its 1x1 reads (if it reads one), the 1x1's output
struct FmapLaunch { size_t pages1 = 0, begin1 = 0, pages3 = 0, begin3 = 0; int grid1 = 0, grid3 = 0; bool bf = false; double fl1 = 0, by1 = 0, fl3 = 0, by3 = 0; };
struct RoiLaunch { std::vector<RoiArgs> e; std::vector<size_t> rows; size_t eoff = 0, boff = 0; int grid = 0; };
struct TablePlan {
    // the call: scans = the u8 entry's, or nullptr (then table_arenas fills in the pages' d_image)
    const char* fn; int n_pages; std::vector<asep_gnn_page>& pages; const ScanIn* scans; const int32_t *h, *w; int P; hipStream_t s;
    int ncls = 1, chans = 1; size_t n_maps = 0, nu = 0, nef = 0; std::vector<size_t> logit_items;                          // table_checks
    bool mvn = false; std::vector<size_t> img_items, mom_items, mom_off; double* d_mom = nullptr;                        // table_arenas
    std::vector<const float*> imgs; std::vector<float*> outs;
    std::vector<asep_gnn::PageRec> recs; std::vector<std::vector<FmapStep>> plans;                                       // table_map_plan
    std::vector<GenMap> gen;                                                                                             // (page by page, a page's maps in order)
    TableBlob blob; std::vector<FmapLaunch> fl; RoiLaunch roi[2];               // table_build_fmaps, table_build_rois; roi[0] fp32 maps, [1] bf16 maps
};

int table_checks(const asep_gnn* g, TablePlan& p) {
    const char* fn = p.fn;
    if (p.P < 1) { set_error("%s: P = %d region points", fn, p.P); return ASEP_ERR_ARG; }
    p.ncls = std::max(1, aru_num_classes(g->backbone));
    p.chans = std::max(1, aru_input_channels(g->backbone));
    p.n_maps = g->vis_names.size();
    p.logit_items.resize(p.n_pages);
    for (int b = 0; b < p.n_pages; ++b) {
        const asep_gnn_page& q = p.pages[b];
        const int h = p.h[b], w = p.w[b];
        if (h < 1 || w < 1) { set_error("%s: page %d has the size %d x %d, both sides must be positive", fn, b, h, w); return ASEP_ERR_ARG; }
        if (p.scans) {
            const ScanIn& sc = p.scans[b];
            if (!sc.d_scan || sc.H < 1 || sc.W < 1 || (size_t)sc.H * sc.W > 0x7fffffffull || (size_t)h * w > 0x7fffffffull) {
                set_error("%s: page %d: the scan is NULL or its size %d x %d (target %d x %d) is not served", fn, b, sc.H, sc.W, h, w);
                return ASEP_ERR_ARG;
            }
            if (!(sc.C == p.chans || (sc.C == 3 && p.chans == 1))) {   // 3 -> 1 is Pillow's luma per tap; 1 -> 3 has no meaning
                set_error("%s: page %d: the scan has %d image channel(s), the backbone takes %d", fn, b, sc.C, p.chans);
                return ASEP_ERR_ARG;
            }
        }
        if (int rc = check_visual_page(g, fn, b, q, !p.scans)) return rc;
        if ((size_t)q.N * q.N > (size_t)1 << 30) { set_error("%s: page %d: N=%d too large for the dense edge table", fn, b, q.N); return ASEP_ERR_UNSUPPORTED; }
        p.logit_items[b] = (size_t)h * w * p.ncls;
        p.nu += (size_t)q.N * g->Uin;
        if (g->vise_total > 0) p.nef += (size_t)q.E * g->Ed;
    }
    return ASEP_OK;
}

// arenas: ONE buffer each for the pages' logits, node features, edge features and generated maps, carved per page.  Each keeps the largest
// sum it has served, so a call whose page mix changes allocates only when its sum is a new maximum
int table_arenas(asep_gnn* g, TablePlan& p) {
    const int n = p.n_pages;
    std::vector<size_t> off, img_off;
    const size_t logit_total = arena_offsets(p.logit_items.data(), n, 64, off);
    g->vis_pool.begin();
    float* d_logits = (float*)g->vis_pool.get(logit_total * sizeof(float));
    // (the same three requests in the same order whatever the call needs, so that a buffer keeps its role from call to call)
    p.mvn = aru_mvn(g->backbone);
    p.img_items.resize(n); p.mom_items.resize(n);
    for (int b = 0; b < n; ++b) {
        p.img_items[b] = (size_t)p.h[b] * p.w[b] * p.chans;
        p.mom_items[b] = 2 * (size_t)moments_parts(p.img_items[b]) + 2;      // doubles: the partial pairs, then room for {mean, 1 / sd}
    }
    const size_t img_total = p.scans ? arena_offsets(p.img_items.data(), n, 64, img_off) : 0;
    const size_t mom_total = p.mvn ? arena_offsets(p.mom_items.data(), n, 2, p.mom_off) : 0;
    float* d_images = (float*)g->vis_pool.get(img_total * sizeof(float));
    p.d_mom = (double*)g->vis_pool.get(mom_total * sizeof(double));
    g->batch_images.clear();
    if (p.scans)
        for (int b = 0; b < n; ++b) {
            p.pages[b].d_image = d_images + img_off[b];
            g->batch_images.push_back(asep_gnn::FmapRef{p.pages[b].d_image, p.h[b], p.w[b], p.chans, 0});
        }
    p.imgs.resize(n); p.outs.resize(n);
    for (int b = 0; b < n; ++b) { p.imgs[b] = p.pages[b].d_image; p.outs[b] = d_logits + off[b]; }
    int rc = reserve_floats(&g->d_u_cat, &g->u_cat_cap, p.nu);
    if (!rc && p.nef) rc = reserve_floats(&g->d_ef_cat, &g->ef_cat_cap, p.nef);
    return rc;
}

// in front of the backbone: the scans' resize and the pages' moments, one launch per call each, over one table; then the grouped backbone forward
int table_backbone(asep_gnn* g, TablePlan& p) {
    const int n = p.n_pages; hipStream_t s = p.s;
    g->stream = s;
    aru_prof_stream(g->backbone, s);
    std::vector<const float*> stats(n, nullptr);
    int rc = ASEP_OK;
    if (p.scans || p.mvn) {
        TableBlob pre;
        size_t r_pages = 0, r_begin = 0, m_pages = 0, m_begin = 0;
        std::vector<int32_t> rb, mb;
        if (p.scans) {
            std::vector<ResizePage> rp(n);
            std::vector<size_t> px(n);
            for (int b = 0; b < n; ++b) {
                const ScanIn& sc = p.scans[b];
                rp[b] = resize_page(sc.d_scan, sc.H, sc.W, sc.C, sc.C != p.chans, p.h[b], p.w[b], const_cast<float*>(p.pages[b].d_image));
                px[b] = (size_t)p.h[b] * p.w[b];
            }
            if (!page_unit_table(px.data(), n, 256, rb)) { set_error("%s: the %d pages are too large for one resize launch", p.fn, n); return ASEP_ERR_UNSUPPORTED; }
            r_pages = pre.add(rp.data(), rp.size()); r_begin = pre.add(rb.data(), rb.size());
        }
        if (p.mvn) {
            std::vector<MomentsPage> mp(n);
            std::vector<size_t> parts(n);
            for (int b = 0; b < n; ++b) {
                double* base = p.d_mom + p.mom_off[b];
                mp[b] = MomentsPage{p.pages[b].d_image, p.img_items[b], base, (float*)(base + p.mom_items[b] - 2), moments_parts(p.img_items[b])};
                parts[b] = (size_t)mp[b].parts;
                stats[b] = mp[b].stats;
            }
            if (!page_unit_table(parts.data(), n, 1, mb)) { set_error("%s: too many pages for one moments launch", p.fn); return ASEP_ERR_UNSUPPORTED; }
            m_pages = pre.add(mp.data(), mp.size()); m_begin = pre.add(mb.data(), mb.size());
        }
        asep_gnn::TableSlot* slot = nullptr;
        if ((rc = put_tables(g, pre, s, &slot))) return rc;
        if (p.scans) {
            ProfiledLaunch pl(g, "prep_resize_tf1_pages_kernel", std::to_string(n) + " pages", 0.0, 0.0);
            rc = resize_tf1_pages_launch((const ResizePage*)(slot->d + r_pages), (const int32_t*)(slot->d + r_begin), n, rb[n], s);
        }
        if (rc) return rc;
        if (p.mvn && (rc = aru_moments_pages(g->backbone, (const MomentsPage*)(slot->d + m_pages), (const int32_t*)(slot->d + m_begin), n, mb[n], s))) return rc;
        if ((rc = tables_read(slot, s))) return rc;
    }
    if (p.mvn) aru_set_page_stats(g->backbone, stats.data());
    rc = asep_aru_forward_batch_dev2(g->backbone, n, p.imgs.data(), p.h, p.w, p.outs.data(), nullptr, nullptr, 0.f, s);
    aru_set_page_stats(g->backbone, nullptr);
    if (!rc) g->stream = s;
    return rc;
}

// every map of every page: the backbone's end points (known once the forward is queued), the generated ones in one arena
int table_map_plan(asep_gnn* g, TablePlan& p) {
    p.recs.resize(p.n_pages); p.plans.resize(p.n_pages);
    std::vector<size_t> arena_items;                                  // per generated (page, map): the 1x1's output, then the map itself
    for (int b = 0; b < p.n_pages; ++b) {
        std::vector<const float*> end_p;
        if (int rc = page_map_plan(g, page_prefix(b), p.plans[b], end_p)) return rc;
        p.recs[b].maps.resize(p.n_maps);
        for (size_t i = 0; i < p.n_maps; ++i) {
            const FmapStep& k = p.plans[b][i];
            p.recs[b].maps[i] = map_ref(k.generated ? nullptr : end_p[i], k.out);   // (a generated one's address follows below)
            if (!k.generated) continue;
            p.gen.push_back(GenMap{b, i, end_p[i], nullptr});
            arena_items.push_back(k.n1); arena_items.push_back(k.n2);
        }
    }
    if (g->n_generated) {
        std::vector<size_t> aoff;
        const size_t total = arena_offsets(arena_items.data(), (int)arena_items.size(), 64, aoff);
        g->fmap_pool.begin();
        float* base = (float*)g->fmap_pool.get(total * sizeof(float));
        for (size_t k = 0; k < p.gen.size(); ++k) {
            p.gen[k].mid = base + aoff[2 * k];
            p.recs[p.gen[k].page].maps[p.gen[k].map].p = base + aoff[2 * k + 1];
        }
    }
    return ASEP_OK;
}

// the tables of the generated maps: per map two (1x1, 3x3) over the pages
int table_build_fmaps(const asep_gnn* g, TablePlan& p) {
    const int n = p.n_pages;
    p.fl.resize(p.n_maps);
    for (size_t i = 0; i < p.n_maps; ++i) {
        if (g->vis_gen[i].depth < 0) continue;
        std::vector<FmapPage> p1(n), p3(n);
        std::vector<size_t> it1(n), it3(n);
        FmapLaunch& L = p.fl[i];
        L.bf = p.plans[0][i].in.bf != 0;
        for (const GenMap& m : p.gen) {                              // map i of every page, in page order
            if (m.map != i) continue;
            const int b = m.page;
            const FmapStep& k = p.plans[b][i];
            if ((k.in.bf != 0) != L.bf) { set_error("%s: end points of one call differ in precision", p.fn); return ASEP_ERR_ARG; }
            p1[b] = FmapPage{k.src < 0 ? m.src : p.recs[b].maps[k.src].p, m.mid, k.d.ih, k.d.iw, k.d.ih, k.d.iw, 0, 0};
            p3[b] = FmapPage{m.mid, const_cast<float*>(p.recs[b].maps[i].p), k.d.ih, k.d.iw, k.d.oh, k.d.ow, k.d.pad_t, k.d.pad_l};
            it1[b] = k.n1; it3[b] = k.n2;
            L.fl1 += k.fl1; L.by1 += k.io1; L.fl3 += k.fl3; L.by3 += k.io3;
        }
        L.by1 += p.plans[0][i].w1;                                    // (the filter and bias once per launch)
        L.by3 += p.plans[0][i].w3;
        std::vector<int32_t> b1, b3;
        if (!page_unit_table(it1.data(), n, 256, b1) || !page_unit_table(it3.data(), n, 256, b3)) {
            set_error("%s: feature map %zu of the %d pages is too large for one launch", p.fn, i, n);
            return ASEP_ERR_UNSUPPORTED;
        }
        L.grid1 = b1[n]; L.grid3 = b3[n];
        L.pages1 = p.blob.add(p1.data(), p1.size()); L.begin1 = p.blob.add(b1.data(), b1.size());
        L.pages3 = p.blob.add(p3.data(), p3.size()); L.begin3 = p.blob.add(b3.data(), b3.size());
    }
    return ASEP_OK;
}

// the regions' entries, fp32 maps and bf16 maps apart; the pages' rows of d_u_cat into the page records
int table_build_rois(asep_gnn* g, TablePlan& p) {
    const RoiSide nodes = node_side(g), edges = edge_side(g);
    size_t urow = 0, efrow = 0;
    for (int b = 0; b < p.n_pages; ++b) {
        const asep_gnn_page& q = p.pages[b];
        p.recs[b].N = q.N; p.recs[b].u_off = urow * g->Uin;
        int col = nodes.fed, ecol = edges.fed;
        for (size_t i = 0; i < p.n_maps; ++i) {
            const asep_gnn::FmapRef& m = p.recs[b].maps[i];
            RoiLaunch& L = p.roi[m.bf ? 1 : 0];
            L.e.push_back(roi_entry(m, q.d_regions, p.P, q.d_num_points, nodes, i, g->d_u_cat + urow * g->Uin, col));
            L.rows.push_back((size_t)q.N);
            col += g->vis_d[i];
            if (g->vise_total > 0 && q.E > 0) {
                L.e.push_back(roi_entry(m, q.d_edge_regions, p.P, q.d_edge_num_points, edges, i, g->d_ef_cat + efrow * g->Ed, ecol));
                L.rows.push_back((size_t)q.E);
                ecol += g->vise_d[i];
            }
        }
        urow += (size_t)q.N;
        if (g->vise_total > 0) efrow += (size_t)q.E;
    }
    for (RoiLaunch& L : p.roi) {
        if (L.e.empty()) continue;
        std::vector<int32_t> bg;
        if (!page_unit_table(L.rows.data(), (int)L.rows.size(), 1, bg)) { set_error("%s: too many regions for one launch", p.fn); return ASEP_ERR_UNSUPPORTED; }
        L.grid = bg.back();
        L.eoff = p.blob.add(L.e.data(), L.e.size());
        L.boff = p.blob.add(bg.data(), bg.size());
    }
    return ASEP_OK;
}

// the tables to the device, then one launch per stage over all pages
int table_launches(asep_gnn* g, const TablePlan& p) {
    const int n = p.n_pages; hipStream_t s = p.s;
    asep_gnn::TableSlot* slot = nullptr;
    if (int rc = put_tables(g, p.blob, s, &slot)) return rc;
    const char* tab = slot->d;
    for (size_t i = 0; i < p.n_maps; ++i) {
        const asep_gnn::FmapGen& G = g->vis_gen[i];
        if (G.depth < 0) continue;
        const FmapLaunch& L = p.fl[i];
        const std::string where = "fm_" + std::to_string(i) + " " + std::to_string(n) + " pages";
        FmapPagesArgs a{};
        a.pages = (const FmapPage*)(tab + L.pages1); a.begin = (const int32_t*)(tab + L.begin1); a.n_pages = n;
        a.W = G.W1; a.b = G.b1; a.Ci = G.Cin; a.Co = G.depth / 2; a.stride = 1;
        if (L.grid1 > 0) {
            ProfiledLaunch pl(g, L.bf ? "fmap_conv1x1_pages_kernel<true>" : "fmap_conv1x1_pages_kernel<false>", where + " " + std::to_string(G.Cin) + "->" + std::to_string(G.depth / 2), L.fl1, L.by1);
            if (L.bf) hipLaunchKernelGGL(fmap_conv1x1_pages_kernel<true>, dim3((unsigned)L.grid1), dim3(256), 0, s, a);
            else hipLaunchKernelGGL(fmap_conv1x1_pages_kernel<false>, dim3((unsigned)L.grid1), dim3(256), 0, s, a);
        }
        FmapPagesArgs c = a;
        c.pages = (const FmapPage*)(tab + L.pages3); c.begin = (const int32_t*)(tab + L.begin3);
        c.W = G.W2; c.b = G.b2; c.Ci = G.depth / 2; c.Co = G.depth; c.stride = G.stride;
        if (L.grid3 > 0) {
            ProfiledLaunch pl(g, "fmap_conv3x3_pages_kernel", where + " " + std::to_string(G.depth / 2) + "->" + std::to_string(G.depth) + " s" + std::to_string(G.stride), L.fl3, L.by3);
            hipLaunchKernelGGL(fmap_conv3x3_pages_kernel, dim3((unsigned)L.grid3), dim3(256), 0, s, c);
        }
    }
    for (int k = 0; k < 2; ++k) {
        const RoiLaunch& L = p.roi[k];
        if (L.grid < 1) continue;
        RoiPagesArgs a{(const RoiArgs*)(tab + L.eoff), (const int32_t*)(tab + L.boff), (int)L.e.size()};
        ProfiledLaunch pl(g, k ? "gnn_roi_compress_pages_kernel<true>" : "gnn_roi_compress_pages_kernel<false>",
                          std::to_string(n) + " pages " + std::to_string(L.e.size()) + " entries " + std::to_string(L.grid) + " regions", 0.0, 0.0);
        if (k) hipLaunchKernelGGL(gnn_roi_compress_pages_kernel<true>, dim3((unsigned)L.grid), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(gnn_roi_compress_pages_kernel<false>, dim3((unsigned)L.grid), dim3(256), 0, s, a);
    }
    ASEP_HIP_CHECK(hipGetLastError());
    return tables_read(slot, s);
}

// the graphs, page by page (they batch nothing across pages today: N, E and R differ); then what the read-backs serve
int table_graphs(asep_gnn* g, TablePlan& p) {
    const RoiSide nodes = node_side(g), edges = edge_side(g);
    float *d_u = g->d_u_cat, *d_efc = g->d_ef_cat;
    for (int b = 0; b < p.n_pages; ++b) {
        const asep_gnn_page& q = p.pages[b];
        copy_fed_cols(nodes, q.N, q.d_node_feat, d_u, p.s);
        if (g->vise_total > 0 && q.E > 0) copy_fed_cols(edges, q.E, q.d_edge_feat, d_efc, p.s);
        if (int rc = visual_graph_dev(g, q, &d_u, &d_efc, p.s)) return rc;
    }
    g->fmap_last = p.recs[p.n_pages - 1].maps;                      // as after the uniform entry: the last page's maps
    g->fmap_last_prefix = page_prefix(p.n_pages - 1);
    g->batch_pages = std::move(p.recs);
    g->batch_serial = g->fwd_serial;
    return ASEP_OK;
}

int visual_batch2_impl(asep_gnn* g, TablePlan&& p) {
    int rc = table_checks(g, p);
    if (!rc) rc = table_arenas(g, p);
    if (!rc) rc = table_backbone(g, p);
    if (!rc) rc = table_map_plan(g, p);
    if (!rc) rc = table_build_fmaps(g, p);
    if (!rc) rc = table_build_rois(g, p);
    if (!rc) rc = table_launches(g, p);
    if (!rc) rc = table_graphs(g, p);
    return rc;
}

// what the two entries check before they copy their page lists
int batch2_head_checks(asep_gnn* g, const char* fn, int n_pages, const void* pages, const int32_t* h, const int32_t* w) {
    if (!g || !g->backbone) { set_error("%s: no backbone attached", fn); return ASEP_ERR_ARG; }
    if (n_pages < 1) { set_error("%s: n_pages = %d, at least one page is needed", fn, n_pages); return ASEP_ERR_ARG; }
    if (!pages) { set_error("%s: pages is NULL", fn); return ASEP_ERR_ARG; }
    if (!h || !w) { set_error("%s: the size array %s is NULL (page 0 and every other page need h[b] x w[b])", fn, !h ? "h" : "w"); return ASEP_ERR_ARG; }
    return ASEP_OK;
}

// page `page` of the handle's last call over a page table, or nullptr with the error set
const asep_gnn::PageRec* batch_page(asep_gnn* g, const char* fn, int page) {
    if (!g || g->batch_serial != g->fwd_serial || g->batch_pages.empty()) { set_error("%s: the handle's last forward was not a call over a page table (asep_gnn_forward_visual_batch_dev2 / _u8_dev)", fn); return nullptr; }
    if (page < 0 || page >= (int)g->batch_pages.size()) { set_error("%s: page %d of a call of %zu pages", fn, page, g->batch_pages.size()); return nullptr; }
    return &g->batch_pages[page];
}

}  // namespace

extern "C" {

// ABI 9: asep_gnn_forward_visual_batch_dev for pages of DIFFERENT image sizes.  One launch per call, over a page table in device memory, for:
// the resize of uint8 scans (the u8 entry), the per-image moments of the backbone's standardisation, the two convolutions of each generated
// map, ROI max + compression of all node and interaction regions.  The backbones run as one grouped forward over the page list
// (asep_aru_forward_batch_dev2's launches), the graphs page by page as before.  The kernels' bodies are the single-page ones.
int asep_gnn_forward_visual_batch_dev2(asep_gnn* g, int n_pages, const asep_gnn_page* pages, const int32_t* h, const int32_t* w, int P, void* stream) {
    ASEP_GUARD_BEGIN
    const char* fn = "asep_gnn_forward_visual_batch_dev2";
    if (int rc = batch2_head_checks(g, fn, n_pages, pages, h, w)) return rc;
    std::vector<asep_gnn_page> pg(pages, pages + n_pages);
    return visual_batch2_impl(g, TablePlan{fn, n_pages, pg, nullptr, h, w, P, (hipStream_t)stream});
    ASEP_GUARD_END
}

int asep_gnn_forward_visual_batch_u8_dev(asep_gnn* g, int n_pages, const asep_gnn_page_u8* pages, const int32_t* h, const int32_t* w, int P, void* stream) {
    ASEP_GUARD_BEGIN
    const char* fn = "asep_gnn_forward_visual_batch_u8_dev";
    if (int rc = batch2_head_checks(g, fn, n_pages, pages, h, w)) return rc;
    std::vector<asep_gnn_page> pg(n_pages);
    std::vector<ScanIn> scans(n_pages);
    for (int b = 0; b < n_pages; ++b) {
        pg[b] = pages[b].page;
        scans[b] = ScanIn{pages[b].d_scan, pages[b].src_h, pages[b].src_w, pages[b].src_c};
    }
    return visual_batch2_impl(g, TablePlan{fn, n_pages, pg, scans.data(), h, w, P, (hipStream_t)stream});
    ASEP_GUARD_END
}

int asep_gnn_get_page_node_features(asep_gnn* g, int page, float* out, size_t max_floats) {
    ASEP_GUARD_BEGIN
    const asep_gnn::PageRec* r = batch_page(g, "asep_gnn_get_page_node_features", page);
    if (!r) return ASEP_ERR_ARG;
    if (!out) { set_error("asep_gnn_get_page_node_features: out is NULL"); return ASEP_ERR_ARG; }
    return copy_node_features_out(g, "asep_gnn_get_page_node_features", r->u_off, r->N, out, max_floats);
    ASEP_GUARD_END
}

int asep_gnn_get_page_feature_map(asep_gnn* g, int page, int index, float* out, size_t max_floats, int32_t dims[3]) {
    ASEP_GUARD_BEGIN
    const asep_gnn::PageRec* r = batch_page(g, "asep_gnn_get_page_feature_map", page);
    if (!r) return ASEP_ERR_ARG;
    if (!dims || index < 0 || index >= (int)r->maps.size()) { set_error("asep_gnn_get_page_feature_map: bad argument"); return ASEP_ERR_ARG; }
    return copy_map_out(g, "asep_gnn_get_page_feature_map", r->maps[index], out, max_floats, dims);
    ASEP_GUARD_END
}

int asep_gnn_get_page_image(asep_gnn* g, int page, float* out, size_t max_floats, int32_t dims[3]) {
    ASEP_GUARD_BEGIN
    const asep_gnn::PageRec* r = batch_page(g, "asep_gnn_get_page_image", page);
    if (!r) return ASEP_ERR_ARG;
    if (!dims || g->batch_images.size() != g->batch_pages.size()) { set_error("asep_gnn_get_page_image: the last call was not fed uint8 scans"); return ASEP_ERR_ARG; }
    return copy_map_out(g, "asep_gnn_get_page_image", g->batch_images[page], out, max_floats, dims);
    ASEP_GUARD_END
}

int asep_gnn_forward_visual(asep_gnn* g, int N, int E, const int32_t* edges, const float* node_feat, const float* edge_feat,
                            const float* image, int h, int w, const float* regions, int P, const int32_t* num_points,
                            const float* edge_regions, const int32_t* edge_num_points, int R, const int32_t* relations, float* probs_out) {
    ASEP_GUARD_BEGIN
    if (!g || !g->backbone) { set_error("asep_gnn_forward_visual: no backbone attached"); return ASEP_ERR_ARG; }
    const int U = g->Uin, ug = U - g->vis_total;
    if (N < 1 || E < 0 || R < 0 || h < 1 || w < 1 || P < 1 || !image || !regions || !num_points || (ug > 0 && !node_feat) ||
        (E > 0 && !edges) || (R > 0 && !probs_out)) { set_error("asep_gnn_forward_visual: bad argument"); return ASEP_ERR_ARG; }
    int rc;
    if (E > 0 && (rc = check_indices("interacting_nodes", edges, (size_t)E, N))) return rc;
    if (relations && R > 0 && (rc = check_indices("relations", relations, (size_t)R, N))) return rc;
    const size_t ne = (size_t)E * 2, nug = (size_t)N * ug, nf = edge_feat ? (size_t)E * g->Ed_fed : 0;
    const bool vedges = g->vise_total > 0 && E > 0;
    if (vedges && (!edge_regions || !edge_num_points)) { set_error("asep_gnn_forward_visual: this graph assigns visual features to edges: edge_regions / edge_num_points required"); return ASEP_ERR_ARG; }
    const size_t nr = relations ? (size_t)R * 2 : 0, no = (size_t)R * g->cfg.num_classes;
    const size_t ni = (size_t)h * w * std::max(1, aru_input_channels(g->backbone));   // [h,w,C], C the attached backbone's
    const size_t nreg = (size_t)N * 2 * P;
    auto up = [&](const void* src, size_t bytes) -> void* {          // grow-only staging + async copy on the null stream
        void* d = g->host_stage.get(std::max<size_t>(bytes, 4));
        if (bytes && src) ASEP_HIP_CHECK_THROW(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, nullptr));
        return d;
    };
    g->host_stage.begin();
    int32_t* d_e = (int32_t*)up(edges, ne * 4);
    float* d_ug = (float*)up(node_feat, nug * 4);
    float* d_f = (float*)up(edge_feat, nf * 4);
    int32_t* d_r = (int32_t*)up(relations, nr * 4);
    float* d_img = (float*)up(image, ni * 4);
    float* d_reg = (float*)up(regions, nreg * 4);
    int32_t* d_np = (int32_t*)up(num_points, (size_t)N * 4);
    float* d_ereg = (float*)up(vedges ? edge_regions : nullptr, vedges ? (size_t)E * 2 * P * 4 : 0);
    int32_t* d_enp = (int32_t*)up(vedges ? edge_num_points : nullptr, vedges ? (size_t)E * 4 : 0);
    float* d_o = (float*)up(nullptr, no * 4);
    rc = asep_gnn_forward_visual_dev(g, N, E, ne ? d_e : nullptr, nug ? d_ug : nullptr, nf ? d_f : nullptr, d_img, h, w, d_reg,
                                     P, d_np, vedges ? d_ereg : nullptr, vedges ? d_enp : nullptr, R, nr ? d_r : nullptr, d_o, nullptr);
    if (rc) return rc;
    if (R > 0) ASEP_HIP_CHECK(hipMemcpyAsync(probs_out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    ASEP_HIP_CHECK(hipStreamSynchronize(nullptr));
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_gnn_get_node_features(asep_gnn* g, float* out, size_t max_floats) {
    ASEP_GUARD_BEGIN
    if (!g || !out || !g->d_u_cat) { set_error("asep_gnn_get_node_features: no visual forward has run"); return ASEP_ERR_ARG; }
    return copy_node_features_out(g, "asep_gnn_get_node_features", 0, g->N, out, max_floats);
    ASEP_GUARD_END
}

double asep_gnn_flops(const asep_gnn* g, int N, int E_corrected, int R) {
    if (!g) return 0.0;
    const asep_gnn_cfg& c = g->cfg;
    auto mlp_mac = [](const MlpW& m) {
        double s = 0;
        for (int l = 0; l < m.nl; ++l) s += (double)m.dims[l] * m.dims[l + 1];
        return s;
    };
    double per_edge = 0;
    if (c.attention_heads > 0)
        for (int k = 0; k < c.attention_heads; ++k) per_edge += mlp_mac(g->att_w[k].inter) + mlp_mac(g->att_w[k].att);
    else per_edge = mlp_mac(g->msg);
    double mac = (double)c.num_transition_steps * ((double)E_corrected * per_edge + (double)N * 4.0 * g->V * g->H);
    mac += (double)R * ((double)2 * g->H * c.cls_hidden1 + mlp_mac(g->cls_rest));
    return 2.0 * mac;
}

}  // extern "C"

// ---- ABI 12: the graph part of the relation net for the pages of ONE call (gnn_batch_kernels.h) -----------------------------------------------
// asep_gnn_forward_batch[_dev]: edge correction, T x (message, aggregation / attention soft-max, LSTM update) and the pair classifier each as one
// launch over all pages.  The correction, the attention pairing's chunk ranks and the classifier go through the page table; every stage between
// them is the single-page kernel over the nodes of the call (one CSR-by-target over all pages): graph_steps above, which forward_impl runs too.
namespace {

const char* table_error_text(GnnTableError e) {
    switch (e) {
        case GNN_TABLE_BAD_N: return "N < 1";
        case GNN_TABLE_BAD_E: return "E < 0";
        case GNN_TABLE_BAD_R: return "R < 0";
        case GNN_TABLE_PAGE_TOO_LARGE: return "N too large for the dense edge table (N^2 > 2^30)";
        case GNN_TABLE_SUM_TABLES: return "the edge tables of the pages up to this one do not fit one allocation (sum of N^2 > 2^30): split the call";
        case GNN_TABLE_SUM_INDEX: return "the nodes, edges or relations of the pages up to this one do not fit a 31-bit index: split the call";
        default: return "";
    }
}

// every check of a batched graph call that needs no device: the handle, the arrays, the page sizes and sums, the output buffer
int batch_graph_checks(asep_gnn* g, const char* fn, int n_pages, const int32_t* N, const int32_t* E, const int32_t* R, const void* node_feat,
                       const void* edges, const void* edge_feat, const void* probs_out, size_t max_floats, GnnPageTable& tab, GnnUnitTables& units) {
    if (!g) { set_error("%s: null handle", fn); return ASEP_ERR_ARG; }
    g->batch_launches = 0;
    if (g->backbone || g->vis_total > 0 || g->cfg.visual_edge_dims > 0) {
        set_error("%s: this graph has visual %s features: its pages go through asep_gnn_forward_visual_batch_dev2", fn,
                  g->cfg.visual_edge_dims > 0 ? "edge" : "node");
        return ASEP_ERR_ARG;
    }
    if (n_pages < 1) { set_error("%s: n_pages = %d, at least one page is needed", fn, n_pages); return ASEP_ERR_ARG; }
    if (!N || !E || !R) { set_error("%s: the size array %s is NULL", fn, !N ? "N" : (!E ? "E" : "R")); return ASEP_ERR_ARG; }
    if (!node_feat) { set_error("%s: node_feat is NULL", fn); return ASEP_ERR_ARG; }
    if (g->cfg.num_classes < 2) { set_error("%s: the output is the class-1 probability, this model has %d class", fn, g->cfg.num_classes); return ASEP_ERR_ARG; }
    const asep_gnn_cfg& c = g->cfg;
    const int width = std::max({g->Uin, g->U, g->Upad, 64, g->H, g->H + g->Uin, g->I, g->Iout, std::max(c.attention_heads, 1) * std::max(g->att_xd, 1),
                                (int)c.cls_hidden1, (int)c.num_classes});
    int bad = -1;
    const GnnTableError te = gnn_page_table(N, E, R, n_pages, c.undirected_graph != 0, width, tab, &bad);
    if (te != GNN_TABLE_OK) {
        set_error("%s: %s in page %d (N=%d E=%d R=%d)", fn, table_error_text(te), bad, N[bad], E[bad], R[bad]);
        return te == GNN_TABLE_BAD_N || te == GNN_TABLE_BAD_E || te == GNN_TABLE_BAD_R ? ASEP_ERR_ARG : ASEP_ERR_UNSUPPORTED;
    }
    if (tab.edges > 0 && !edges) {
        const int b = (int)(std::find_if(E, E + n_pages, [](int32_t e) { return e > 0; }) - E);
        set_error("%s: edges is NULL, E = %d in page %d", fn, E[b], b);
        return ASEP_ERR_ARG;
    }
    if (tab.edges > 0 && c.edge_feature_dim > 0 && !edge_feat) { set_error("%s: edge features required", fn); return ASEP_ERR_ARG; }
    if (tab.rels > 0 && !probs_out) { set_error("%s: probs_out is NULL", fn); return ASEP_ERR_ARG; }
    if (max_floats < tab.rels) {
        set_error("%s: the output buffer holds %zu floats, the %d pages have %llu relations", fn, max_floats, n_pages, (unsigned long long)tab.rels);
        return ASEP_ERR_ARG;
    }
    if (!gnn_unit_tables(tab, c.undirected_graph != 0, c.cls_hidden1, g->cls_fast ? 256 : PAIRG_P, units)) {
        set_error("%s: the blocks of the %d pages do not fit one launch: split the call", fn, n_pages);
        return ASEP_ERR_UNSUPPORTED;
    }
    return ASEP_OK;
}

int forward_batch_impl(asep_gnn* g, const GnnPageTable& tab, const GnnUnitTables& units, const int32_t* d_edges, const float* d_u,
                       const float* d_ef, const int32_t* d_rel, float* d_out, hipStream_t s) {
    const asep_gnn_cfg& c = g->cfg;
    const int n = (int)tab.rows.size();
    const int NN = (int)tab.nodes, EE = (int)tab.edges, RR = (int)tab.rels;
    const int und = c.undirected_graph ? 1 : 0;
    BufferPool& pool = g->batch_pool;
    long& nl = g->batch_launches;                            // (0 since batch_graph_checks)
    g->stream = s;
    g->N = NN;
    ++g->fwd_serial;
    pool.begin();
    // the page table and the launches' unit tables: one blob, one copy
    TableBlob blob;
    const size_t o_rows = blob.add(tab.rows.data(), tab.rows.size());
    const size_t o_node = blob.add(tab.node_begin.data(), tab.node_begin.size());
    const size_t o_fill = blob.add(units.fill.data(), units.fill.size());
    const size_t o_chunk = blob.add(units.chunk.data(), units.chunk.size());
    const size_t o_pre = blob.add(units.pre.data(), units.pre.size());
    const size_t o_cls = blob.add(units.cls.data(), units.cls.size());
    asep_gnn::TableSlot* slot = nullptr;
    if (int rc = put_tables(g, blob, s, &slot)) return rc;
    auto pages = [&](size_t off) { return GnnPagesArgs{(const GnnPageRow*)(slot->d + o_rows), (const int32_t*)(slot->d + off), n}; };

    // ---- edge correction (misc.py:7-151), every page's own table ----
    EdgeBufs eb{};
    if (int rc = edge_bufs(pool, (size_t)tab.cells, (size_t)NN, (size_t)tab.max_corrected, eb, s)) return rc;
    if (units.fill[n] > 0) COUNTED_LAUNCH(nl, edge_table_pages_kernel, dim3(units.fill[n]), dim3(256), 0, s, pages(o_fill), d_edges, und, eb.table);
    COUNTED_LAUNCH(nl, edge_count_pages_kernel, dim3(NN), dim3(64), 0, s, pages(o_node), eb.table, eb.rowcnt, eb.colcnt);
    COUNTED_LAUNCH(nl, edge_scan_kernel, dim3(1), dim3(1024), 0, s, eb.rowcnt, eb.colcnt, NN, eb.rowptr, eb.colptr);   // (integer sums: one scan over the call)
    COUNTED_LAUNCH(nl, edge_emit_pages_kernel, dim3(NN), dim3(64), 0, s, pages(o_node), eb.table, eb.rowptr, eb.colptr, eb.sorted, eb.sfirst, eb.tsrc, eb.tfirst);
    g->d_rowptr = eb.rowptr;
    g->gb_sorted = eb.sorted; g->gb_sfirst = eb.sfirst; g->gb_rowptr = eb.rowptr;

    // ---- the steps over the nodes of the call; tfirst holds rows of the call's edge features ----
    GraphOut go;
    auto chunk_rank = [&](int* widx, long& count) {
        COUNTED_LAUNCH(count, edge_chunk_rank_pages_kernel, dim3(units.chunk[n]), dim3(256), 0, s, pages(o_chunk), eb.sorted, eb.rowptr, eb.colptr, widx);
    };
    if (int rc = graph_steps(g, pool, NN, std::max(EE, 1), (size_t)tab.max_corrected, eb, d_u, d_ef, s, chunk_rank, go)) return rc;
    nl += go.launches;

    // ---- the pair classifier, every page's own relations ----
    float* Pt = (float*)pool.get((size_t)NN * c.cls_hidden1 * 4);
    float* Qt = (float*)pool.get((size_t)NN * c.cls_hidden1 * 4);
    float* probs = (float*)pool.get((size_t)std::max(RR, 1) * c.num_classes * 4);
    if (RR > 0) {
        COUNTED_LAUNCH(nl, gnn_pair_pre_pages_kernel, dim3(units.pre[n]), dim3(256), 0, s, pages(o_pre), go.hcls, go.Hc, g->C1, c.cls_hidden1, Pt, Qt);
        PairArgs pa{};
        PairGenArgs pg{};
        pair_args(g, Pt, Qt, d_rel, probs, pa, pg);
        if (g->cls_fast)
            COUNTED_LAUNCH(nl, (gnn_pair_cls_pages_kernel<64, 32, 2>), dim3(units.cls[n]), dim3(256), 0, s, pages(o_cls), pa);
        else
            COUNTED_LAUNCH(nl, gnn_pair_cls_generic_pages_kernel, dim3(units.cls[n]), dim3(256), 2 * (size_t)PAIRG_P * g->cls_maxw * sizeof(float), s,
                           pages(o_cls), pg);
        COUNTED_LAUNCH(nl, gnn_take_class_kernel, dim3(cdiv(RR, 256)), dim3(256), 0, s, probs, RR, c.num_classes, 1, d_out);
    }
    if (int rc = tables_read(slot, s)) return rc;
    ASEP_HIP_CHECK(hipGetLastError());
    g->graph_pages = tab.rows;
    g->graph_serial = g->fwd_serial;
    return ASEP_OK;
}

// "names a node outside" per page, as check_indices says it for one page
int check_page_indices(const char* fn, const char* what, const int32_t* idx, const GnnPageTable& tab, bool relations) {
    for (size_t b = 0; b < tab.rows.size(); ++b) {
        const GnnPageRow& r = tab.rows[b];
        const int32_t* p = idx + 2 * (size_t)(relations ? r.rel_off : r.edge_off);
        const size_t cnt = (size_t)(relations ? r.R : r.E);
        for (size_t i = 0; i < 2 * cnt; ++i)
            if (p[i] < 0 || p[i] >= r.N) {
                set_error("%s: %s[%zu] = (%d, %d) names a node outside 0..%d in page %d", fn, what, i / 2, p[i & ~(size_t)1], p[i | 1], r.N - 1, (int)b);
                return ASEP_ERR_ARG;
            }
    }
    return ASEP_OK;
}

const GnnPageRow* graph_batch_page(asep_gnn* g, const char* fn, int page) {
    if (!g || g->graph_serial != g->fwd_serial || g->graph_pages.empty()) {
        set_error("%s: the handle's last forward was not asep_gnn_forward_batch[_dev]", fn);
        return nullptr;
    }
    if (page < 0 || page >= (int)g->graph_pages.size()) {
        set_error("%s: page %d, the last call had %zu pages", fn, page, g->graph_pages.size());
        return nullptr;
    }
    return &g->graph_pages[(size_t)page];
}

}  // namespace

extern "C" {

int asep_gnn_forward_batch_dev(asep_gnn* g, int n_pages, const int32_t* N, const int32_t* E, const int32_t* R, const float* d_node_feat,
                               const int32_t* d_edges, const float* d_edge_feat, const int32_t* d_relations, float* d_probs_out,
                               size_t max_floats, void* stream) {
    ASEP_GUARD_BEGIN
    const char* fn = "asep_gnn_forward_batch_dev";
    GnnPageTable tab;
    GnnUnitTables units;
    if (int rc = batch_graph_checks(g, fn, n_pages, N, E, R, d_node_feat, d_edges, d_edge_feat, d_probs_out, max_floats, tab, units)) return rc;
    return forward_batch_impl(g, tab, units, d_edges, d_node_feat, d_edge_feat, d_relations, d_probs_out, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_gnn_forward_batch(asep_gnn* g, int n_pages, const int32_t* N, const int32_t* E, const int32_t* R, const float* node_feat,
                           const int32_t* edges, const float* edge_feat, const int32_t* relations, float* probs_out, size_t max_floats) {
    ASEP_GUARD_BEGIN
    const char* fn = "asep_gnn_forward_batch";
    GnnPageTable tab;
    GnnUnitTables units;
    int rc = batch_graph_checks(g, fn, n_pages, N, E, R, node_feat, edges, edge_feat, probs_out, max_floats, tab, units);
    if (rc) return rc;
    if (tab.edges > 0 && (rc = check_page_indices(fn, "interacting_nodes", edges, tab, false))) return rc;
    if (relations && tab.rels > 0 && (rc = check_page_indices(fn, "relations", relations, tab, true))) return rc;
    const size_t no = (size_t)tab.rels;
    const StagedGraph st = stage_graph(g, (size_t)tab.nodes, (size_t)tab.edges, no, no, edges, node_feat, edge_feat, relations);
    rc = forward_batch_impl(g, tab, units, st.e, st.u, st.f, st.r, st.o, nullptr);
    if (rc) return rc;
    if (no) ASEP_HIP_CHECK(hipMemcpyAsync(probs_out, st.o, no * sizeof(float), hipMemcpyDeviceToHost, nullptr));
    ASEP_HIP_CHECK(hipStreamSynchronize(nullptr));
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_gnn_get_page_hidden(asep_gnn* g, int page, float* out, size_t max_floats) {
    ASEP_GUARD_BEGIN
    const char* fn = "asep_gnn_get_page_hidden";
    const GnnPageRow* r = graph_batch_page(g, fn, page);
    if (!r) return ASEP_ERR_ARG;
    const size_t cnt = (size_t)r->N * g->H;
    if (!out || max_floats < cnt) { set_error("%s: buffer too small (%zu floats needed)", fn, cnt); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipStreamSynchronize(g->stream));
    ASEP_HIP_CHECK(hipMemcpy(out, g->d_h + (size_t)r->node_off * g->H, cnt * sizeof(float), hipMemcpyDeviceToHost));
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_gnn_get_page_edges(asep_gnn* g, int page, int32_t* out_edges, int32_t* out_first, int max_edges) {
    ASEP_GUARD_BEGIN
    const char* fn = "asep_gnn_get_page_edges";
    const GnnPageRow* r = graph_batch_page(g, fn, page);
    if (!r) return ASEP_ERR_ARG;
    ASEP_HIP_CHECK(hipStreamSynchronize(g->stream));
    int ends[2] = {0, 0};
    ASEP_HIP_CHECK(hipMemcpy(&ends[0], g->gb_rowptr + r->node_off, sizeof(int), hipMemcpyDeviceToHost));
    ASEP_HIP_CHECK(hipMemcpy(&ends[1], g->gb_rowptr + r->node_off + r->N, sizeof(int), hipMemcpyDeviceToHost));
    const int cnt = ends[1] - ends[0];
    if (cnt < 0 || (cnt > 0 && (!out_edges || max_edges < cnt))) { set_error("%s: page %d has %d corrected edges, the buffer holds %d", fn, page, cnt, max_edges); return ASEP_ERR_ARG; }
    if (cnt > 0) {
        ASEP_HIP_CHECK(hipMemcpy(out_edges, g->gb_sorted + 2 * (size_t)ends[0], (size_t)cnt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < 2 * cnt; ++i) out_edges[i] -= r->node_off;       // node numbers of the call -> of the page
        if (out_first) ASEP_HIP_CHECK(hipMemcpy(out_first, g->gb_sfirst + ends[0], (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return cnt;
    ASEP_GUARD_END
}

long asep_gnn_batch_launches(const asep_gnn* g) { return g ? g->batch_launches : ASEP_ERR_ARG; }

}  // extern "C"
