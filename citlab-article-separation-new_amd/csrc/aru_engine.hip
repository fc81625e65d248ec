// ARU-Net inference engine (host side): the packed weights (fragment orders: aru_pack.h) on the device, buffer
// management and the layer schedule of ARU_v1.py:62-294.  Entry points: include/asep_hip.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>

#include "aru_kernels.h"
#include "res8_kernels.h"
#include "res8v_kernels.h"
#include "bf16_kernels.h"
#include "res8w_kernels.h"
#include "res8ws_kernels.h"
#include "level0_plan.h"
#include "launch_plan.h"
#include "convr_kernels.h"
#include "split_kernels.h"
#include "pyr_kernels.h"
#include "asep_common.h"
#include "aru_pack.h"

using namespace asep;

namespace {

struct Tensor {
    float* p = nullptr;    // bf: the buffer holds bf16 (2 bytes per element; native bf16 path), accessed through bp()
    int H = 0, W = 0, C = 0;
    bool bf = false;
    size_t count() const { return (size_t)H * W * C; }
    bf16_t* bp() const { return reinterpret_cast<bf16_t*>(p); }
};

// A convolution whose weights are packed as the A operand of v_mfma_f32_16x16x4_f32: its shape decisions (ConvPlan, aru_pack.h) + the packed filters
struct PackedConv : ConvPlan {
    float* d_w = nullptr;
    float* d_b = nullptr;
    float* d_wino = nullptr;   // Winograd F(2x2,3x3) transformed weights U = G g G^T, packed [g][pos][mtile][lane][4]
    float* d_wv = nullptr;     // scalar-operand filters of the vector-ALU kernels: deconv 16 -> 8 [tap][ci][co] (deconv8v_kernel),
                               // 4x4 conv 32 -> 1 [tap][ci] (conv_c1out_kernel)
    bf16_t* d_wb = nullptr;    // conv: [chunk][mtile][lane][8]; deconv: MODE 2 [G][tap][mtile][lane][8], MODE 1 [frag 0..5][mtile][lane][8]
    bf16_t* d_wb8 = nullptr;   // deconv 16 -> 8 (level 0): the three class-pair fragments of deconvb8_kernel [3][lane][8]
    bf16_t* d_ws = nullptr;    // the filter as three bf16 parts, [chunk][part h, m, l][mtile][lane][8]
    bf16_t* d_ws16 = nullptr;  // 3x3, Cin % 16 == 0, Cin >= 32: stages of 16 channels, chunk = two taps (convs16_kernel): [stage][chunk 5][part][mtile][lane][8]
};

struct DirectConv {        // first layers on the vector ALU: Cin == 1 (conv_c1_kernel), or Cin == 3 of a colour net (conv_c3_kernel)
    int k = 0, cout = 0, cin = 1;
    float* d_w = nullptr;  // [k*k][cin][cout]
    float* d_b = nullptr;
};

}  // namespace

struct asep_aru {
    asep_aru_cfg cfg{};
    std::map<std::string, PackedConv> convs;   // keyed by variable scope, e.g. "aru_net/featMapG/unet_down_1/convR_0"
    struct ResB { int C = 0; bf16_t* d_w = nullptr; float* d_b = nullptr; };
    std::map<std::string, ResB> resb;          // bf16 path: fused residual-block tails (8- / 16-channel levels), keyed by block scope
    std::map<std::string, float*> taps;        // RU_v2 (cfg.input_pyramid): the image rows of a block's conv1 [9][channels][cout] (pyr_tap_kernel), keyed by the conv's scope
    // bf16 path, whole level-0 blocks in one kernel each (res8b_kernel): pixel-pair A fragments
    bf16_t* d_r8b_down_w = nullptr;  // [3 convs][3 ky][64][8]
    float* d_r8b_down_b = nullptr;   // [3][8]
    bf16_t* d_r8b_up_w1 = nullptr;   // conv1 of unet_up_0 [3 ky][2 halves][64][8]
    bf16_t* d_r8f_up_w1 = nullptr;   // the same for res8f_kernel's planar input tile [3 ky][2 sources][64][8]: k = 8 (window pixel kk) + channel of the source
    bf16_t* d_r8f_down_w1 = nullptr; // conv1 of unet_down_0 as ONE pair fragment [64][8] (k = window row / column, res8f_kernel)
    float* d_r8b_down_w1r = nullptr; // the same filter [9][8] as fp32 values rounded to bfloat16 (border tiles, res8b_tile)
    bool use_res32 = true;           // ASEP_BF_RES32=0: the 32-channel residual tails layer by layer (convb_kernel)
    int walk_mode = 1;               // ASEP_BF_WALK: 1 both level-0 blocks on the walkers (default), 2 the UP block only, 0 neither
    bool use_deconvs = true;         // ASEP_SPLIT_DECONV=0: the deconvolutions of the f32s engine on the fp32 MFMA (deconv_mfma_kernel) instead of split products
    bool use_convr = true;           // ASEP_BF_CONVR=0: the 64 -> 64 layers on convb_kernel instead of the register-resident form (convr_kernels.h)
    unsigned char* d_zero_trash = nullptr;   // 16 zero bytes (padding source of convr_kernel) + 4 KB behind them that nobody reads (its dump)
    int fused_act = 0;               // bf16 engine, elu / leaky RESIDUAL graphs (round 6): the level-0 blocks and the 16-channel tails on the general fused forms
                                     // res8b_kernel<UP, ACT> / resb_tail_kernel<16, ACT> (activation on the fp32 sums before the rounding); 0: ReLU graph, or layer by layer
    bool use_walk = true;            // ASEP_BF_WALK=0: the level-0 blocks as 16 x 32 tiles (res8f_kernel) instead of the column-strip walkers (res8w_kernels.h)
    bf16_t* d_r8b_up_w = nullptr;    // [3][3][64][8]
    float* d_r8b_up_b = nullptr;     // [3][8]
    float* d_r8b_up_b1 = nullptr;    // [8]
    DirectConv det_first, att_first;
    // fused level-0 residual blocks (feat_root == 8, res_depth == 3): pixel-pair MFMA fragments
    float* d_r8_down_wr = nullptr;   // [3][6][64][4]
    float* d_r8_down_br = nullptr;   // [3][8]
    float* d_r8_up_w1 = nullptr;     // unet_up_0/conv1 as two 8-channel pixel-pair passes [2][6][64][4]
    float* d_r8_up_wr = nullptr;     // [3][6][64][4]
    float* d_r8_up_br = nullptr;     // [3][8]
    float* d_r8_up_b1 = nullptr;     // [8]
    // the same filters in scalar layout for the fp32 vector-ALU kernels (res8v_kernels.h)
    float* d_r8v_down_wr = nullptr;  // [3][R8V_FILTER]
    float* d_r8v_up_w1 = nullptr;    // [2][R8V_FILTER]
    float* d_r8v_up_wr = nullptr;    // [3][R8V_FILTER]
    bool r8_valu = true;             // fp32 only; ASEP_R8_VALU=0 runs the fp32 MFMA variants instead
    // f32s engine, ReLU graph: the level-0 blocks as split-product strip walkers (res8ws_kernels.h); three-part pair fragments [..][part 3][64][8]
    bool use_split_walk = true;      // ASEP_SPLIT_WALK=0: f32s level 0 on res8v_*_kernel instead
    bf16_t* d_r8ws_down_w = nullptr; // [3 convs][3 ky][3 parts][64][8]
    bf16_t* d_r8ws_up_w = nullptr;   // [3 convs][3 ky][3 parts][64][8]
    bf16_t* d_r8ws_up_w1 = nullptr;  // conv1 of unet_up_0 [3 ky][2 sources][3 parts][64][8]
    bool use_fused8 = true;          // ASEP_FUSED8=0 falls back to the layer-by-layer kernels
    bool fused8_wanted = true;       // what ASEP_FUSED8 said (use_fused8 is also switched off for the graph variants)
    bool fused8_var = false;         // elu / leaky RESIDUAL graphs: the level-0 blocks on res8v_*_kernel<activation> (round 4)
    float* d_att_head = nullptr;     // A fragment of attPart/conv1 for att_head_kernel (12 output channels, 4x4 taps)
    bf16_t* d_att_headb = nullptr;   // the same as ONE bf16 fragment [64][8] (att_headb_kernel, bf16 path)
    float* d_logit_w = nullptr;
    float* d_logit_b = nullptr;
    float* d_logit_wd = nullptr;     // two classes: [16][feat_root] class-1 minus class-0 filter + the bias difference (combine_kernel behind a soft-max)
    float* d_stats = nullptr;      // mvn {mean, 1/std}
    const float* const* page_stats = nullptr;   // aru_set_page_stats: per page of the next forward its {mean, 1/std}, computed by the caller
    double* d_sums = nullptr;
    // A lane = one in-order chain of launches (stream + its buffer pool + a side stream for the attention branch).
    // A batch of pages is split over the lanes so that two independent chains fill each other's launch tails.
    struct Lane {
        hipStream_t s = nullptr;         // lane 0 uses the caller's stream
        bool own_stream = false;
        hipStream_t side = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_begin = nullptr, ev_done = nullptr;
        hipStream_t bside = nullptr;     // the border tiles of the strip walkers run beside the walkers (run_res8w); not the attention branch's
        hipEvent_t ev_bfork = nullptr, ev_bjoin = nullptr;   // stream: its chain is busy while the level-0 down block runs
        BufferPool pool;
        ~Lane() {
            if (ev_fork) (void)hipEventDestroy(ev_fork);
            if (ev_bfork) (void)hipEventDestroy(ev_bfork);
            if (ev_bjoin) (void)hipEventDestroy(ev_bjoin);
            if (ev_join) (void)hipEventDestroy(ev_join);
            if (ev_begin) (void)hipEventDestroy(ev_begin);
            if (ev_done) (void)hipEventDestroy(ev_done);
            if (side) (void)hipStreamDestroy(side);
            if (bside) (void)hipStreamDestroy(bside);
            if (own_stream && s) (void)hipStreamDestroy(s);
        }
    };
    std::vector<std::unique_ptr<Lane>> lanes;
    Lane* cur = nullptr;
    int last_nl = 0;                     // lanes of the previous call: a call with another count releases every lane's arena first (below)
    bool lanes_forced = false;           // ASEP_LANES given: split any batch of >= 2 pages
    int num_lanes = 2;                   // page lanes of a batch call (ASEP_LANES overrides).  Two lanes since round 6: two independent chains fill each other's launch
                                         // tails (r4j: 1 / 2 / 3 / 4 lanes = 119.3 / 121.2 / 120.3 / 115.8 pages/s fp32; round 5: 1 / 2 / 3 = 467 / 477 / 478 bf16, 137.6 / 139.8
                                         // f32s; the round-5 driver run: f32s 135.8 -> 138.4, bf16 469.6 -> 487.5, outputs bit-identical).  A lane takes at least four pages, so
                                         // calls of fewer than eight pages stay on one lane.  Two launches of one kernel then share the chip and each takes about twice as long,
                                         // so a per-launch figure must not be taken from that schedule: while a handle records launch times (asep_aru_profile, any mode) its
                                         // calls run on ONE lane -- the bench line's roofline block and rocprofv3's averages of the event-timed steps describe a kernel, not the
                                         // sharing (DESIGN_LESSONS 47, 49)
    std::map<std::string, Tensor> endpoints;
    hipStream_t stream = nullptr;
    std::vector<void*> owned;

    // optional per-launch timing with HIP events on the launch stream (bench.py roofline leg)
    struct ProfRec { int kid; double flops, bytes, xflops; hipEvent_t a, b; };
    int num_cus = 256;
    BufferPool host_stage;         // device staging of the host-pointer entry point (grow-only)
    hipStream_t host_stream = nullptr;   // transfers + forward of the host-pointer entry point (created on first use)
    bool use_xcd_sched = true;     // ASEP_XCD_SCHED=0: identity tile order (persistent kernels: no tile table; one-shot kernels: no XCD bands)
    std::map<std::string, const int32_t*> sched_cache;
    bool bf16 = false;             // cfg.compute_dtype == 1: native bf16 data path (bf16_kernels.h): bf16 activations in HBM / LDS,
                                   // v_mfma_f32_16x16x32_bf16 with fp32 accumulation; fp32 image in, fp32 probabilities out
    bool split = false;            // cfg.compute_dtype == 2: fp32 tensors and accumulation, every product of the convolutions with >= 12 input channels
                                   // as six bf16 x bf16 partial products (split_kernels.h).  Level 0 stays on the vector-ALU blocks (DESIGN_LESSONS 32)
    bool use_c12 = true;           // ASEP_C12=0: 12-channel inputs padded to a 16-channel group (read when the weights are packed)
    bool fuse_pool = true;         // ASEP_FUSE_POOL=0: separate maxpool2_kernel after every conv
    bool fuse_act = true;          // ASEP_FUSE_ACT=0: elu / leaky of the graph variants as a separate act_kernel pass behind every conv
    bool profiling = false;
    bool prof_detail = false;      // per-layer names (scope + spatial size) instead of per-kernel names
    bool prof_in_situ = false;     // keep the attention side stream while recording (times include what shares the chip)
    std::vector<std::string> prof_names;
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;

    ~asep_aru() {
        for (void* p : owned)
            if (p) (void)hipFree(p);
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        if (host_stream) (void)hipStreamDestroy(host_stream);
    }
    hipEvent_t next_event() {
        if (ev_next == ev_pool.size()) {
            hipEvent_t e;
            ASEP_HIP_CHECK_THROW(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
        return ev_pool[ev_next++];
    }
    int prof_kid(const std::string& name) {
        for (size_t i = 0; i < prof_names.size(); ++i)
            if (prof_names[i] == name) return (int)i;
        prof_names.push_back(name);
        return (int)prof_names.size() - 1;
    }
    int feat(int l) const { return cfg.feat_root << l; }
    // n elements of device memory that the handle owns from the moment they exist; throws HipError
    template <class T>
    T* alloc(size_t n) {
        owned.push_back(nullptr);
        ASEP_HIP_CHECK_THROW(hipMalloc(&owned.back(), n * sizeof(T)));
        return (T*)owned.back();
    }
    // the one way of putting a host vector on the device (never less than 16 bytes: 4 floats, 8 bf16); throws HipError
    template <class T>
    T* put(const std::vector<T>& h) {
        T* d = alloc<T>(std::max(h.size(), 16 / sizeof(T)));
        ASEP_HIP_CHECK_THROW(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class T>
    T* put_some(const std::vector<T>& h) { return h.empty() ? nullptr : put(h); }   // a vector left empty by its packer: the member stays unset
};

namespace {

// Brackets one kernel launch with two events when profiling is on (no-op otherwise).
// Names are the kernels' rocprofv3 names without "void ", "asep::", blanks and the argument list (every template
// argument spelled out), so that scripts/roofline_from_profiles.py can join the two sources without a name table.
struct ProfScope {
    asep_aru* m;
    hipEvent_t a = nullptr, b = nullptr;
    bool on = false;
    double flops;
    double xflops = -1;        // EXECUTED FLOPs where they differ from the algorithmic credit (< 0: the same)
    double bytes = 0;          // ALGORITHMIC HBM bytes of the launch: every input tensor read once, every output written once, the filter
                               // once (SURVEY.md section 8d per-unit figure x the units of the launch); set by the launcher
    std::string name, detail;
    ProfScope(asep_aru* m_, const std::string& name_, double flops_, const std::string& detail_ = std::string())
        : m(m_), flops(flops_), name(name_), detail(detail_) {
        if (!m->profiling) return;
        on = true;
        a = m->next_event();
        b = m->next_event();
        ASEP_HIP_CHECK_THROW(hipEventRecord(a, m->stream));
    }
    void set_name(const std::string& n) { name = n; }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(b, m->stream);
        m->prof_recs.push_back({m->prof_kid(m->prof_detail && !detail.empty() ? name + " " + detail : name), flops, bytes, xflops < 0 ? flops : xflops, a, b});
    }
};
std::string targs(std::initializer_list<std::string> l) {
    std::string s = "<";
    for (const std::string& x : l) s += (s.size() > 1 ? "," : "") + x;
    return s + ">";
}
inline std::string tb(bool b) { return b ? "true" : "false"; }
inline std::string ti(int i) { return std::to_string(i); }

// a schedule table on the device, owned by the handle; nullptr when it cannot be put there (the callers' contract)
const int32_t* put_table(asep_aru* m, const std::vector<int32_t>& t) {
    try {
        return m->put(t);
    } catch (const HipError&) {
        return nullptr;
    }
}

// XCD-aware order of the persistent fused kernels' tiles.  Workgroups are dealt round-robin to the 8 XCDs (block b
// runs on XCD b % 8, each with its own 4 MB L2).  In the order of xcd_order (launch_plan.h) the 32 blocks of an XCD work on spatially adjacent
// tiles at the same time, and on the rows just below right after, so the 8-row / 14-column halo overlap of neighbouring tiles is served by
// that XCD's L2 instead of being fetched again.
//
// work unit -> tile table of the PERSISTENT kernels (res8v_*, res32_tail_kernel: resident blocks walk the units with a grid stride) for the
// problems' tile grids `probs`, cached on the device.  nullptr on failure: identity.
const int32_t* xcd_schedule(asep_aru* m, const std::vector<TileDims>& probs, int total) {
    std::string key = "u";
    for (const TileDims& q : probs) key += ":" + std::to_string(q.tx) + "x" + std::to_string(q.ty);
    auto it = m->sched_cache.find(key);
    if (it != m->sched_cache.end()) return it->second;
    const std::vector<int32_t> sched = xcd_order(probs, total);      // (launch_plan.h)
    if (sched.empty()) return nullptr;
    const int32_t* d = put_table(m, sched);
    if (d) m->sched_cache[key] = d;
    return d;
}

// the persistent fp32 level-0 kernels: nblocks resident blocks, unit k = block + i * nblocks
const int32_t* tile_schedule(asep_aru* m, const Res8Args& a, int nblocks, int unit_h) {
    if (!m->use_xcd_sched || nblocks % 8 != 0 || a.total_tiles < 2 * nblocks) return nullptr;
    std::vector<TileDims> probs;
    for (int i = 0; i < a.nprob; ++i) probs.push_back({a.p[i].tiles_x, (a.p[i].H + unit_h - 1) / unit_h, a.p[i].tile_begin});
    return xcd_schedule(m, probs, a.total_tiles);
}

// one-shot kernels (one block per tile): XCD bands (XcdMap, aru_kernels.h) from a few waves of blocks per XCD on.  *n_units = blocks to launch
// along x (the grid is padded to eight equal chunks; surplus blocks leave at once).
XcdMap oneshot_map(asep_aru* m, int total, int* n_units) {
    const OneshotPlan p = oneshot_plan(total, m->use_xcd_sched);     // (launch_plan.h)
    if (n_units) *n_units = p.units;
    return XcdMap{p.chunk, total};
}

// ---- kernel launchers: every launch covers one layer of a LIST of problems (pages x scales) -----------------
typedef std::vector<Tensor> TL;

Tensor new_tensor(asep_aru* m, int H, int W, int C, bool bf = false) {     // bf: a bf16 tensor of the native bf16 path
    Tensor t;
    t.H = H; t.W = W; t.C = C; t.bf = bf;
    t.p = (float*)m->cur->pool.get(t.count() * (bf ? sizeof(bf16_t) : sizeof(float)));
    return t;
}

inline double tbytes(const Tensor& t) { return (double)t.count() * (t.bf ? 2.0 : 4.0); }

std::string dims_of(const TL& l) {
    std::string d;
    for (size_t i = 0; i < l.size() && i < 3; ++i) d += (i ? "+" : "") + std::to_string(l[i].H) + "x" + std::to_string(l[i].W);
    if (l.size() > 3) d += "+..(" + std::to_string(l.size()) + ")";
    return d;
}

// the usual layer text of a profiler record: scope, the pages of the launch, channels in -> out
std::string layer_text(const std::string& scope, const TL& sub, int cin, int cout) {
    return scope + " " + dims_of(sub) + " " + std::to_string(cin) + "->" + std::to_string(cout);
}

// One launch of a launcher: problems [b0, b1) of its list, the numbering of their work units (launch_plan.h) and the record's sums so far.
struct Chunk {
    size_t b0, b1;
    UnitCounter units;
    double flops = 0, bytes = 0;
    TL sub(const TL& l) const { return TL(l.begin() + b0, l.begin() + b1); }
};
template <class A> auto set_total(A& a, int t, int) -> decltype((void)(a.total_tiles = t)) { a.total_tiles = t; }
template <class A> auto set_total(A& a, int t, long) -> decltype((void)(a.total = t)) { a.total = t; }
template <class A> void set_total(A&, int, ...) {}
// The skeleton of every layer launcher: the n problems of a list in launches of at most MAXP.  Per launch a value-initialised Args; fill(p, i, k)
// sets slot p = a.p[i - b0] of problem i, takes its unit numbers from k.units and adds its flops and bytes to k (bytes starts at bytes0, the
// launcher's filter term); then nprob and the total (where Args has one) are set and launch(a, k) picks the kernel and launches.
template <class Args, class Fill, class Launch>
void for_chunks(size_t n, double bytes0, Fill fill, Launch launch) {
    for (size_t c = 0; c < num_chunks(n); ++c) {
        Args a{};
        Chunk k{chunk_begin(c), chunk_end(n, c)};
        k.bytes = bytes0;
        for (size_t i = k.b0; i < k.b1; ++i) fill(a.p[i - k.b0], i, k);
        a.nprob = (int)(k.b1 - k.b0);
        set_total(a, k.units.total, 0);
        launch(a, k);
    }
}
// problem slot <- its 2-D tile numbering
template <class P>
void set_tiles(P& p, const Units& u) { p.tiles_x = u.per_row; p.tile_begin = u.begin; }

// launches conv_mfma_kernel<...> and gives the profiler record that instantiation's exact name
#define ASEP_CONV_LAUNCH(KH_, KW_, MT_, C8_, TH_, DB_, BF_, C12_, MB_)                                                   \
    do {                                                                                                                 \
        ps.set_name("conv_mfma_kernel" + targs({ti(KH_), ti(KW_), ti(MT_), tb(C8_), ti(TH_), tb(DB_), tb(BF_), tb(C12_), ti(MB_)})); \
        hipLaunchKernelGGL((conv_mfma_kernel<KH_, KW_, MT_, C8_, TH_, DB_, BF_, C12_, MB_>), grid, dim3(256), 0, s, a);  \
    } while (0)

template <int KH, int KW>
void launch_conv_k(asep_aru* m, const PackedConv& pc, const ConvArgs& a, int total_tiles, double flops, double bytes,
                   const std::string& scope, const TL& in0, bool big_tile) {
    const int mt = pc.c8 ? 1 : (pc.mtiles % 4 == 0 ? 4 : (pc.mtiles % 2 == 0 ? 2 : 1));
    dim3 grid(total_tiles, pc.mtiles / mt);                  // (total_tiles = the schedule's units: padded to 8 when grid.y > 1)
    ProfScope ps(m, "conv_mfma_kernel", flops, layer_text(scope, in0, pc.cin, pc.cout));
    ps.bytes = bytes;
    hipStream_t s = m->stream;
    const bool res_op = a.p[0].res != nullptr;
    const bool has_res = res_op || KH != 3;      // (the four-blocks-per-CU variant exists for 3x3 only: 4x4 needs 140 VGPRs)
    if constexpr (KW == 4) {
        if (pc.c12) {                                        // one m-tile, one channel group: 16 x 32 tiles, single LDS buffer
            ASEP_CONV_LAUNCH(KH, KW, 1, false, 16, false, false, true, 2);
            return;
        }
    }
    if constexpr (KH == 3) {
        if (pc.c8 && big_tile && !res_op) {                  // 8 -> 16 (level-1 conv1): 16 x 32-pixel blocks, four per CU
            ASEP_CONV_LAUNCH(3, 3, 1, true, 16, false, false, false, 4);
            return;
        }
    }
    if (pc.c8) ASEP_CONV_LAUNCH(KH, KW, 1, true, CONV_TH, true, false, false, 2);
    else if (mt == 1 && big_tile && !has_res) ASEP_CONV_LAUNCH(3, 3, 1, false, 16, false, false, false, 4);
    else if (mt == 1 && big_tile) ASEP_CONV_LAUNCH(KH, KW, 1, false, 16, false, false, false, 2);
    else if (mt == 4) ASEP_CONV_LAUNCH(KH, KW, 4, false, CONV_TH, true, false, false, 2);
    else if (mt == 2 && !res_op) ASEP_CONV_LAUNCH(KH, KW, 2, false, CONV_TH, true, false, false, 3);   // no residual prefetch: three blocks per CU
    else if (mt == 2) ASEP_CONV_LAUNCH(KH, KW, 2, false, CONV_TH, true, false, false, 2);
    else ASEP_CONV_LAUNCH(KH, KW, 1, false, CONV_TH, true, false, false, 2);
}

enum PoolKind { POOL_MAX, POOL_AVG_C1, POOL_CHANSUM, POOL_AVG_C3 };
TL run_pool(asep_aru* m, const TL& in, PoolKind kind);
// launchers of the kernels that are instantiated at the end of this file (see the note there)
void launch_conv_c1_12(asep_aru* m, const C1Args& a, int tiles);
void launch_avgpool_c3(asep_aru* m, const PoolArgs& a, dim3 grid);
void launch_pyr_tap(asep_aru* m, const TapArgs& a, int ch, int tiles);
void launch_combine12(const CombineArgs& ca, dim3 grid, int nsct, hipStream_t stream);

// launches convs_kernel<...> under that instantiation's name
#define ASEP_CONVS_LAUNCH(KH_, KW_, C16_, MT_, TH_, MB_)                                                              \
    do {                                                                                                              \
        ps.set_name("convs_kernel" + targs({ti(KH_), ti(KW_), tb(C16_), ti(MT_), ti(TH_), ti(MB_)}));                 \
        hipLaunchKernelGGL((convs_kernel<KH_, KW_, C16_, MT_, TH_, MB_>), grid, dim3(256), 0, m->stream, a);          \
    } while (0)

// the filter term of a conv launch's bytes (esize bytes per value) and the problem slot of the fp32 / f32s conv launchers: operands, tw x th tiles,
// 2 * MAC flops, every operand tensor once
double conv_wbytes(const PackedConv& pc, double esize) { return (double)pc.kh * pc.kw * pc.cin * pc.cout * esize; }
auto conv_fill(const PackedConv& pc, int tw, int th, const TL& in0, const TL* in1, const TL* res, const TL& out, const TL* pool) {
    return [=, &pc, &in0, &out](ConvProb& p, size_t i, Chunk& k) {
        p.in0 = in0[i].p; p.in1 = in1 ? (*in1)[i].p : nullptr; p.res = res ? (*res)[i].p : nullptr;
        p.out = out.empty() ? nullptr : out[i].p;
        p.pool = pool ? (*pool)[i].p : nullptr;
        p.H = p.Ho = in0[i].H; p.W = p.Wo = in0[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, tw, th));
        k.flops += 2.0 * in0[i].H * in0[i].W * pc.kh * pc.kw * (double)pc.cin * pc.cout;
        k.bytes += tbytes(in0[i]) + (in1 ? tbytes((*in1)[i]) : 0.0) + (res ? tbytes((*res)[i]) : 0.0) + (out.empty() ? 0.0 : tbytes(out[i])) +
                   (pool ? tbytes((*pool)[i]) : 0.0);
    };
}

// a conv layer on the split-product kernel (split_kernels.h): same operands and results as run_conv's fp32 kernels
TL run_conv_split(asep_aru* m, const PackedConv& pc, const std::string& scope, const TL& in0, const TL* in1, bool relu_in, bool relu_out,
                  const TL* res, TL* pooled, bool keep_full, int act) {
    const bool fuse_pool = pooled && m->fuse_pool;
    TL out;
    if (keep_full || !fuse_pool)
        for (const Tensor& t : in0) out.push_back(new_tensor(m, t.H, t.W, pc.cout));
    if (fuse_pool) {
        pooled->clear();
        for (const Tensor& t : in0) pooled->push_back(new_tensor(m, (t.H + 1) / 2, (t.W + 1) / 2, pc.cout));
    }
    const bool c16 = pc.smode == 1;
    // (measured, 4 pages per launch: 32 -> 16 1230 -> 930 us on convs16_kernel, but 64 -> 64 378 -> 405 and 32 -> 32 431 -> 534: with more than one
    //  m-tile the barrier per chunk and the 16-channel stages cost more than the shared fragments save: one-m-tile layers only.
    //  The same kernel with the fragments fetched per wave (ALDS = false; 16-channel stages + halo prefetch only) spills and was slower still:
    //  521 / 527 us for those two layers -- not instantiated)
    const bool alds = pc.d_ws16 && pc.mtiles == 1;
    const int mt = (pc.mtiles % 4 == 0 && !c16) ? 4 : (pc.mtiles % 2 == 0 ? 2 : 1);
    const int th = (c16 && pc.kh == 3 && mt == 1) ? 16 : 8;
    for_chunks<ConvArgs>(in0.size(), conv_wbytes(pc, 4.0), conv_fill(pc, CONV_TW, th, in0, in1, res, out, fuse_pool ? pooled : nullptr), [&](ConvArgs& a, const Chunk& k) {
        a.c0 = in0[0].C; a.c1 = in1 ? (*in1)[0].C : 0;
        a.wpk = (const f32x4*)(alds ? pc.d_ws16 : pc.d_ws); a.bias = pc.d_b;
        a.cout = pc.cout; a.mtiles = pc.mtiles; a.groups = alds ? pc.cin / 16 : pc.cin / 32;
        a.relu_in = relu_in; a.relu_out = relu_out; a.act = act;
        a.skip_full = fuse_pool && !keep_full;
        int units;
        a.xm = oneshot_map(m, k.units.total, &units);
        dim3 grid(units, pc.mtiles / mt);
        ProfScope ps(m, "convs_kernel", k.flops, layer_text(scope, k.sub(in0), pc.cin, pc.cout));
        ps.bytes = k.bytes;
        if (alds) {                                          // (one m-tile: mt == 1)
            ps.set_name("convs16_kernel<1,8,3,true>");
            hipLaunchKernelGGL((convs16_kernel<1, 8, 3, true>), grid, dim3(256), 0, m->stream, a);
        } else if (pc.kh == 3) {
            if (c16 && th == 16) ASEP_CONVS_LAUNCH(3, 3, true, 1, 16, 2);
            else if (c16 && mt == 2) ASEP_CONVS_LAUNCH(3, 3, true, 2, 8, 3);
            else if (c16) ASEP_CONVS_LAUNCH(3, 3, true, 1, 8, 3);
            else if (mt == 4) ASEP_CONVS_LAUNCH(3, 3, false, 4, 8, 2);
            else if (mt == 2) ASEP_CONVS_LAUNCH(3, 3, false, 2, 8, 2);
            else ASEP_CONVS_LAUNCH(3, 3, false, 1, 8, 2);
        } else {
            if (c16 && mt == 2) ASEP_CONVS_LAUNCH(4, 4, true, 2, 8, 2);
            else if (c16) ASEP_CONVS_LAUNCH(4, 4, true, 1, 8, 2);
            else { set_error("internal: conv %s (4x4, %d input channels) was packed for the split-product kernel", scope.c_str(), pc.cin); throw ArgError(); }
        }
    });
    if (pooled && !fuse_pool) *pooled = run_pool(m, out, POOL_MAX);
    return out;
}

// stride-1 SAME conv on the (optionally concatenated) inputs of every problem

// pooled != nullptr: also produce maxpool2 of the output.  The direct kernels and the register-resident Winograd kernel take
// the 2x2 max in their epilogue (ConvProb::pool); the others are followed by maxpool2_kernel.  keep_full = false: the caller
// reads only the pooled tensor (attention CNN), so the unpooled one is not stored (and the returned list is empty) when the
// pool is fused.
TL run_conv(asep_aru* m, const std::string& scope, const TL& in0, const TL* in1, bool relu_in, bool relu_out,
            const TL* res, TL* pooled = nullptr, bool keep_full = true, int act = 0) {
    auto it = m->convs.find(scope);
    if (it == m->convs.end()) { set_error("internal: conv %s not packed", scope.c_str()); throw ArgError(); }
    const PackedConv& pc = it->second;
    const int cin = in0[0].C + (in1 ? (*in1)[0].C : 0);
    if (cin != pc.cin) {
        set_error("internal: conv %s expects Cin=%d, got %d", scope.c_str(), pc.cin, cin);
        throw ArgError();
    }
    if (!((pc.kh == 3 && pc.kw == 3) || (pc.kh == 4 && pc.kw == 4))) {
        set_error("conv %s: unsupported kernel size %dx%d", scope.c_str(), pc.kh, pc.kw);
        throw ArgError();
    }
    if (pc.d_wv && pc.cout == 1 && m->r8_valu && !in1 && !res && !pooled) {
        // single output channel (attention conv4): one pixel per thread on the vector ALU
        TL out1;
        for (const Tensor& t : in0) out1.push_back(new_tensor(m, t.H, t.W, 1));
        for_chunks<ConvArgs>(in0.size(), 0.0, [&](ConvProb& p, size_t i, Chunk& k) {
            p.in0 = in0[i].p; p.out = out1[i].p;
            p.H = p.Ho = in0[i].H; p.W = p.Wo = in0[i].W;
            set_tiles(p, k.units.next_tiles(p.H, p.W, C1O_T, C1O_T));
            k.flops += 2.0 * in0[i].H * in0[i].W * 16.0 * pc.cin;
            k.bytes += tbytes(in0[i]) + tbytes(out1[i]);
        }, [&](ConvArgs& a, const Chunk& k) {
            a.c0 = pc.cin; a.cout = 1;
            a.wpk = (const f32x4*)pc.d_wv; a.bias = pc.d_b;
            a.relu_in = relu_in; a.relu_out = relu_out; a.act = act;
            int units;
            a.xm = oneshot_map(m, k.units.total, &units);
            ProfScope ps(m, "conv_c1out_kernel", k.flops, scope);
            ps.bytes = k.bytes;
            hipLaunchKernelGGL(conv_c1out_kernel, dim3(units), dim3(256), 0, m->stream, a);
        });
        return out1;
    }
    if (m->split && pc.d_ws) return run_conv_split(m, pc, scope, in0, in1, relu_in, relu_out, res, pooled, keep_full, act);
    const bool wino = pc.d_wino && pc.mtiles > 1;            // (Winograd pays from 32 output channels: DESIGN_LESSONS 4, 16)
    const int wino_mt = pc.mtiles % 4 == 0 ? 4 : (pc.mtiles % 2 == 0 ? 2 : 1);
    const bool fuse_pool = pooled && m->fuse_pool && pc.cout % 4 == 0 && (!wino || wino_mt <= 2);
    TL out;
    if (keep_full || !fuse_pool)
        for (const Tensor& t : in0) out.push_back(new_tensor(m, t.H, t.W, pc.cout));
    if (fuse_pool) {
        pooled->clear();
        for (const Tensor& t : in0) pooled->push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), pc.cout));
    }
    // single channel group, one 16-channel output tile: 16 x 32 pixel blocks, single LDS buffer (more MFMA work per
    // block against the fixed load latency of these short blocks)
    // (two channel groups only for the residual-free 3x3 variant: four blocks per CU hide the refill of its single LDS buffer)
    const bool big_tile = !wino && (!pc.c8 || (pc.kh == 3 && !res)) && (pc.groups == 1 || (pc.groups == 2 && !res && pc.kh == 3)) && pc.mtiles == 1;
    // Winograd blocks are 4 x 32 output pixels, those of the register-resident variant for one m-tile 8 x 32
    const int tw = wino ? WINO_TW : CONV_TW, th = wino ? (wino_mt == 1 ? 2 * WINO_TH : WINO_TH) : (big_tile ? 16 : CONV_TH);
    for_chunks<ConvArgs>(in0.size(), conv_wbytes(pc, 4.0), conv_fill(pc, tw, th, in0, in1, res, out, fuse_pool ? pooled : nullptr), [&](ConvArgs& a, const Chunk& k) {
        a.c0 = in0[0].C; a.c1 = in1 ? (*in1)[0].C : 0;
        a.wpk = (const f32x4*)(wino ? pc.d_wino : pc.d_w); a.bias = pc.d_b;
        a.cout = pc.cout; a.mtiles = pc.mtiles; a.groups = pc.groups;
        a.relu_in = relu_in; a.relu_out = relu_out; a.act = act;
        a.skip_full = fuse_pool && !keep_full;
        const TL sub = k.sub(in0);
        int units;
        a.xm = oneshot_map(m, k.units.total, &units);
        if (wino) {
            const int mt = wino_mt;
            dim3 grid(units, pc.mtiles / mt);
            std::string pname;
            if (mt == 1) pname = "conv_winor_kernel<false,1,true>";
            else if (mt == 2) pname = !res ? "conv_winor_kernel<false,2,false>" : "conv_winor_kernel<false,2,true>";
            else pname = "conv_wino_kernel" + targs({ti(mt), tb(false)});
            ProfScope ps(m, pname, k.flops, layer_text(scope, sub, pc.cin, pc.cout));
            ps.bytes = k.bytes;
            if (mt == 1) {
                hipLaunchKernelGGL((conv_winor_kernel<false, 1, true>), grid, dim3(256), 0, m->stream, a);
            } else if (mt == 2) {
                // register-resident variant: a wave per (tile row, m-tile); grid.y counts pairs of m-tiles
                if (!res) hipLaunchKernelGGL((conv_winor_kernel<false, 2, false>), grid, dim3(256), 0, m->stream, a);
                else hipLaunchKernelGGL((conv_winor_kernel<false, 2, true>), grid, dim3(256), 0, m->stream, a);
            } else hipLaunchKernelGGL((conv_wino_kernel<4>), grid, dim3(256), 0, m->stream, a);
        } else if (pc.kh == 3) launch_conv_k<3, 3>(m, pc, a, units, k.flops, k.bytes, scope, sub, big_tile);
        else launch_conv_k<4, 4>(m, pc, a, units, k.flops, k.bytes, scope, sub, big_tile);
    });
    if (pooled && !fuse_pool) *pooled = run_pool(m, out, POOL_MAX);
    return out;
}

// conv2d_transpose 3x3 stride 2 SAME to the spatial sizes of `like` (ARU_v1.py:255-259)
TL run_deconv(asep_aru* m, const std::string& scope, const TL& in, const TL& like, bool relu_out, int act = 0) {
    auto it = m->convs.find(scope);
    if (it == m->convs.end()) { set_error("internal: deconv %s not packed", scope.c_str()); throw ArgError(); }
    const PackedConv& pc = it->second;
    if (pc.kh != 3 || pc.kw != 3 || in[0].C != pc.cin) {
        set_error("deconv %s: unsupported shape (k=%d, Cin %d vs %d)", scope.c_str(), pc.kh, pc.cin, in[0].C);
        throw ArgError();
    }
    TL out;
    for (size_t i = 0; i < in.size(); ++i) {
        if (cdiv(like[i].H, 2) != in[i].H || cdiv(like[i].W, 2) != in[i].W) {
            set_error("deconv %s: output %dx%d incompatible with input %dx%d", scope.c_str(), like[i].H, like[i].W, in[i].H, in[i].W);
            throw ArgError();
        }
        out.push_back(new_tensor(m, like[i].H, like[i].W, pc.cout));
    }
    const int mt = pc.mtiles % 2 == 0 ? 2 : 1;
    const bool valu = pc.d_wv && m->r8_valu;                 // level 0: one input position per thread on the vector ALU
#ifndef DS_ROWS
#define DS_ROWS 8                  // input rows per block of deconvs_kernel (16: 280 / 310 / 477 us against 260 / 312 / 440)
#endif
    const bool splitd = m->split && m->use_deconvs && pc.d_ws && pc.smode == 2 && !valu;   // >= 32 input channels: split products (deconvs_kernel)
    const int tw = valu ? DCV_T : DC_TW, th = valu ? DCV_T : (splitd ? DS_ROWS : DC_TH);
    for_chunks<ConvArgs>(in.size(), 9.0 * pc.cin * pc.cout * 4.0, [&](ConvProb& p, size_t i, Chunk& k) {
        p.in0 = in[i].p; p.in1 = nullptr; p.res = nullptr; p.out = out[i].p;
        p.H = in[i].H; p.W = in[i].W; p.Ho = out[i].H; p.Wo = out[i].W;
        p.pbh = std::max((in[i].H - 1) * 2 + 3 - out[i].H, 0) / 2;
        p.pbw = std::max((in[i].W - 1) * 2 + 3 - out[i].W, 0) / 2;
        set_tiles(p, k.units.next_tiles(p.H, p.W, tw, th));
        k.flops += 2.0 * in[i].H * in[i].W * 9.0 * pc.cin * pc.cout;
        k.bytes += tbytes(in[i]) + tbytes(out[i]);
    }, [&](ConvArgs& a, const Chunk& k) {
        a.c0 = in[0].C; a.c1 = 0;
        a.wpk = (const f32x4*)pc.d_w; a.bias = pc.d_b;
        a.cout = pc.cout; a.mtiles = pc.mtiles; a.groups = pc.groups;
        a.relu_in = 0; a.relu_out = relu_out; a.act = act;
        int units;
        a.xm = oneshot_map(m, k.units.total, &units);
        dim3 grid(units, pc.mtiles / mt);
        const std::string dname = valu ? std::string("deconv8v_kernel") : (splitd ? "deconvs_kernel" + targs({ti(mt), ti(DS_ROWS)}) : "deconv_mfma_kernel" + targs({ti(mt), tb(false)}));
        ProfScope ps(m, dname, k.flops, layer_text(scope, k.sub(in), pc.cin, pc.cout));
        ps.bytes = k.bytes;
        if (valu) {
            a.wpk = (const f32x4*)pc.d_wv;
            hipLaunchKernelGGL(deconv8v_kernel, dim3(units), dim3(256), 0, m->stream, a);
        } else if (splitd) {
            a.wpk = (const f32x4*)pc.d_ws; a.groups = pc.cin / 32;
            if (mt == 2) hipLaunchKernelGGL((deconvs_kernel<2, DS_ROWS>), grid, dim3(256), 0, m->stream, a);
            else hipLaunchKernelGGL((deconvs_kernel<1, DS_ROWS>), grid, dim3(256), 0, m->stream, a);
        } else if (mt == 2) hipLaunchKernelGGL((deconv_mfma_kernel<2>), grid, dim3(256), 0, m->stream, a);
        else hipLaunchKernelGGL((deconv_mfma_kernel<1>), grid, dim3(256), 0, m->stream, a);
    });
    return out;
}

// launches conv_c3_kernel<cout, bf> (defined at the end of this file)
void launch_conv_c3(asep_aru* m, const C1Args& a, int cout, bool bf, int tiles);

// first layer (Cin == 1, or the interleaved 3-channel page of a colour net); stats[i] = per-problem {mean, 1/std} pointer or nullptr.
// bf16 engine: fp32 image -> bf16 [H,W,8] (pre-ReLU t of unet_down_0, or the activated conv1 of graph 'U')
TL run_direct(asep_aru* m, const DirectConv& dc, const TL& imgs, bool relu, const std::vector<const float*>& stats, int act = 0) {
    const bool bf = m->bf16, rgb = dc.cin == 3;              // colour net: conv_c3_kernel
    if (bf && (dc.k != 3 || dc.cout != 8 || (dc.cin != 1 && !rgb))) {    // (the bf16 engine is a feat_root 8 engine: combine_kernel)
        set_error("bf16 path: first-layer conv k=%d cin=%d cout=%d not instantiated", dc.k, dc.cin, dc.cout);
        throw ArgError();
    }
    TL out;
    for (const Tensor& t : imgs) out.push_back(new_tensor(m, t.H, t.W, dc.cout, bf));
    for_chunks<C1Args>(imgs.size(), 0.0, [&](C1Prob& p, size_t i, Chunk& k) {
        p.img = imgs[i].p; p.out = out[i].p; p.stats = stats.empty() ? nullptr : stats[i];
        p.H = imgs[i].H; p.W = imgs[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, 64, 4));
        k.flops += 2.0 * imgs[i].H * imgs[i].W * dc.k * dc.k * dc.cin * dc.cout;
        k.bytes += tbytes(imgs[i]) + tbytes(out[i]);
    }, [&](C1Args& a, const Chunk& k) {
        a.w = dc.d_w; a.bias = dc.d_b; a.relu = relu ? 1 : 0; a.act = act;
        ProfScope ps(m, rgb ? "conv_c3_kernel<" + std::to_string(dc.cout) + "," + tb(bf) + ">"
                            : "conv_c1_kernel<" + std::to_string(dc.k) + "," + std::to_string(dc.cout) + (bf ? ",true>" : ">"), k.flops);
        ps.bytes = k.bytes;
        const int tiles = k.units.total;
        dim3 grid(tiles);
        if (rgb && dc.k == 3 && (dc.cout == 8 || (dc.cout == 16 && !bf))) launch_conv_c3(m, a, dc.cout, bf, tiles);
        else if (dc.cin != 1) { set_error("first-layer conv k=%d cin=%d cout=%d not instantiated", dc.k, dc.cin, dc.cout); throw ArgError(); }
        else if (bf) hipLaunchKernelGGL((conv_c1_kernel<3, 8, true>), grid, dim3(256), 0, m->stream, a);
        else if (dc.k == 3 && dc.cout == 8) hipLaunchKernelGGL((conv_c1_kernel<3, 8>), grid, dim3(256), 0, m->stream, a);
        else if (dc.k == 3 && dc.cout == 16) hipLaunchKernelGGL((conv_c1_kernel<3, 16>), grid, dim3(256), 0, m->stream, a);
        else if (dc.k == 3 && dc.cout == 12) launch_conv_c1_12(m, a, tiles);
        else if (dc.k == 4 && dc.cout == 12) hipLaunchKernelGGL((conv_c1_kernel<4, 12>), grid, dim3(256), 0, m->stream, a);
        else { set_error("first-layer conv k=%d cout=%d not instantiated", dc.k, dc.cout); throw ArgError(); }
    });
    return out;
}

// The streaming passes (pools, channel sums, act_kernel): one launch of 256-thread blocks per chunk, every problem a range of blocks of
// `per_block` items over the tensors `l`.  fill(p, i, k) sets problem i's pointers and dims, adds its bytes to k and returns its items;
// launch(a, grid) launches.
template <class Args, class Fill, class Launch>
void stream_pass(asep_aru* m, const TL& l, const char* name, size_t per_block, Fill fill, Launch launch) {
    for_chunks<Args>(l.size(), 0.0, [&](auto& p, size_t i, Chunk& k) {
        const size_t items = fill(p, i, k);
        p.blk_begin = k.units.next_blocks(items, per_block).begin;
    }, [&](Args& a, const Chunk& k) {
        a.C = l[0].C;
        ProfScope ps(m, name, 0.0);
        ps.bytes = k.bytes;
        launch(a, dim3(k.units.total));
    });
}

TL run_pool(asep_aru* m, const TL& in, PoolKind kind) {
    TL out;
    for (const Tensor& t : in) {
        if (kind == POOL_CHANSUM) out.push_back(new_tensor(m, t.H, t.W, 1));
        else out.push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), t.C));
    }
    stream_pass<PoolArgs>(m, in, kind == POOL_MAX ? "maxpool2_kernel" : (kind == POOL_AVG_C1 ? "avgpool2_c1_kernel" : (kind == POOL_AVG_C3 ? "avgpool2_cn_kernel<3>" : "chansum_kernel")), POOL_ITEMS,
        [&](PoolProb& p, size_t i, Chunk& k) {
            k.bytes += tbytes(in[i]) + tbytes(out[i]);
            p.in = in[i].p; p.out = out[i].p; p.H = in[i].H; p.W = in[i].W; p.Ho = out[i].H; p.Wo = out[i].W;
            return kind == POOL_MAX ? out[i].count() / 4 : (size_t)out[i].H * out[i].W;
        }, [&](const PoolArgs& a, dim3 grid) {
            if (kind == POOL_MAX) hipLaunchKernelGGL(maxpool2_kernel, grid, dim3(256), 0, m->stream, a);
            else if (kind == POOL_AVG_C1) hipLaunchKernelGGL(avgpool2_c1_kernel, grid, dim3(256), 0, m->stream, a);
            else if (kind == POOL_AVG_C3) launch_avgpool_c3(m, a, grid);
            else hipLaunchKernelGGL(chansum_kernel, grid, dim3(256), 0, m->stream, a);
        });
    return out;
}

int grid_1d(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 256 * 8); }

// the profiler's layer text of a level-0 block over the pages `l`
std::string res8_what(bool up, const TL& l) {
    return (up ? "unet_up_0 (conv1[16->8]+3xconvR+add) " : "unet_down_0 (conv1+3xconvR+add+pool) ") + dims_of(l);
}

// the vector-ALU level-0 kernels address their tensors with 32-bit element offsets: below 2^28 pixels per tensor (2^31 elements at 8 channels)
bool r8v_fits(const TL& l) {
    for (const Tensor& t : l)
        if ((size_t)t.H * t.W >= ((size_t)1 << 28)) return false;
    return true;
}

// f32s level 0 on the split-product strip walkers (res8ws_kernels.h): pages with room for the walker's region (level0_plan.h), ReLU graph only
bool r8ws_fits(const Tensor& t) { return walk_region(t.H, t.W).fits; }
bool r8ws_on(asep_aru* m) { return m->split && m->use_split_walk && m->r8_valu && m->cfg.activation == 0 && m->d_r8ws_down_w; }
// the work units of a res8v launch over `a` (unit height R8_OH * R8_NP) that the strip walkers do not cover: for a page in `walk`, the units
// that touch the frame around its walker region (level0_plan.h), for the other pages all units.  Cached device list; nullptr on failure.
const int32_t* r8ws_frame_units(asep_aru* m, const Res8Args& a, const std::vector<bool>& walk, int* count) {
    std::string key = "f";
    for (int i = 0; i < a.nprob; ++i) key += ":" + std::to_string(a.p[i].H) + "x" + std::to_string(a.p[i].W) + (walk[i] ? "w" : "t");
    std::vector<int32_t> units;
    for (int i = 0; i < a.nprob; ++i) frame_units(a.p[i].H, a.p[i].W, a.p[i].tiles_x, a.p[i].tile_begin, walk[i], R8_OW, R8_OH * R8_NP, &units);
    *count = (int)units.size();
    auto it = m->sched_cache.find(key);
    if (it != m->sched_cache.end()) return it->second;
    if (units.empty()) return nullptr;
    const int32_t* d = put_table(m, units);
    if (d) m->sched_cache[key] = d;
    return d;
}

// the walker launch for the pages of a (a.p[i] for walk[i]); the frame units must have been launched before it on the same stream
void run_res8ws(asep_aru* m, bool up, const Res8Args& a, const std::vector<bool>& walk, const std::string& what) {
    Res8WSArgs wa{};
    int n = 0, items = 0;
    double flops = 0, bytes = 0;
    long strip_rows = 0;
    for (int i = 0; i < a.nprob; ++i) {
        if (!walk[i]) continue;
        const Res8Prob& q = a.p[i];
        Res8WSProb& p = wa.p[n++];
        if (up) { p.skip = q.img; p.dec = q.in1; }
        else { p.img = q.img; p.stats = q.stats; p.pool = q.pool; }
        p.out = q.out;
        p.H = q.H; p.W = q.W;
        const WalkRegion r = walk_region(p.H, p.W);
        p.n_strips = r.n_strips;
        p.y_end = r.y_end;
        strip_rows += (long)r.n_strips * r.rows();
        flops += 2.0 * r.pixels() * (9.0 * (up ? 16 : 1) * 8 + 3 * 9.0 * 64);
        bytes += r.pixels() * ((up ? 64.0 : 4.0) + 32.0 + (p.pool ? 8.0 : 0.0));
    }
    if (!n) return;
    const int band = walk_band(strip_rows, m->num_cus, up ? R8WS_UP_WAVES_PER_CU : R8WS_DOWN_WAVES_PER_CU);
    for (int i = 0; i < n; ++i) {
        Res8WSProb& p = wa.p[i];
        p.band = band;
        p.tile_begin = items;
        items += walk_region(p.H, p.W).items(band);
    }
    wa.nprob = n;
    if (up) { wa.b1 = m->d_r8_up_b1; wa.w1s = (const u32x4*)m->d_r8ws_up_w1; wa.ws = (const u32x4*)m->d_r8ws_up_w; wa.bias = m->d_r8_up_br; }
    else { wa.b1 = m->det_first.d_b; wa.w1f = m->det_first.d_w; wa.ws = (const u32x4*)m->d_r8ws_down_w; wa.bias = m->d_r8_down_br; }
    int units = items;
    wa.xm = oneshot_map(m, items, &units);
    ProfScope ps(m, up ? "res8ws_kernel<true>" : "res8ws_kernel<false>", flops, what);
    ps.bytes = bytes;
    if (up) hipLaunchKernelGGL(res8ws_kernel<true>, dim3(units), dim3(64), 0, m->stream, wa);
    else hipLaunchKernelGGL(res8ws_kernel<false>, dim3(units), dim3(64), 0, m->stream, wa);
}

// the kernel of a fused fp32 level-0 block with rocprofv3's name for it (template arguments spelled out): the vector-ALU form with the graph's
// activation (0 ReLU, 1 elu, 2 leaky), or the MFMA form (ReLU only)
struct Res8Kernel { void (*fn)(const Res8Args); const char* name; };
Res8Kernel res8_kernel(bool up, bool valu, int actv) {
    static const Res8Kernel k[2][4] = {
        {{res8v_down_kernel<0>, "res8v_down_kernel<0>"}, {res8v_down_kernel<1>, "res8v_down_kernel<1>"}, {res8v_down_kernel<2>, "res8v_down_kernel<2>"},
         {res8_down_kernel<false>, "res8_down_kernel<false>"}},
        {{res8v_up_kernel<0>, "res8v_up_kernel<0>"}, {res8v_up_kernel<1>, "res8v_up_kernel<1>"}, {res8v_up_kernel<2>, "res8v_up_kernel<2>"},
         {res8_up_kernel<false>, "res8_up_kernel<false>"}}};
    return k[up][valu ? actv : 3];
}

// fused fp32 level-0 block.  down: images in0 -> d0 (and maxpool2(d0) if want_pool); up: [skip in0, deconv *in1] -> block output
void run_res8(asep_aru* m, bool up, const TL& in0, const TL* in1, const std::vector<const float*>& stats, bool want_pool, TL* d_out, TL* pool_out) {
    for (const Tensor& t : in0) {
        d_out->push_back(new_tensor(m, t.H, t.W, 8));
        if (want_pool) pool_out->push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), 8));
    }
    const size_t lds = up ? R8_UP_LDS : R8_DOWN_LDS;
    const char* layer = up ? "unet_up_0" : "unet_down_0";
    for_chunks<Res8Args>(in0.size(), 0.0, [&](Res8Prob& p, size_t i, Chunk& k) {
        k.bytes += tbytes(in0[i]) + (up ? tbytes((*in1)[i]) : 0.0) + tbytes((*d_out)[i]) + (want_pool ? tbytes((*pool_out)[i]) : 0.0);
        p.img = in0[i].p; p.in1 = up ? (*in1)[i].p : nullptr; p.stats = stats.empty() ? nullptr : stats[i];
        p.out = (*d_out)[i].p; p.pool = want_pool ? (*pool_out)[i].p : nullptr;
        p.H = in0[i].H; p.W = in0[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, R8_OW, R8_OH * R8_NP));
        k.flops += 2.0 * in0[i].H * in0[i].W * (9.0 * (up ? 16 : 1) * 8 + 3 * 9.0 * 64);
    }, [&](Res8Args& a, const Chunk& c) {
        const int tiles = c.units.total;
        const double flops = c.flops, bytes = c.bytes;
        const TL sub = c.sub(in0);
        const bool valu = m->r8_valu && r8v_fits(sub);       // vector-ALU kernels, with weights in their own order
        if (up) { a.w1 = valu ? m->d_r8v_up_w1 : m->d_r8_up_w1; a.b1 = m->d_r8_up_b1; }
        else { a.w1 = m->det_first.d_w; a.b1 = m->det_first.d_b; }
        a.wr = (const f32x4*)(up ? (valu ? m->d_r8v_up_wr : m->d_r8_up_wr) : (valu ? m->d_r8v_down_wr : m->d_r8_down_wr));
        a.br = up ? m->d_r8_up_br : m->d_r8_down_br;
        const int actv = m->cfg.activation;                  // graph variants (fused8_var): the same block with elu / leaky (vector-ALU form only)
        const Res8Kernel k = res8_kernel(up, valu, actv);
        a.sched = tile_schedule(m, a, std::min(tiles, m->num_cus), R8_OH * R8_NP);
        if (valu && r8ws_on(m) && (!up || m->d_r8ws_up_w1)) {
            // the frame units on the res8v kernel, then the split-product walkers over the rest of the pages that have room for them
            std::vector<bool> walk(a.nprob);
            bool any = false;
            for (int i = 0; i < a.nprob; ++i) { walk[i] = r8ws_fits(sub[i]); any = any || walk[i]; }
            if (any) {
                int nu = 0;
                Res8Args f = a;
                f.sched = r8ws_frame_units(m, a, walk, &nu);
                if (!f.sched) { set_error("level-0 frame schedule: device allocation failed"); throw ArgError(); }
                f.total_tiles = nu;
                {
                    const double share = (double)nu / tiles;          // (the frame units' share of the launch's work units)
                    ProfScope ps(m, k.name, flops * share, std::string(layer) + " frame " + dims_of(sub));
                    ps.bytes = bytes * share;
                    hipLaunchKernelGGL(k.fn, dim3(std::min(nu, m->num_cus)), dim3(R8_THREADS), lds, m->stream, f);
                }
                run_res8ws(m, up, a, walk, res8_what(up, sub));
                return;
            }
        }
        ProfScope ps(m, k.name, flops, res8_what(up, sub));
        ps.bytes = bytes;
        if (actv && !valu) { set_error("level-0 block of an elu / leaky graph: image too large for the vector-ALU kernel"); throw ArgError(); }
        hipLaunchKernelGGL(k.fn, dim3(std::min(tiles, m->num_cus)), dim3(R8_THREADS), lds, m->stream, a);
    });
}

// ================================================================================================
// Native bf16 data path (cfg.compute_dtype == 1): launchers of bf16_kernels.h
// ================================================================================================
void run_res8b_tiles(asep_aru* m, bool up, const TL& a0, const TL* a1, const std::vector<const float*>& stats, bool want_pool, const TL& outs, const TL* pool_out);

// whole level-0 blocks of the bf16 path (res8b_kernel)
// A level-0 block (up: [skip, deconv] in; down: the fp32 image in, pool out) of the pages the strip walker serves (res8w_kernels.h): one launch of
// walker items (one wave each) + one launch of the border tiles around the walkers' regions.  `outs` / `pools` are the pages' output tensors.
void run_res8w(asep_aru* m, bool up, const TL& in0, const TL* dec, const std::vector<const float*>& stats, const TL& outs, const TL* pools) {
    for (size_t c = 0; c < num_chunks(in0.size()); ++c) {      // (two argument structs, a band rule over the whole launch: not on for_chunks)
        const size_t b0 = chunk_begin(c), b1 = chunk_end(in0.size(), c);
        Res8WArgs wa{};
        Res8WBArgs ba{};
        double flops = 0, bytes = 0, wshare = 0;
        long strip_rows = 0;
        for (size_t i = b0; i < b1; ++i) {
            Res8WProb& p = wa.p[i - b0];
            if (up) { p.skip = in0[i].bp(); p.dec = (*dec)[i].bp(); }
            else { p.img = in0[i].p; p.stats = stats.empty() ? nullptr : stats[i]; p.pool = pools ? (*pools)[i].bp() : nullptr; }
            p.out = outs[i].bp();
            p.H = in0[i].H; p.W = in0[i].W;
            const WalkRegion r = walk_region(p.H, p.W);
            p.n_strips = r.n_strips;
            p.y_end = r.y_end;
            strip_rows += (long)r.n_strips * r.rows();
            bytes += tbytes(in0[i]) + (up ? tbytes((*dec)[i]) : 0.0) + tbytes(outs[i]) + (pools ? tbytes((*pools)[i]) : 0.0);
            flops += 2.0 * p.H * p.W * (9.0 * (up ? 16 : 1) * 8 + 3 * 9.0 * 64);
            wshare += r.pixels();
        }
        // rows of an item (eight waves per CU): an item's head and tail cost about fifteen iterations of the general form (profiles/r6_walk:
        // 64 / 128 / 256 / 400 / 800 rows per item = 952 / 798 / 747 / 752 / 739 us per 4-page launch)
        int band = walk_band(strip_rows, m->num_cus, 8);
#ifdef ASEP_ABLATION
        if (const char* e = getenv("ASEP_BF_WALK_BAND")) band = std::max(2, atoi(e) & ~1);      // (measurement knob of ablation builds)
#endif
        int items = 0, btiles = 0;
        for (size_t i = b0; i < b1; ++i) {
            Res8WProb& p = wa.p[i - b0];
            p.band = band;
            p.tile_begin = items;
            items += walk_region(p.H, p.W).items(band);
            Res8BProb& q = ba.b.p[i - b0];
            q.skip = p.skip; q.dec = p.dec; q.img = p.img; q.stats = p.stats; q.out = p.out; q.pool = p.pool; q.H = p.H; q.W = p.W;
            q.tile_begin = btiles;
            const BorderPlan bp = border_plan(p.H, p.W);
            ba.nbx[i - b0] = bp.nbx; ba.nby[i - b0] = bp.nby;
            ba.y_end[i - b0] = bp.y_end; ba.xr[i - b0] = bp.xr;
            btiles += bp.tiles();
        }
        wa.nprob = ba.b.nprob = (int)(b1 - b0);
        if (up) {
            wa.b1 = m->d_r8b_up_b1; wa.w1pf = (const u32x4*)m->d_r8f_up_w1; wa.wpk = (const u32x4*)m->d_r8b_up_w; wa.bias = m->d_r8b_up_b;
            ba.b.w1pk = (const u32x4*)m->d_r8b_up_w1; ba.b.b1 = m->d_r8b_up_b1; ba.b.wpk = (const u32x4*)m->d_r8b_up_w; ba.b.bias = m->d_r8b_up_b;
        } else {
            wa.b1 = m->det_first.d_b; wa.w1pf = (const u32x4*)m->d_r8f_down_w1; wa.wpk = (const u32x4*)m->d_r8b_down_w; wa.bias = m->d_r8b_down_b;
            ba.b.w1 = m->d_r8b_down_w1r ? m->d_r8b_down_w1r : m->det_first.d_w; ba.b.b1 = m->det_first.d_b; ba.b.wpk = (const u32x4*)m->d_r8b_down_w; ba.b.bias = m->d_r8b_down_b;
        }
        TL sub(in0.begin() + b0, in0.begin() + b1);
        const std::string what = res8_what(up, sub);
        double area = 0;
        for (size_t i = b0; i < b1; ++i) area += (double)in0[i].H * in0[i].W;
        const double wf = wshare / area;                     // the walker's share of the pages' pixels
        int units = items;
        wa.xm = oneshot_map(m, items, &units);
        // the border tiles (4 % of the pixels in 256-thread blocks) run BESIDE the walkers on a stream of their own: they fill the walkers' tail.
        // While launch times are recorded everything stays on one stream.
        asep_aru::Lane& L = *m->cur;
        const bool beside = !m->profiling && L.bside;
        if (beside) {
            ASEP_HIP_CHECK_THROW(hipEventRecord(L.ev_bfork, m->stream));
            ASEP_HIP_CHECK_THROW(hipStreamWaitEvent(L.bside, L.ev_bfork, 0));
        }
        {
            ProfScope ps(m, up ? "res8w_kernel<true>" : "res8w_kernel<false>", flops * wf, what);
            ps.bytes = bytes * wf;
            if (up) hipLaunchKernelGGL(res8w_kernel<true>, dim3(units), dim3(64), 0, m->stream, wa);
            else hipLaunchKernelGGL(res8w_kernel<false>, dim3(units), dim3(64), 0, m->stream, wa);
        }
        {
            ProfScope ps(m, up ? "res8wb_kernel<true>" : "res8wb_kernel<false>", flops * (1.0 - wf), what);
            ps.bytes = bytes * (1.0 - wf);
            if (up) hipLaunchKernelGGL(res8wb_kernel<true>, dim3(btiles), dim3(256), 0, beside ? L.bside : m->stream, ba);
            else hipLaunchKernelGGL(res8wb_kernel<false>, dim3(btiles), dim3(256), 0, beside ? L.bside : m->stream, ba);
        }
        if (beside) {
            ASEP_HIP_CHECK_THROW(hipEventRecord(L.ev_bjoin, L.bside));
            ASEP_HIP_CHECK_THROW(hipStreamWaitEvent(m->stream, L.ev_bjoin, 0));
        }
    }
}

void run_res8b(asep_aru* m, bool up, const TL& a0, const TL* a1, const std::vector<const float*>& stats, bool want_pool, TL* d_out, TL* pool_out) {
    for (const Tensor& t : a0) {
        d_out->push_back(new_tensor(m, t.H, t.W, 8, true));
        if (want_pool) pool_out->push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), 8, true));
    }
    if (!m->fused_act && m->use_walk && (up || m->walk_mode == 1) && (up ? m->d_r8f_up_w1 != nullptr : m->d_r8f_down_w1 != nullptr)) {
        // pages with room for at least four strips and two tile rows of walker region go to the strip walker, the others stay on the tile kernels
        TL ws, wd, wo, wp, rs, rd, ro, rp;
        std::vector<const float*> wst, rst;
        for (size_t i = 0; i < a0.size(); ++i) {
            const Tensor& t = a0[i];
            const bool fits = walk_region(t.H, t.W).fits;
            (fits ? ws : rs).push_back(t);
            if (up) (fits ? wd : rd).push_back((*a1)[i]);
            (fits ? wo : ro).push_back((*d_out)[i]);
            if (want_pool) (fits ? wp : rp).push_back((*pool_out)[i]);
            if (!stats.empty()) (fits ? wst : rst).push_back(stats[i]);
        }
        if (!ws.empty()) {
            run_res8w(m, up, ws, up ? &wd : nullptr, wst, wo, want_pool ? &wp : nullptr);
            if (!rs.empty()) run_res8b_tiles(m, up, rs, up ? &rd : nullptr, rst, want_pool, ro, want_pool ? &rp : nullptr);
            return;
        }
    }
    run_res8b_tiles(m, up, a0, a1, stats, want_pool, *d_out, pool_out);
}

// the tile kernels (res8f_kernel for interior tiles + res8b_tile for border tiles in one launch) on the given output tensors
void run_res8b_tiles(asep_aru* m, bool up, const TL& a0, const TL* a1, const std::vector<const float*>& stats, bool want_pool, const TL& outs, const TL* pool_out) {
    struct K { void (*fn)(const Res8BArgs); const char* name; };
    static const K general[2][3] = {{{res8b_kernel<false>, "res8b_kernel<false,0>"}, {res8b_kernel<false, 1>, "res8b_kernel<false,1>"}, {res8b_kernel<false, 2>, "res8b_kernel<false,2>"}},
                                    {{res8b_kernel<true>, "res8b_kernel<true,0>"}, {res8b_kernel<true, 1>, "res8b_kernel<true,1>"}, {res8b_kernel<true, 2>, "res8b_kernel<true,2>"}}};
    static const K lean[2] = {{res8f_kernel<false>, "res8f_kernel<false>"}, {res8f_kernel<true>, "res8f_kernel<true>"}};
    for_chunks<Res8BArgs>(a0.size(), 0.0, [&](Res8BProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(a0[i]) + (up ? tbytes((*a1)[i]) : 0.0) + tbytes(outs[i]) + (want_pool ? tbytes((*pool_out)[i]) : 0.0);
        if (up) { p.skip = a0[i].bp(); p.dec = (*a1)[i].bp(); }
        else { p.img = a0[i].p; p.stats = stats.empty() ? nullptr : stats[i]; }
        p.out = outs[i].bp(); p.pool = want_pool ? (*pool_out)[i].bp() : nullptr;
        p.H = a0[i].H; p.W = a0[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, 32, 16));
        k.flops += 2.0 * a0[i].H * a0[i].W * (9.0 * (up ? 16 : 1) * 8 + 3 * 9.0 * 64);
    }, [&](Res8BArgs& a, const Chunk& k) {
        if (up) { a.w1pk = (const u32x4*)m->d_r8b_up_w1; a.b1 = m->d_r8b_up_b1; a.wpk = (const u32x4*)m->d_r8b_up_w; a.bias = m->d_r8b_up_b; }
        else { a.w1 = m->d_r8b_down_w1r ? m->d_r8b_down_w1r : m->det_first.d_w; a.b1 = m->det_first.d_b; a.wpk = (const u32x4*)m->d_r8b_down_w; a.bias = m->d_r8b_down_b; }
        const TL sub = k.sub(a0);
        int units;
        a.xm = oneshot_map(m, k.units.total, &units);
        bool small = true;                                   // res8f_kernel addresses its tensors with 32-bit byte offsets (16 bytes per pixel)
        for (const Tensor& t : sub) small = small && (size_t)t.H * t.W < ((size_t)1 << 28);
        // elu / leaky: the general form for every tile; else the lean form for interior tiles (their 24 x 40 input window inside the image) and
        // the general form for border tiles in one launch; else the general form
        const bool f = !m->fused_act && small && (up || m->d_r8f_down_w1);
        if (f && !up) a.w1pk = (const u32x4*)m->d_r8f_down_w1;
        if (f && up) a.w1pf = (const u32x4*)m->d_r8f_up_w1;
        const K& kn = f ? lean[up] : general[up][m->fused_act];
        ProfScope ps(m, kn.name, k.flops, res8_what(up, sub));
        ps.bytes = k.bytes;
        hipLaunchKernelGGL(kn.fn, dim3(units), dim3(256), 0, m->stream, a);
    });
}

#define ASEP_CONVB_LAUNCH(KH_, KW_, MODE_, MT_, WM_, TH_, MB_)                                                         \
    do {                                                                                                               \
        ps.set_name("convb_kernel" + targs({ti(KH_), ti(KW_), ti(MODE_), ti(MT_), ti(WM_), ti(TH_), ti(MB_), tb(false), ti(4)})); \
        hipLaunchKernelGGL((convb_kernel<KH_, KW_, MODE_, MT_, WM_, TH_, MB_, false, 4>), grid, dim3(256), 0, m->stream, a); \
    } while (0)
#define ASEP_CONVB_LAUNCH8(KH_, KW_, MODE_, MT_, WM_, TH_, MB_, RES_)                                                  \
    do {                                                                                                               \
        ps.set_name("convb_kernel" + targs({ti(KH_), ti(KW_), ti(MODE_), ti(MT_), ti(WM_), ti(TH_), ti(MB_), tb(RES_), ti(8)})); \
        hipLaunchKernelGGL((convb_kernel<KH_, KW_, MODE_, MT_, WM_, TH_, MB_, RES_, 8>), grid, dim3(512), 0, m->stream, a); \
    } while (0)
#define ASEP_CONVB_LAUNCH_RES(KH_, KW_, MODE_, MT_, WM_, TH_, MB_)                                                     \
    do {                                                                                                               \
        ps.set_name("convb_kernel" + targs({ti(KH_), ti(KW_), ti(MODE_), ti(MT_), ti(WM_), ti(TH_), ti(MB_), tb(true), ti(4)})); \
        hipLaunchKernelGGL((convb_kernel<KH_, KW_, MODE_, MT_, WM_, TH_, MB_, true, 4>), grid, dim3(256), 0, m->stream, a); \
    } while (0)

// maxpool2 of a ReLU layer's bf16 output (behind convr_kernel's RES form)
TL run_maxpool2b(asep_aru* m, const TL& in) {
    TL out;
    for (const Tensor& t : in) out.push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), t.C, true));
    stream_pass<MaxPoolBArgs>(m, in, "maxpool2b_kernel", 256, [&](MaxPoolBProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(in[i]) + tbytes(out[i]);
        p.in = in[i].bp(); p.out = out[i].bp(); p.H = in[i].H; p.W = in[i].W;
        return out[i].count() / 8;
    }, [&](const MaxPoolBArgs& a, dim3 grid) { hipLaunchKernelGGL(maxpool2b_kernel, grid, dim3(256), 0, m->stream, a); });
    return out;
}

// the 64 -> 64 3x3 layers with the filter in registers (convr_kernels.h): one wave per SIMD, a wave = the pipeline of a 32-column strip
TL run_convr(asep_aru* m, const std::string& scope, const PackedConv& pc, const TL& in0, bool relu_in, bool relu_out, const TL* res) {
    TL out;
    for (const Tensor& t : in0) out.push_back(new_tensor(m, t.H, t.W, 64, true));
    // the instantiations by (relu_in, relu_out) of the 64-channel form without residual
    struct K { void (*fn)(const ConvRArgs); };
    static const K plain[2][2] = {{{convr_kernel<false, false>}, {convr_kernel<false, true>}}, {{convr_kernel<true, false>}, {convr_kernel<true, true>}}};
    const int cin = in0[0].C;
    for_chunks<ConvRArgs>(in0.size(), 9.0 * cin * 64 * 2.0, [&](ConvRProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(in0[i]) + tbytes(out[i]) + (res ? tbytes((*res)[i]) : 0.0);
        p.in = in0[i].bp(); p.res = res ? (*res)[i].bp() : nullptr; p.out = out[i].bp();
        p.H = in0[i].H; p.W = in0[i].W;
        const Units u = k.units.next_strips(p.H, p.W, 32);
        p.strips = u.per_row; p.begin = u.begin;
        k.flops += 2.0 * in0[i].H * in0[i].W * 9.0 * cin * 64.0;
    }, [&](ConvRArgs& a, const Chunk& k) {
        a.wpk = (const u32x4*)pc.d_wb; a.bias = pc.d_b;
        a.zero = m->d_zero_trash;
        // one wave per SIMD; a wave's range = total / waves rows (never fewer than 8: a range starts with three rows of latency)
        const int blocks = std::max(1, std::min(m->num_cus, k.units.total / 32));
        ProfScope ps(m, "convr_kernel" + targs({tb(relu_in), tb(relu_out), tb(res != nullptr), ti(cin)}), k.flops, layer_text(scope, k.sub(in0), cin, 64));
        ps.bytes = k.bytes;
        void (*fn)(const ConvRArgs) = cin == 32 ? convr_kernel<false, false, false, 32> : res ? convr_kernel<false, true, true> : plain[relu_in][relu_out].fn;
        hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, m->stream, a);
    });
    return out;
}

// stride-1 SAME conv of the bf16 path.  pooled != nullptr: the epilogue also writes maxpool2 of the output (always fused here);
// keep_full = false: only the pooled tensor is stored; pool_f32: the pooled tensor is fp32 (input of conv_c1out_kernel)
// relu_out = true on an elu / leaky graph (cfg.activation != 0): the layer's activation is that function (ConvBArgs::act), applied to the
// fp32 sums before the rounding; relu_out = false: identity (block-opening conv1)
TL run_convb(asep_aru* m, const std::string& scope, const TL& in0, const TL* in1, bool relu_in, bool relu_out, const TL* res,
             TL* pooled = nullptr, bool keep_full = true, bool pool_f32 = false) {
    const int act = relu_out ? m->cfg.activation : 0;
    if (act) relu_out = false;
    auto it = m->convs.find(scope);
    if (it == m->convs.end()) { set_error("internal: conv %s not packed", scope.c_str()); throw ArgError(); }
    const PackedConv& pc = it->second;
    const int cin = in0[0].C + (in1 ? (*in1)[0].C : 0);
    const int cin_w = pc.cin == 12 ? 16 : pc.cin;           // attention conv2 reads the head's zero-padded 16-channel plane
    if (cin != cin_w || !in0[0].bf) { set_error("internal: conv %s expects %d bf16 channels, got %d", scope.c_str(), cin_w, cin); throw ArgError(); }
    if (pc.bmode < 0 || !pc.d_wb || !((pc.kh == 3 && pc.kw == 3) || (pc.kh == 4 && pc.kw == 4)) || in0[0].C % 8 != 0 || pc.cout % 8 != 0) {
        set_error("conv %s (%dx%d, %d -> %d channels) is not served by the bf16 kernels", scope.c_str(), pc.kh, pc.kw, pc.cin, pc.cout);
        throw ArgError();
    }
    // output-channel tiles per block: 1 (cout 8 / 16), 2 (cout 32: one wave row, 16 x 32 pixels), 4 (cout >= 64: two wave
    // rows of two m-tiles, 8 x 32 pixels)
    if (m->use_convr && pc.kh == 3 && pc.kw == 3 && pc.bmode == 2 && !in1 && pc.cout == 64 && pc.mtiles == 4 && !act &&
        ((in0[0].C == 64 && (!res || (!relu_in && relu_out)) && (!pooled || (relu_out && keep_full && !pool_f32))) ||
         (in0[0].C == 32 && !res && !pooled && !relu_in && !relu_out))) {
        TL out = run_convr(m, scope, pc, in0, relu_in, relu_out, res);
        // (the block-closing layer of unet_down_3 also pools: convr_kernel has no fused pool; a ReLU output's 2 x 2 maxima are taken from the stored
        // tensor -- the same values convb_kernel's epilogue compares -- by a streaming kernel: 100 + 41 us against 160)
        if (pooled) *pooled = run_maxpool2b(m, out);
        return out;
    }
    const int mtb = pc.mtiles >= 4 ? 4 : pc.mtiles;
    if (pc.mtiles % mtb != 0 || mtb == 3) { set_error("conv %s: %d output tiles not instantiated", scope.c_str(), pc.mtiles); throw ArgError(); }
    const int th = (mtb == 4 || (mtb == 2 && pc.bmode == 2)) ? 8 : 16;
    TL out;
    if (keep_full || !pooled)
        for (const Tensor& t : in0) out.push_back(new_tensor(m, t.H, t.W, pc.cout, true));
    if (pooled) {
        pooled->clear();
        for (const Tensor& t : in0) {
            pooled->push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), pc.cout, !pool_f32));
        }
    }
    for_chunks<ConvBArgs>(in0.size(), conv_wbytes(pc, 2.0), [&](ConvBProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(in0[i]) + (in1 ? tbytes((*in1)[i]) : 0.0) + (res ? tbytes((*res)[i]) : 0.0) + (out.empty() ? 0.0 : tbytes(out[i])) +
                   (pooled ? tbytes((*pooled)[i]) : 0.0);
        p.in0 = in0[i].bp(); p.in1 = in1 ? (*in1)[i].bp() : nullptr; p.res = res ? (*res)[i].bp() : nullptr;
        p.out = out.empty() ? nullptr : out[i].bp();
        p.pool = pooled ? (void*)(*pooled)[i].p : nullptr;
        p.H = in0[i].H; p.W = in0[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, 32, th));
        k.flops += 2.0 * in0[i].H * in0[i].W * pc.kh * pc.kw * (double)pc.cin * pc.cout;
    }, [&](ConvBArgs& a, const Chunk& k) {
        a.wpk = (const u32x4*)pc.d_wb; a.bias = pc.d_b;
        a.c0 = in0[0].C; a.c1 = in1 ? (*in1)[0].C : 0;
        a.cout = pc.cout; a.mtiles = pc.mtiles; a.groups = cin / 32;
        a.relu_in = relu_in; a.relu_out = relu_out; a.act = act; a.skip_full = pooled && !keep_full; a.pool_f32 = pool_f32;
        int units;
        a.xm = oneshot_map(m, k.units.total, &units);
        dim3 grid(units, pc.mtiles / mtb);
        ProfScope ps(m, "convb_kernel", k.flops, layer_text(scope, k.sub(in0), pc.cin, pc.cout));
        ps.bytes = k.bytes;
        bool res32 = res != nullptr;                          // the RESP kernels address the residual operand with 32-bit byte offsets
        for (size_t i = k.b0; res && i < k.b1; ++i) res32 = res32 && tbytes((*res)[i]) < 4294967296.0;
        const int key = pc.kh * 100 + pc.bmode * 10 + mtb + (th == 8 && mtb == 2 ? 1000 : 0) + (res32 && pc.bmode == 2 && pc.kh == 3 && mtb >= 2 ? 2000 : 0);
        switch (key) {
            case 3322: ASEP_CONVB_LAUNCH_RES(3, 3, 2, 2, 1, 8, 3); break;       // residual operand in the initial value (32- and >= 64-channel convR_2)
            case 2324: ASEP_CONVB_LAUNCH8(3, 3, 2, 2, 2, 8, 2, true); break;    // (the residual is part of the accumulators' initial value: the eight-wave form's registers)
            case 1322: ASEP_CONVB_LAUNCH(3, 3, 2, 2, 1, 8, 4); break;
            case 301: ASEP_CONVB_LAUNCH(3, 3, 0, 1, 1, 16, 3); break;
            case 302: ASEP_CONVB_LAUNCH(3, 3, 0, 2, 1, 16, 3); break;
            case 304: ASEP_CONVB_LAUNCH(3, 3, 0, 2, 2, 8, 3); break;
            case 311: ASEP_CONVB_LAUNCH(3, 3, 1, 1, 1, 16, 3); break;
            case 312: ASEP_CONVB_LAUNCH(3, 3, 1, 2, 1, 16, 3); break;
            case 314: ASEP_CONVB_LAUNCH(3, 3, 1, 2, 2, 8, 3); break;
            case 321: ASEP_CONVB_LAUNCH(3, 3, 2, 1, 1, 16, 3); break;
            case 324: ASEP_CONVB_LAUNCH8(3, 3, 2, 2, 2, 8, 2, false); break;   // >= 64 channels: eight waves over the same LDS tile
            case 411: ASEP_CONVB_LAUNCH(4, 4, 1, 1, 1, 16, 3); break;
            case 412: ASEP_CONVB_LAUNCH(4, 4, 1, 2, 1, 16, 3); break;
            case 414: ASEP_CONVB_LAUNCH(4, 4, 1, 2, 2, 8, 3); break;
            case 421: ASEP_CONVB_LAUNCH(4, 4, 2, 1, 1, 16, 2); break;
            case 422: ASEP_CONVB_LAUNCH(4, 4, 2, 2, 1, 16, 2); break;
            case 424: ASEP_CONVB_LAUNCH(4, 4, 2, 2, 2, 8, 1); break;       // (16 taps x 4 m-tiles of fragments: one block per CU is what its registers allow)
            default: set_error("conv %s: bf16 kernel variant %d not instantiated", scope.c_str(), key); throw ArgError();
        }
    });
    return out;
}

// fused tail of a residual block (3 x convR + t + ReLU [+ pool]) for the 8- / 16-channel levels
bool has_resb(asep_aru* m, const std::string& scope) { return m->resb.count(scope) != 0; }

TL run_resb_tail(asep_aru* m, const std::string& scope, const TL& t, TL* pooled) {
    const asep_aru::ResB& rb = m->resb.at(scope);
    if (t[0].C != rb.C || !t[0].bf) { set_error("internal: residual tail %s expects %d bf16 channels", scope.c_str(), rb.C); throw ArgError(); }
    TL out;
    for (const Tensor& x : t) out.push_back(new_tensor(m, x.H, x.W, rb.C, true));
    if (pooled) {
        pooled->clear();
        for (const Tensor& x : t) pooled->push_back(new_tensor(m, cdiv(x.H, 2), cdiv(x.W, 2), rb.C, true));
    }
    struct K { void (*fn)(const ResBArgs); };
    static const K tail32[3] = {{res32_tail_kernel<0>}, {res32_tail_kernel<1>}, {res32_tail_kernel<2>}};
    static const K general[2][3] = {{{resb_tail_kernel<8>}, {resb_tail_kernel<8, 1>}, {resb_tail_kernel<8, 2>}}, {{resb_tail_kernel<16>}, {resb_tail_kernel<16, 1>}, {resb_tail_kernel<16, 2>}}};
    for_chunks<ResBArgs>(t.size(), 3.0 * 9.0 * rb.C * rb.C * 2.0, [&](ResBProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(t[i]) + tbytes(out[i]) + (pooled ? tbytes((*pooled)[i]) : 0.0);
        p.t = t[i].bp(); p.out = out[i].bp(); p.pool = pooled ? (*pooled)[i].bp() : nullptr;
        p.H = t[i].H; p.W = t[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, RB_TW, RB_TH));
        k.flops += 2.0 * t[i].H * t[i].W * 3 * 9.0 * rb.C * rb.C;
    }, [&](ResBArgs& a, const Chunk& k) {
        a.wpk = (const u32x4*)rb.d_w; a.bias = rb.d_b;
        const int tiles = k.units.total, act = m->fused_act;
        const TL sub = k.sub(t);
        const std::string what = scope + " (3xconvR+add" + (pooled ? "+pool) " : ") ") + dims_of(sub);
        if (rb.C == 32) {                                    // persistent kernel: table (its units are walked with a grid stride)
            std::vector<TileDims> probs;
            for (int i = 0; i < a.nprob; ++i) probs.push_back({a.p[i].tiles_x, cdiv(a.p[i].H, RB_TH), a.p[i].tile_begin});
            a.sched = (m->use_xcd_sched && tiles >= 8 * 64) ? xcd_schedule(m, probs, tiles) : nullptr;
            static bool attr[3] = {false, false, false};
            if (!attr[act]) {
                ASEP_HIP_CHECK_THROW(hipFuncSetAttribute((const void*)tail32[act].fn, hipFuncAttributeMaxDynamicSharedMemorySize, Res32Layout::BYTES));
                attr[act] = true;
            }
            ProfScope ps(m, "res32_tail_kernel" + targs({ti(act)}), k.flops, what);
            ps.bytes = k.bytes;
            a.ntiles = tiles;
            hipLaunchKernelGGL(tail32[act].fn, dim3(std::min(tiles, m->num_cus)), dim3(512), Res32Layout::BYTES, m->stream, a);
            return;
        }
        int units;
        a.xm = oneshot_map(m, tiles, &units);
        bool small16 = true;                                 // res16f_kernel addresses its tensors with 32-bit byte offsets (32 bytes per pixel)
        for (const Tensor& x : sub) small16 = small16 && (size_t)x.H * x.W < ((size_t)1 << 27);
        // elu / leaky: the general form; 16 channels: the lean form for interior tiles, the general form for border tiles, one launch
        const bool f16 = !act && rb.C == 16 && small16;
        ProfScope ps(m, f16 ? std::string("res16f_kernel") : "resb_tail_kernel" + targs({ti(rb.C), ti(act)}), k.flops, what);
        ps.bytes = k.bytes;
        hipLaunchKernelGGL(f16 ? res16f_kernel : general[rb.C == 16][act].fn, dim3(units), dim3(256), 0, m->stream, a);
    });
    return out;
}

TL run_deconvb(asep_aru* m, const std::string& scope, const TL& in, const TL& like, bool relu_out) {
    const int act = relu_out ? m->cfg.activation : 0;        // (elu / leaky graphs: the deconvolution's activation, layers.py:342-367)
    if (act) relu_out = false;
    auto it = m->convs.find(scope);
    if (it == m->convs.end()) { set_error("internal: deconv %s not packed", scope.c_str()); throw ArgError(); }
    const PackedConv& pc = it->second;
    if (pc.bmode < 1 || !pc.d_wb || in[0].C != pc.cin || !in[0].bf || pc.cout % 8 != 0) {
        set_error("deconv %s (%d -> %d channels) is not served by the bf16 kernels", scope.c_str(), pc.cin, pc.cout);
        throw ArgError();
    }
    TL out;
    for (size_t i = 0; i < in.size(); ++i) {
        if (cdiv(like[i].H, 2) != in[i].H || cdiv(like[i].W, 2) != in[i].W) {
            set_error("deconv %s: output %dx%d incompatible with input %dx%d", scope.c_str(), like[i].H, like[i].W, in[i].H, in[i].W);
            throw ArgError();
        }
        out.push_back(new_tensor(m, like[i].H, like[i].W, pc.cout, true));
    }
    const int mt = pc.mtiles % 2 == 0 ? 2 : 1;
    const bool d8 = pc.d_wb8 && relu_out && !act;           // level 0 (16 -> 8): no LDS, whole pixels straight to HBM
    const int dth = d8 ? D8_RW : 8;                          // input rows per block (16 rows for one m-tile measured slower: 148 -> 187 us at level 0)
    const int dtw = d8 ? D8_TW : DCB_TW;
    void (*const fn)(const DeconvBArgs) = d8 ? deconvb8_kernel : pc.bmode == 1 ? (mt == 1 ? deconvb_kernel<1, 1, 8> : deconvb_kernel<1, 2, 8>)
                                                                               : (mt == 1 ? deconvb_kernel<2, 1, 8> : deconvb_kernel<2, 2, 8>);
    for_chunks<DeconvBArgs>(in.size(), 9.0 * pc.cin * pc.cout * 2.0, [&](DeconvBProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(in[i]) + tbytes(out[i]);
        p.in = in[i].bp(); p.out = out[i].bp();
        p.Hi = in[i].H; p.Wi = in[i].W; p.Ho = out[i].H; p.Wo = out[i].W;
        p.pbh = std::max((in[i].H - 1) * 2 + 3 - out[i].H, 0) / 2;
        p.pbw = std::max((in[i].W - 1) * 2 + 3 - out[i].W, 0) / 2;
        set_tiles(p, k.units.next_tiles(p.Hi, p.Wi, dtw, dth));
        k.flops += 2.0 * in[i].H * in[i].W * 9.0 * pc.cin * pc.cout;
    }, [&](DeconvBArgs& a, const Chunk& k) {
        a.wpk = (const u32x4*)(d8 ? pc.d_wb8 : pc.d_wb); a.bias = pc.d_b;
        a.cin = pc.cin; a.cout = pc.cout; a.mtiles = pc.mtiles; a.groups = pc.cin / 32; a.relu_out = relu_out; a.act = act;
        int units;
        a.xm = oneshot_map(m, k.units.total, &units);
        ProfScope ps(m, d8 ? std::string("deconvb8_kernel") : "deconvb_kernel" + targs({ti(pc.bmode), ti(mt), ti(dth)}), k.flops,
                     layer_text(scope, k.sub(in), pc.cin, pc.cout));
        ps.bytes = k.bytes;
        hipLaunchKernelGGL(fn, d8 ? dim3(units) : dim3(units, pc.mtiles / mt), dim3(256), 0, m->stream, a);
    });
    return out;
}

TL run_chansum_bf(asep_aru* m, const TL& in) {
    TL out;
    for (const Tensor& t : in) out.push_back(new_tensor(m, t.H, t.W, 1));
    stream_pass<PoolBArgs>(m, in, "chansumb_kernel", POOL_ITEMS, [&](PoolBProb& p, size_t i, Chunk& k) {
        k.bytes += tbytes(in[i]) + tbytes(out[i]);
        p.in = in[i].bp(); p.out = out[i].p; p.H = in[i].H; p.W = in[i].W;
        return (size_t)in[i].H * in[i].W;
    }, [&](const PoolBArgs& a, dim3 grid) { hipLaunchKernelGGL(chansumb_kernel, grid, dim3(256), 0, m->stream, a); });
    return out;
}

// ---- network schedule (ARU_v1.py), evaluated for all problems in lock step ---------------------------------
// residual block: conv1 (identity) -> t ; relu ; (res_depth-1) x conv+relu ; conv (identity) ; +t ; relu
// ---- graph variants (asep_aru_cfg.activation != 0 and / or plain_u; fp32 path only): the layer kernels store pre-activation values,
//      act_kernel follows (on the pooled tensor too: the activations are increasing, the fused 2x2 max commutes with them) ----
void apply_act(asep_aru* m, TL& l) {
    stream_pass<PoolArgs>(m, l, "act_kernel", (size_t)POOL_ITEMS * 4, [&](PoolProb& p, size_t i, Chunk& k) {
        k.bytes += 2.0 * tbytes(l[i]);
        p.in = l[i].p; p.out = l[i].p; p.H = p.Ho = l[i].H; p.W = p.Wo = l[i].W;
        return l[i].count();
    }, [&](const PoolArgs& a, dim3 grid) { hipLaunchKernelGGL(act_kernel, grid, dim3(256), 0, m->stream, a, m->cfg.activation); });
}
// conv / deconv / first conv followed by the graph's activation (act = false: identity layers).  Round 4: elu / leaky are applied in the
// epilogue of the producing kernel (ConvArgs::act: the same arithmetic as act_kernel, so the results are bit-identical to the separate pass
// of round 3, which ASEP_FUSE_ACT=0 still selects): a variant's layer is one launch and one write instead of launch + read + write.
// The fused 2x2 max pool sees the ACTIVATED values (both functions are increasing: the same as activating the pooled maximum).
TL conv_act(asep_aru* m, const std::string& scope, const TL& in0, const TL* in1, bool relu_in, bool act, const TL* res,
            TL* pooled = nullptr, bool keep_full = true) {
    if (m->cfg.activation == 0 || !act) return run_conv(m, scope, in0, in1, relu_in, act, res, pooled, keep_full);
    if (m->fuse_act) return run_conv(m, scope, in0, in1, relu_in, false, res, pooled, keep_full, m->cfg.activation);
    TL out = run_conv(m, scope, in0, in1, relu_in, false, res, pooled, keep_full);
    apply_act(m, out);
    if (pooled) apply_act(m, *pooled);
    return out;
}
TL deconv_act(asep_aru* m, const std::string& scope, const TL& in, const TL& like) {
    if (m->cfg.activation == 0) return run_deconv(m, scope, in, like, true);
    if (m->fuse_act) return run_deconv(m, scope, in, like, false, m->cfg.activation);
    TL out = run_deconv(m, scope, in, like, false);
    apply_act(m, out);
    return out;
}
TL direct_act(asep_aru* m, const DirectConv& dc, const TL& imgs, bool act, const std::vector<const float*>& stats) {
    if (m->cfg.activation == 0 || !act) return run_direct(m, dc, imgs, act, stats);
    if (m->fuse_act || m->bf16) return run_direct(m, dc, imgs, false, stats, m->cfg.activation);
    TL out = run_direct(m, dc, imgs, false, stats);
    apply_act(m, out);
    return out;
}

TL res_block_tail(asep_aru* m, const std::string& scope, const TL& t, TL* pooled = nullptr) {
    if (m->bf16 && has_resb(m, scope)) return run_resb_tail(m, scope, t, pooled);      // one kernel for the whole tail
    TL r = t;
    const int rd = m->cfg.res_depth;
    for (int i = 0; i < rd; ++i) {
        const bool last = (i == rd - 1);
        const std::string sc = scope + "/convR_" + std::to_string(i);
        // (relu_in of the first conv: the ReLU between conv1 and convR_0 -- a ReLU in every activation variant, ARU_v1.py:214)
        r = m->bf16 ? run_convb(m, sc, r, nullptr, /*relu_in=*/i == 0, /*relu_out=*/true, last ? &t : nullptr, last ? pooled : nullptr)
                    : conv_act(m, sc, r, nullptr, /*relu_in=*/i == 0, /*act=*/true, last ? &t : nullptr, last ? pooled : nullptr);
    }
    return r;
}

// RU_v2: t += tap(I_l) behind conv1 `scope` (pyr_kernels.h): imgs = the pyramid level of the block, t = conv1's result, one launch for all pages
void run_tap(asep_aru* m, const std::string& scope, const TL& imgs, const TL& t, const std::vector<const float*>& stats) {
    auto it = m->taps.find(scope);
    if (it == m->taps.end()) { set_error("internal: input-pyramid tap of %s not loaded", scope.c_str()); throw ArgError(); }
    const int ch = imgs[0].C, cout = t[0].C;
    for (size_t i = 0; i < t.size(); ++i)
        if (imgs[i].H != t[i].H || imgs[i].W != t[i].W) {
            set_error("internal: input pyramid %dx%d against %dx%d at %s", imgs[i].H, imgs[i].W, t[i].H, t[i].W, scope.c_str());
            throw ArgError();
        }
    for_chunks<TapArgs>(t.size(), 9.0 * ch * cout * 4.0, [&](TapProb& p, size_t i, Chunk& k) {
        p.img = imgs[i].p; p.t = t[i].p; p.stats = stats.empty() ? nullptr : stats[i];
        p.H = t[i].H; p.W = t[i].W;
        set_tiles(p, k.units.next_tiles(p.H, p.W, PYR_TW, PYR_TH));
        k.flops += 2.0 * t[i].H * t[i].W * 9.0 * ch * cout;
        k.bytes += tbytes(imgs[i]) + 2.0 * tbytes(t[i]);       // t is read and written
    }, [&](TapArgs& a, const Chunk& k) {
        a.w = it->second; a.cout = cout;
        ProfScope ps(m, "pyr_tap_kernel<" + ti(ch) + ">", k.flops, layer_text(scope + " tap", k.sub(t), ch, cout));
        ps.bytes = k.bytes;
        launch_pyr_tap(m, a, ch, k.units.total);
    });
}

// names[i] = end-point prefix of problem i ("scale_<s>" for page 0, "p<b>/scale_<s>" otherwise)
TL det_cnn(asep_aru* m, const TL& imgs, const std::vector<std::string>& names, const std::vector<const float*>& stats) {
    const int n = m->cfg.scale_space_num;
    std::vector<TL> skips;
    TL u = imgs;
    // colour pages (3 channels, graphs RU / U): the fused level-0 DOWN forms contain the 1-channel conv1, so the block runs as conv_c3_kernel +
    // the block tail (or conv2), the path of the graph variants; the UP block and the deeper levels never see the page
    const bool rgb = m->det_first.cin == 3;
    // RU_v2 (cfg.input_pyramid): the page average-pooled once per level (RU_v2.py:92-96; with mvn the taps standardise while they load: the pool
    // commutes with the affine map); conv1 of the down blocks l >= 1 and, with inp4up, of the up blocks gets tap(I_l) added to its result
    const bool pyr = m->cfg.input_pyramid != 0, pyr_up = pyr && m->cfg.inp4up != 0;
    std::vector<TL> ipyr;
    if (pyr) {
        ipyr.push_back(imgs);
        for (int l = 1; l < n; ++l) ipyr.push_back(run_pool(m, ipyr.back(), rgb ? POOL_AVG_C3 : POOL_AVG_C1));
    }
    auto publish = [&](const TL& l, const std::string& suffix) {
        for (size_t i = 0; i < l.size(); ++i) m->endpoints[names[i] + suffix] = l[i];
    };
    // the three layer ops of the schedule on the handle's engine; act: the graph's activation behind the layer (the wrappers carry the rules)
    auto first = [&](bool act) { return direct_act(m, m->det_first, imgs, act, stats); };
    auto conv = [&](const std::string& sc, const TL& in0, const TL* in1, bool act, TL* pooled = nullptr) {
        return m->bf16 ? run_convb(m, sc, in0, in1, false, act, nullptr, pooled) : conv_act(m, sc, in0, in1, false, act, nullptr, pooled);
    };
    auto deconv = [&](const std::string& sc, const TL& in, const TL& like) {
        return m->bf16 ? run_deconvb(m, sc, in, like, true) : deconv_act(m, sc, in, like);
    };
    for (int l = 0; l < n; ++l) {
        const std::string scope = "aru_net/featMapG/unet_down_" + std::to_string(l);
        const bool pool = l < n - 1;
        TL d, pooled;
        if (l == 0 && !rgb && (m->bf16 ? m->d_r8b_down_w && m->det_first.k == 3 && m->det_first.cout == 8
                                       : (m->use_fused8 || (m->fused8_var && r8v_fits(imgs))) && m->d_r8_down_wr)) {
            // the whole block in one kernel: image -> d0 (+ pool)
            if (m->bf16) run_res8b(m, false, imgs, nullptr, stats, pool, &d, &pooled);
            else run_res8(m, false, imgs, nullptr, stats, pool, &d, &pooled);
        } else if (m->cfg.plain_u) {                         // graph 'U': conv1 + conv2, both activated (ARU_v1.py:228-233)
            TL c1 = (l == 0) ? first(true) : conv(scope + "/conv1", u, nullptr, true);
            d = conv(scope + "/conv2", c1, nullptr, true, pool ? &pooled : nullptr);
        } else {                                             // conv1 -> t, then the block tail, whose last conv also emits maxpool2(d)
            TL t = (l == 0) ? first(false) : conv(scope + "/conv1", u, nullptr, false);
            if (pyr && l > 0) run_tap(m, scope + "/conv1", ipyr[l], t, stats);
            d = res_block_tail(m, scope, t, pool ? &pooled : nullptr);
        }
        skips.push_back(d);
        publish(d, "_unet_down_" + std::to_string(l) + "_conv");
        if (pool) publish(pooled, "_unet_down_" + std::to_string(l) + "_pool");
        u = pool ? pooled : d;
    }
    for (int l = n - 2; l >= 0; --l) {
        const std::string scope = "aru_net/featMapG/unet_up_" + std::to_string(l);
        const TL& skip = skips[l];
        TL v = deconv(scope + "/deconv", u, skip);
        publish(v, "_unet_up_" + std::to_string(l) + "_deconv");
        if (l == 0 && !pyr_up && (m->bf16 ? m->d_r8b_up_w1 != nullptr : (m->use_fused8 || (m->fused8_var && r8v_fits(skip))) && m->d_r8_up_w1)) {
            TL d, none;                                      // conv1 over [skip, deconv] + the tail in one kernel
            if (m->bf16) run_res8b(m, true, skip, &v, {}, false, &d, &none);
            else run_res8(m, true, skip, &v, {}, false, &d, &none);
            u = d;
        } else if (m->cfg.plain_u) {                         // ARU_v1.py:283-288
            TL c1 = conv(scope + "/conv1", skip, &v, true);
            u = conv(scope + "/conv2", c1, nullptr, true);
        } else {
            TL t = conv(scope + "/conv1", skip, &v, false);  // concat [skip, deconv]
            if (pyr_up) run_tap(m, scope + "/conv1", ipyr[l], t, stats);   // RU_v2.py:142-144: [skip, deconv, I_l]
            u = res_block_tail(m, scope, t);
        }
        publish(u, "_unet_up_" + std::to_string(l) + "_conv");
    }
    return u;
}

TL att_cnn(asep_aru* m, const TL& imgs, const std::vector<const float*>& stats) {
    const std::string p = "aru_net/attMapG/attPart/conv";
    TL y;
    if (m->bf16 && !m->d_att_head) { set_error("bf16 path: attention head 4x4 / 12 channels expected"); throw ArgError(); }
    // the fused head (conv1 + activation + pool, one pooled pixel per thread) also serves the elu / leaky variants (round 4): the pool
    // is taken on the pre-activation values, the activation on the maximum
    const bool head_variant = m->d_att_head && !m->use_fused8 && m->fused8_wanted && m->fuse_act && m->cfg.activation != 0 && m->r8_valu && !m->bf16;
    if (m->d_att_head && (m->use_fused8 || head_variant || m->bf16)) {
        // conv1 + ReLU + pool1 fused (the full-resolution 12-channel tensor is never materialised)
        // (bf16 path: the head writes a 16-channel bf16 plane, channels 12..15 zero)
        for (const Tensor& t : imgs) y.push_back(new_tensor(m, cdiv(t.H, 2), cdiv(t.W, 2), m->bf16 ? 16 : 12, m->bf16));
        bool headb = m->bf16 && m->d_att_headb && m->cfg.activation == 0;
        // (att_headb_kernel addresses the pooled plane with 32-bit element offsets: images of 2^28 pixels and more take the vector-ALU head below,
        //  which refuses them with an error instead of wrapping)
        for (const Tensor& t : imgs) headb = headb && (size_t)t.H * t.W < ((size_t)1 << 28);
        auto fill = [&](int tw, int th) {                    // both heads: tw x th tiles of the page in, the pooled plane out
            return [&, tw, th](C1Prob& q, size_t i, Chunk& k) {
                k.bytes += tbytes(imgs[i]) + tbytes(y[i]);
                q.img = imgs[i].p; q.out = y[i].p; q.stats = stats.empty() ? nullptr : stats[i];
                q.H = imgs[i].H; q.W = imgs[i].W;
                set_tiles(q, k.units.next_tiles(q.H, q.W, tw, th));
                k.flops += 2.0 * imgs[i].H * imgs[i].W * 16.0 * 12;
            };
        };
        // bf16 path, ReLU graph: the head on the bf16 MFMA (image and filter as bfloat16 like the feature CNN's first layer)
        if (headb) for_chunks<AttHeadBArgs>(imgs.size(), 0.0, fill(ATTB_TW, ATTB_TH), [&](AttHeadBArgs& a, const Chunk& k) {
            a.wpk = (const u32x4*)m->d_att_headb; a.bias = m->att_first.d_b;
            int units;
            a.xm = oneshot_map(m, k.units.total, &units);
            ProfScope ps(m, "att_headb_kernel", k.flops);
            ps.bytes = k.bytes;
            hipLaunchKernelGGL(att_headb_kernel, dim3(units), dim3(256), 0, m->stream, a);
        });
        else for_chunks<AttHeadArgs>(imgs.size(), 0.0, fill(ATT_TW, ATT_TH), [&](AttHeadArgs& a, const Chunk& k) {
            a.wpk = (const f32x4*)m->d_att_head; a.bias = m->att_first.d_b; a.w = m->att_first.d_w; a.act = m->cfg.activation;
            bool valu = m->r8_valu || m->bf16;               // vector-ALU form (32-bit output offsets, see r8v_fits)
            for (size_t i = k.b0; i < k.b1; ++i) valu = valu && (size_t)imgs[i].H * imgs[i].W < ((size_t)1 << 28);
            if (m->bf16 && !valu) { set_error("bf16 path: image too large for the attention head kernel"); throw ArgError(); }
            if (head_variant && !valu) { set_error("attention head of an elu / leaky graph: image too large for the vector-ALU kernel"); throw ArgError(); }
            ProfScope ps(m, m->bf16 ? "att_headv_kernel<true>" : (valu ? "att_headv_kernel<false>" : "att_head_kernel"), k.flops);
            ps.bytes = k.bytes;
            const dim3 grid(k.units.total);
            if (m->bf16) hipLaunchKernelGGL(att_headv_kernel<true>, grid, dim3(256), 0, m->stream, a);
            else if (valu) hipLaunchKernelGGL(att_headv_kernel<false>, grid, dim3(256), 0, m->stream, a);
            else hipLaunchKernelGGL(att_head_kernel, grid, dim3(256), 0, m->stream, a);
        });
    } else {
        y = direct_act(m, m->att_first, imgs, true, stats);
        y = run_pool(m, y, POOL_MAX);
    }
    TL pooled;
    if (m->bf16) {
        run_convb(m, p + "2", y, nullptr, false, true, nullptr, &pooled, /*keep_full=*/false);
        y = pooled;
        // the last pooled tensor (1/8 resolution, 32 channels) is written as fp32: conv4 is the fp32 vector-ALU kernel
        run_convb(m, p + "3", y, nullptr, false, true, nullptr, &pooled, /*keep_full=*/false, /*pool_f32=*/true);
        y = pooled;
        return conv_act(m, p + "4", y, nullptr, false, true, nullptr);       // (fp32 vector-ALU kernel; the graph's activation)
    }
    conv_act(m, p + "2", y, nullptr, false, true, nullptr, &pooled, /*keep_full=*/false);   // conv + ReLU + pool in one kernel
    y = pooled;
    conv_act(m, p + "3", y, nullptr, false, true, nullptr, &pooled, /*keep_full=*/false);
    y = pooled;
    y = conv_act(m, p + "4", y, nullptr, false, true, nullptr);
    return y;
}

// B pages of identical size through the net; problems = pages x scales
int forward_impl(asep_aru* m, asep_aru::Lane& L, int page0, int B, const float* const* d_imgs, const int32_t* Hs, const int32_t* Ws,
                 float* const* d_outs, uint8_t* const* d_u8s, uint8_t* const* d_masks, float threshold) {
    const asep_aru_cfg& cfg = m->cfg;
    hipStream_t stream = L.s;
    m->stream = stream;
    m->cur = &L;
    L.pool.begin();
    try {
        const int nsc = cfg.use_attention ? cfg.num_scales_att : 1;
        if (nsc > MAX_SCALES) { set_error("num_scales_att %d > %d", nsc, MAX_SCALES); return ASEP_ERR_UNSUPPORTED; }
        // problem order: page-major, scale-minor
        TL level0;
        std::vector<const float*> stats0;
        for (int b = 0; b < B; ++b) {
            Tensor img;
            img.p = const_cast<float*>(d_imgs[b]);
            img.H = Hs[b]; img.W = Ws[b]; img.C = cfg.channels;            // (pages of a call may differ in size: every launch carries per-problem dims)
            level0.push_back(img);
            const float* st = nullptr;
            if (cfg.mvn && m->page_stats) {                               // computed for all pages of the call in front of it (aru_moments_pages)
                st = m->page_stats[page0 + b];
            } else if (cfg.mvn) {
                const int nparts = grid_1d((img.count() + 3) / 4);        // 16-byte loads: a thread takes four values per step
                double* sums = (double*)L.pool.get(2 * (size_t)nparts * sizeof(double));
                float* stt = (float*)L.pool.get(2 * sizeof(float));
                hipLaunchKernelGGL(moments_kernel, dim3(nparts), dim3(256), 0, stream, img.p, img.count(), sums);
                hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(256), 0, stream, sums, nparts, img.count(), stt);
                st = stt;
            }
            stats0.push_back(st);
        }
        // image pyramid.  With mvn the pyramid is built from the standardised image; avg-pooling commutes with
        // the affine map, so scales >= 1 standardise on load with the page's statistics.
        std::vector<TL> pyr{level0};
        for (int s = 1; s < nsc; ++s) pyr.push_back(run_pool(m, pyr.back(), POOL_AVG_C1));
        TL all;
        std::vector<std::string> names;
        std::vector<const float*> stats;
        for (int b = 0; b < B; ++b)
            for (int s = 0; s < nsc; ++s) {
                all.push_back(pyr[s][b]);
                names.push_back(page_prefix(page0 + b) + "scale_" + std::to_string(s));
                stats.push_back(stats0[b]);
            }
        if (!cfg.mvn) stats.clear();

        TL att;
        bool forked = false;
        if (cfg.use_attention) {
            // the attention CNN is a chain of small launches that cannot fill the chip: run it on a side stream next
            // to the feature branch (fork after the pyramid, join before the combine).  Per-launch profiling keeps
            // everything on one stream so that kernel times are not inflated by the overlap.
            if ((!m->profiling || m->prof_in_situ) && L.side) {
                ASEP_HIP_CHECK(hipEventRecord(L.ev_fork, stream));
                ASEP_HIP_CHECK(hipStreamWaitEvent(L.side, L.ev_fork, 0));
                m->stream = L.side;
                forked = true;
            }
            att = att_cnn(m, all, stats);
            if (forked) {
                ASEP_HIP_CHECK(hipEventRecord(L.ev_join, L.side));
                m->stream = stream;
            }
            for (size_t i = 0; i < att.size(); ++i) m->endpoints[page_prefix(page0 + (int)i / nsc) + "att_" + std::to_string(i % nsc)] = att[i];
        }
        TL feat = det_cnn(m, all, names, stats);
        if (forked) ASEP_HIP_CHECK(hipStreamWaitEvent(stream, L.ev_join, 0));
        TL fsum;
        if (nsc > 1) {
            TL coarse;
            for (int b = 0; b < B; ++b)
                for (int s = 1; s < nsc; ++s) coarse.push_back(feat[b * nsc + s]);
            fsum = m->bf16 ? run_chansum_bf(m, coarse) : run_pool(m, coarse, POOL_CHANSUM);
        }
        for (int b = 0; b < B; ++b) {
            const int H = Hs[b], W = Ws[b];
            CombineArgs ca{};
            ca.nsc = nsc; ca.H = H; ca.W = W;
            ca.f0 = feat[b * nsc].p;
            int up = 8;
            for (int s = 0; s < nsc && cfg.use_attention; ++s) {
                const Tensor& a = att[b * nsc + s];
                if (cdiv(H, up) != a.H || cdiv(W, up) != a.W) { set_error("internal: attention map shape"); return ASEP_ERR_ARG; }
                ca.att[s] = a.p; ca.ah[s] = a.H; ca.aw[s] = a.W; ca.aup[s] = up; ca.ash[s] = 3 + s;
                ca.aph[s] = (a.H * up - H) / 2; ca.apw[s] = (a.W * up - W) / 2;
                up *= 2;
            }
            up = 1;
            for (int s = 1; s < nsc; ++s) {
                const Tensor& f = feat[b * nsc + s];
                up *= 2;
                ca.fsum[s] = fsum[b * (nsc - 1) + (s - 1)].p; ca.fh[s] = f.H; ca.fw[s] = f.W; ca.fup[s] = up; ca.fsh[s] = s;
                ca.fph[s] = (f.H * up - H) / 2; ca.fpw[s] = (f.W * up - W) / 2;
            }
            ca.wl = m->d_logit_w; ca.bl = m->d_logit_b;
            ca.wd = (cfg.apply_softmax && cfg.n_classes == 2) ? m->d_logit_wd : nullptr;
            ca.out = d_outs[b]; ca.out_u8 = d_u8s ? d_u8s[b] : nullptr; ca.out_mask = d_masks ? d_masks[b] : nullptr;
            ca.thr255 = (double)threshold * 255.0;
            ca.softmax = cfg.apply_softmax;
            ca.tiles_x = cdiv(W, COMBINE_TW);
            const int ctiles = ca.tiles_x * cdiv(H, 16);
            int cunits = ctiles;
            ca.xm = oneshot_map(m, ctiles, &cunits);
            dim3 grid(cunits);
            // number of scales as a template constant (1 = no attention, 3 = the default ARU-Net) with 32-bit offsets, for tensors
            // below 4 GB; anything else takes the run-time form
            const bool small = (size_t)H * W * std::max(cfg.feat_root, cfg.n_classes) * sizeof(float) < ((size_t)1 << 32);
            const int nsct = small && (nsc == 1 || nsc == 3) ? nsc : 0;
            const std::string cname = "combine_kernel" + targs({ti(cfg.feat_root), ti(cfg.n_classes), tb(m->bf16), ti(nsct)});
#define ASEP_COMB_N(FR, NC, BF)                                                                    \
        if (nsct == 3) hipLaunchKernelGGL((combine_kernel<FR, NC, BF, 3>), grid, dim3(256), 0, stream, ca);      \
        else if (nsct == 1) hipLaunchKernelGGL((combine_kernel<FR, NC, BF, 1>), grid, dim3(256), 0, stream, ca); \
        else hipLaunchKernelGGL((combine_kernel<FR, NC, BF, 0>), grid, dim3(256), 0, stream, ca);
#define ASEP_COMB(FR, NC)                                                                          \
    if (cfg.feat_root == FR && cfg.n_classes == NC && !m->bf16) {                                  \
        ASEP_COMB_N(FR, NC, false)                                                                 \
    } else
#define ASEP_COMBB(NC)                                                                             \
    if (cfg.feat_root == 8 && cfg.n_classes == NC && m->bf16) {                                    \
        ASEP_COMB_N(8, NC, true)                                                                   \
    } else
            auto launch_combine = [&](const CombineArgs& ca) {
                ASEP_COMBB(1) ASEP_COMBB(2) ASEP_COMBB(3) ASEP_COMBB(4)
                ASEP_COMB(8, 1) ASEP_COMB(8, 2) ASEP_COMB(8, 3) ASEP_COMB(8, 4) ASEP_COMB(16, 2)
                if (cfg.feat_root == 12 && cfg.n_classes == 2 && !m->bf16) launch_combine12(ca, grid, nsct, stream);
                else return false;
                return true;
            };
#undef ASEP_COMB
#undef ASEP_COMBB
#undef ASEP_COMB_N
            if (cfg.input_pyramid) {
                // RU_v2: the logits as an end point of their own ("logits", "p<b>/logits"; the probabilities do not determine them): the same
                // kernel once more without the soft-max, 4 (feat_root + n_classes) bytes per pixel
                const Tensor lg = new_tensor(m, H, W, cfg.n_classes);
                m->endpoints[page_prefix(page0 + b) + "logits"] = lg;
                CombineArgs cl = ca;
                cl.out = lg.p; cl.out_u8 = nullptr; cl.out_mask = nullptr; cl.softmax = 0; cl.wd = nullptr;
                ProfScope pl(m, cname, 2.0 * H * W * 16.0 * cfg.feat_root * cfg.n_classes, "logits end point");
                pl.bytes = tbytes(feat[b * nsc]) + tbytes(lg);
                launch_combine(cl);                          // (an unserved width is reported by the launch below)
            }
            ProfScope ps(m, cname, 2.0 * H * W * 16.0 * cfg.feat_root * cfg.n_classes);
            // scale-0 feature map + per further scale its channel sum + the attention maps in; probabilities (+ uint8 / threshold images) out
            ps.bytes = tbytes(feat[b * nsc]) + (double)H * W * cfg.n_classes * (4.0 + (ca.out_u8 ? 1.0 : 0.0) + (ca.out_mask ? 1.0 : 0.0));
            if (ca.wd) ps.xflops = 2.0 * H * W * 16.0 * cfg.feat_root;   // two classes behind a soft-max: the logits conv runs on the difference filter (half the products)
            for (int s2 = 1; s2 < nsc; ++s2) ps.bytes += tbytes(fsum[b * (nsc - 1) + (s2 - 1)]);
            for (int s2 = 0; s2 < nsc && cfg.use_attention; ++s2) ps.bytes += tbytes(att[b * nsc + s2]);
            if (!launch_combine(ca)) { set_error("combine: feat_root=%d n_classes=%d not instantiated", cfg.feat_root, cfg.n_classes); return ASEP_ERR_UNSUPPORTED; }
        }
        ASEP_HIP_CHECK(hipGetLastError());
    } catch (const HipError&) {
        return ASEP_ERR_HIP;
    } catch (const ArgError&) {
        return ASEP_ERR_ARG;
    }
    return ASEP_OK;
}

// 2*MAC of every conv / deconv of one forward (SURVEY.md section 8d formula)
double flops_impl(const asep_aru_cfg& cfg, int H, int W) {
    auto det = [&](int h, int w) {
        double mac = 0;
        int last = cfg.channels;
        std::vector<std::pair<int, int>> dims;
        int hh = h, ww = w;
        for (int l = 0; l < cfg.scale_space_num; ++l) {
            const int f = cfg.feat_root << l;
            dims.push_back({hh, ww});
            mac += (double)hh * ww * (9.0 * last * f + cfg.res_depth * 9.0 * f * f);
            if (cfg.input_pyramid && l > 0) mac += (double)hh * ww * 9.0 * cfg.channels * f;      // RU_v2: the tap of the pooled page
            last = f;
            if (l < cfg.scale_space_num - 1) { hh = cdiv(hh, 2); ww = cdiv(ww, 2); }
        }
        for (int l = cfg.scale_space_num - 2; l >= 0; --l) {
            const int f = cfg.feat_root << l;
            const auto& di = dims[l + 1];
            const auto& d = dims[l];
            mac += (double)di.first * di.second * 9.0 * last * f;                       // deconv, input resolution
            mac += (double)d.first * d.second * (9.0 * 2 * f * f + cfg.res_depth * 9.0 * f * f);
            if (cfg.input_pyramid && cfg.inp4up) mac += (double)d.first * d.second * 9.0 * cfg.channels * f;
            last = f;
        }
        return mac;
    };
    auto att = [&](int h, int w) {
        double mac = 0;
        int chans[5] = {cfg.channels, 12, 16, 32, 1};
        int hh = h, ww = w;
        for (int i = 0; i < 4; ++i) {
            mac += (double)hh * ww * 16.0 * chans[i] * chans[i + 1];
            if (i < 3) { hh = cdiv(hh, 2); ww = cdiv(ww, 2); }
        }
        return mac;
    };
    double mac = 0;
    const int nsc = cfg.use_attention ? cfg.num_scales_att : 1;
    int h = H, w = W;
    for (int s = 0; s < nsc; ++s) {
        mac += det(h, w);
        if (cfg.use_attention) mac += att(h, w);
        h = cdiv(h, 2); w = cdiv(w, 2);
    }
    mac += (double)H * W * 16.0 * cfg.feat_root * cfg.n_classes;
    return 2.0 * mac;
}

}  // namespace

namespace asep {

int aru_endpoint_dev(asep_aru* m, const char* name, const float** d_ptr, int dims[3], int* is_bf16) {
    if (!m || !name || !d_ptr) { set_error("aru_endpoint_dev: bad argument"); return ASEP_ERR_ARG; }
    auto it = m->endpoints.find(name);
    if (it == m->endpoints.end()) { set_error("backbone has no end point '%s' (run a forward first)", name); return ASEP_ERR_ARG; }
    if (it->second.bf && !is_bf16) { set_error("end point '%s' is bf16 (compute_dtype 1) and the caller reads fp32 maps", name); return ASEP_ERR_UNSUPPORTED; }
    if (is_bf16) *is_bf16 = it->second.bf ? 1 : 0;
    *d_ptr = it->second.p;                                  // bf16 maps: the same address, 2 bytes per value
    if (dims) { dims[0] = it->second.H; dims[1] = it->second.W; dims[2] = it->second.C; }
    return ASEP_OK;
}

// "scale_<s>_unet_{down,up}_<l>_{conv,deconv}" -> feat_root * 2^l (ARU_v1.py:208-292)
int aru_endpoint_channels(const asep_aru* m, const char* name) {
    if (!m || !name) return -1;
    int s = 0, l = 0;
    char kind[16] = {0}, what[16] = {0};
    if (sscanf(name, "scale_%d_unet_%15[a-z]_%d_%15[a-z]", &s, kind, &l, what) != 4) return -1;
    if (l < 0 || l >= m->cfg.scale_space_num) return -1;
    return m->cfg.feat_root << l;
}

void aru_prof_stream(asep_aru* m, hipStream_t st) { if (m) m->stream = st; }
void aru_set_page_stats(asep_aru* m, const float* const* stats) { if (m) m->page_stats = stats; }
bool aru_mvn(const asep_aru* m) { return m && m->cfg.mvn; }
int aru_moments_pages(asep_aru* m, const MomentsPage* d_pages, const int32_t* d_begin, int n, int grid, hipStream_t st) {
    if (!m || n < 1 || grid < 1) { set_error("aru_moments_pages: bad argument"); return ASEP_ERR_ARG; }
    m->stream = st;
    {
        ProfScope ps(m, "moments_pages_kernel", 0.0, std::to_string(n) + " pages");
        hipLaunchKernelGGL(moments_pages_kernel, dim3((unsigned)grid), dim3(256), 0, st, d_pages, d_begin, n);
    }
    {
        ProfScope ps(m, "moments_finish_pages_kernel", 0.0, std::to_string(n) + " pages");
        hipLaunchKernelGGL(moments_finish_pages_kernel, dim3((unsigned)n), dim3(256), 0, st, d_pages);
    }
    ASEP_HIP_CHECK(hipGetLastError());
    return ASEP_OK;
}
int aru_num_classes(const asep_aru* m) { return m ? m->cfg.n_classes : -1; }
int aru_input_channels(const asep_aru* m) { return m ? m->cfg.channels : -1; }

// One record of the handle's launch profile (asep_aru_profile) around launches that ANOTHER engine queues on the stream of the handle's last
// forward: the relation net's feature-map generator runs between the backbone and the ROI kernels and is timed in the same report.
void* aru_prof_begin(asep_aru* m, const char* name, const char* detail, double flops, double bytes) {
    if (!m || !m->profiling) return nullptr;
    ProfScope* ps = new ProfScope(m, name, flops, detail ? detail : "");
    ps->bytes = bytes;
    return ps;
}
void aru_prof_end(void* scope) { delete static_cast<ProfScope*>(scope); }

}  // namespace asep

// ---- weights at load time: which packed vector (aru_pack.h) goes into which member, under which cfg and switch -------------------
namespace {

void load_conv(asep_aru* m, const WeightBlob& blob, const std::string& scope, const char* bias_name = "biases", bool deconv = false) {
    const Layer L = find_layer(blob, scope, bias_name);
    const ConvPack c = pack_conv_layer(scope, L, deconv, m->use_c12, m->bf16, m->split);
    PackedConv pc;
    static_cast<ConvPlan&>(pc) = c.plan;
    pc.d_w = m->put(c.w);
    pc.d_b = m->put(L.b.data);
    pc.d_wino = m->put_some(c.wino);
    pc.d_wv = m->put_some(c.wv);
    pc.d_wb = m->put_some(c.wb);
    pc.d_wb8 = m->put_some(c.wb8);
    pc.d_ws = m->put_some(c.ws);
    pc.d_ws16 = m->put_some(c.ws16);
    m->convs[scope] = pc;
}

void load_direct(asep_aru* m, const WeightBlob& blob, const std::string& scope, DirectConv* dc) {
    const Layer L = find_direct(blob, scope);
    dc->k = L.w.dims[0];
    dc->cout = L.w.dims[3];
    dc->d_w = m->put(L.w.data);
    dc->d_b = m->put(L.b.data);
}

// dynamic LDS of a fused block's kernels
void reserve_lds(std::initializer_list<const void*> kernels, size_t bytes, const char* what) {
    for (const void* k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            set_error("cannot reserve %zu bytes of LDS for the fused %s block", bytes, what);
            throw HipError();
        }
}

void load_weights(asep_aru* m, const WeightBlob& blob, bool variant) {
    const asep_aru_cfg* cfg = &m->cfg;
    const int n = cfg->scale_space_num;
    const bool up = n > 1;
    if (cfg->use_attention) {
        load_direct(m, blob, "aru_net/attMapG/attPart/conv1", &m->att_first);
        if (m->att_first.k == 4 && m->att_first.cout == 12) {
            const FilterView W(blob.find("aru_net/attMapG/attPart/conv1/weights")->second);   // [4][4][1][12]
            m->d_att_head = m->put(pack_att_head(W));
            if (m->bf16) m->d_att_headb = m->put(pack_att_headb(W));
        }
        for (int i = 2; i <= 4; ++i) load_conv(m, blob, "aru_net/attMapG/attPart/conv" + std::to_string(i));
    }
    if (cfg->channels == 3) {                                // colour net: the [3,3,3,cout] filter in conv_c3_kernel's order
        const std::string s0 = "aru_net/featMapG/unet_down_0/conv1";
        const Layer L = find_layer(blob, s0);
        m->det_first.d_w = m->put(pack_first_rgb(s0, L, m->bf16));
        m->det_first.d_b = m->put(L.b.data);
        m->det_first.k = 3; m->det_first.cin = 3; m->det_first.cout = L.w.dims[3];
    } else {
        load_direct(m, blob, "aru_net/featMapG/unet_down_0/conv1", &m->det_first);
    }
    for (int l = 0; l < n; ++l) {
        const std::string s = "aru_net/featMapG/unet_down_" + std::to_string(l);
        if (l > 0) load_conv(m, blob, s + "/conv1");
        if (cfg->plain_u) { load_conv(m, blob, s + "/conv2"); continue; }
        for (int r = 0; r < cfg->res_depth; ++r) load_conv(m, blob, convR(s, r));
    }
    for (int l = n - 2; l >= 0; --l) {
        const std::string s = "aru_net/featMapG/unet_up_" + std::to_string(l);
        load_conv(m, blob, s + "/deconv", "bias", true);
        load_conv(m, blob, s + "/conv1");
        if (cfg->plain_u) { load_conv(m, blob, s + "/conv2"); continue; }
        for (int r = 0; r < cfg->res_depth; ++r) load_conv(m, blob, convR(s, r));
    }
    // fused level-0 residual blocks of the fp32 engines (res8_kernels.h, res8v_kernels.h)
    if ((!variant || m->fused8_var) && !m->bf16 && cfg->feat_root == 8 && cfg->res_depth == 3 && m->det_first.k == 3) {
        const Res8Pack p = pack_res8(blob, up, R8V_WINO);
        m->d_r8_down_wr = m->put(p.down_wr);
        m->d_r8_down_br = m->put(p.down_br);
        m->d_r8v_down_wr = m->put(p.v_down_wr);
        if (up) {
            m->d_r8_up_w1 = m->put(p.up_w1);
            m->d_r8_up_wr = m->put(p.up_wr);
            m->d_r8_up_br = m->put(p.up_br);
            m->d_r8_up_b1 = m->put(p.up_b1);
            m->d_r8v_up_w1 = m->put(p.v_up_w1);
            m->d_r8v_up_wr = m->put(p.v_up_wr);
            reserve_lds({(const void*)res8_up_kernel<false>, (const void*)res8v_up_kernel<0>, (const void*)res8v_up_kernel<1>, (const void*)res8v_up_kernel<2>},
                        R8_UP_LDS, "up");
        }
        reserve_lds({(const void*)res8_down_kernel<false>, (const void*)res8v_down_kernel<0>, (const void*)res8v_down_kernel<1>, (const void*)res8v_down_kernel<2>},
                    R8_DOWN_LDS, "residual");
    }
    if (m->split && !variant && m->d_r8_down_wr) {           // f32s, ReLU graph: the split-product strip walkers (left unset for other shapes)
        const Res8wsPack p = pack_res8ws(blob, up);
        m->d_r8ws_up_w = m->put_some(p.up_w);
        m->d_r8ws_up_w1 = m->put_some(p.up_w1);
        m->d_r8ws_down_w = m->put_some(p.down_w);
    }
    // (bf16 path, elu / leaky / 'U' graphs -- round 5: layer by layer on convb_kernel / deconvb_kernel with the activation in their general
    //  epilogues; the fused blocks below bake the ReLU into packed-bf16 maxima and serve the ReLU residual graphs)
    // (round 6: the elu / leaky RESIDUAL graphs take the GENERAL fused forms of the 8- and 16-channel levels -- res8b_tile / resb_tail_tile apply the
    //  activation to fp32 values and take float maxima in their pools, a template parameter serves them; the 32-channel tail the same way; the lean forms and
    //  the walkers stay the ReLU graphs')
    m->fused_act = (m->bf16 && variant && !cfg->plain_u && cfg->activation != 0 && m->fused8_wanted && m->fuse_act) ? cfg->activation : 0;
    const bool fusedb = m->bf16 && (!variant || m->fused_act);
    if (fusedb && cfg->res_depth == 3 && cfg->feat_root == 8) {
        const Res8bPack p = pack_res8b(blob, up);
        m->d_r8b_down_w = m->put_some(p.down_w);
        m->d_r8b_down_b = m->put_some(p.down_b);
        m->d_r8f_down_w1 = m->put_some(p.f_down_w1);
        m->d_r8b_down_w1r = m->put_some(p.down_w1r);
        m->d_r8b_up_w = m->put_some(p.up_w);
        m->d_r8b_up_b = m->put_some(p.up_b);
        m->d_r8b_up_w1 = m->put_some(p.up_w1);
        m->d_r8b_up_b1 = m->put_some(p.up_b1);
        m->d_r8f_up_w1 = m->put_some(p.f_up_w1);
    }
    if (fusedb && cfg->res_depth == 3)
        for (int l = 0; l < n; ++l) {
            const int f = cfg->feat_root << l;
            if (f != 8 && f != 16 && !(f == 32 && m->use_res32)) continue;
            for (const char* side : {"down", "up"}) {
                if (side[0] == 'u' && l == n - 1) continue;
                const std::string scope = std::string("aru_net/featMapG/unet_") + side + "_" + std::to_string(l);
                const ResbPack p = pack_resb(blob, scope, f);
                if (p.ok) m->resb[scope] = {f, m->put(p.w), m->put(p.b)};
            }
        }
    const Layer logit = find_layer(blob, "aru_net/logit/class");
    if (!has_shape(logit.w, 4, 4, cfg->feat_root, cfg->n_classes)) {
        set_error("weights: aru_net/logit/class/weights must be [4,4,%d,%d]", cfg->feat_root, cfg->n_classes);
        throw PackRefusal{ASEP_ERR_WEIGHTS};
    }
    m->d_logit_w = m->put(logit.w.data);
    m->d_logit_b = m->put(logit.b.data);
    if (cfg->n_classes == 2) m->d_logit_wd = m->put(pack_logit_diff(logit));
}

}  // namespace

extern "C" {

asep_aru* asep_aru_load(const void* weight_blob, size_t nbytes, const asep_aru_cfg* cfg) {
    ASEP_GUARD_BEGIN
    if (!cfg || !weight_blob) { set_error("asep_aru_load: null argument"); return nullptr; }
    if (cfg->struct_size != (int32_t)sizeof(asep_aru_cfg)) {
        set_error("asep_aru_load: cfg.struct_size is %d, this library's asep_aru_cfg has %zu bytes (ABI version %d): the binding was "
                  "written against another include/asep_hip.h", cfg->struct_size, sizeof(asep_aru_cfg), ASEP_ABI_VERSION);
        return nullptr;
    }
    if (cfg->channels != 1 && cfg->channels != 3) { set_error("asep_aru_load: %d input channels: 1 (gray) and 3 (RGB) are supported", cfg->channels); return nullptr; }
    if (cfg->channels == 3 && cfg->use_attention) {
        set_error("asep_aru_load: 3-channel input needs a graph without attention (RU or U): the attention graph upsamples its attention map to the "
                  "input's shape with a one-channel filter (ARU_v1.py:115)");
        return nullptr;
    }
    if (cfg->compute_dtype < 0 || cfg->compute_dtype > 2) { set_error("asep_aru_load: compute_dtype %d unknown (0 = fp32, 1 = bf16 MFMA, 2 = fp32 with split bf16 products)", cfg->compute_dtype); return nullptr; }
    if (cfg->scale_space_num < 1 || cfg->res_depth < 1) { set_error("asep_aru_load: bad cfg"); return nullptr; }
    if (cfg->activation < 0 || cfg->activation > 2) { set_error("asep_aru_load: activation %d unknown (0 = relu, 1 = elu, 2 = leaky)", cfg->activation); return nullptr; }
    const bool variant = cfg->activation != 0 || cfg->plain_u != 0;
    if (cfg->plain_u && cfg->use_attention) { set_error("asep_aru_load: graph 'U' has no attention branch (ARU_v1.py:92-97)"); return nullptr; }
    if (cfg->inp4up && !cfg->input_pyramid) { set_error("asep_aru_load: inp4up is an option of the input-pyramid graph (RU_v2.py:143): set input_pyramid"); return nullptr; }
    if (cfg->input_pyramid && (cfg->use_attention || cfg->plain_u)) {
        set_error("asep_aru_load: the input-pyramid graph (RU_v2) is a residual U-Net without attention (RU_v2.py:56: useResidual=True, no attMapG): "
                  "use_attention and plain_u must be 0");
        return nullptr;
    }
    if (cfg->input_pyramid && cfg->compute_dtype == 1) {
        set_error("asep_aru_load: the input-pyramid graph (RU_v2) is served by the fp32 engines (compute_dtype 0 or 2): the bf16 engine's fused block "
                  "tails round conv1's result to bfloat16 before the pooled page's term could be added");
        return nullptr;
    }
    std::map<std::string, HostTensor> blob;
    if (!parse_blob(weight_blob, nbytes, blob)) return nullptr;
    std::map<std::string, std::vector<float>> taps;
    if (cfg->input_pyramid) {
        try {
            // ru_net/... -> the names and conv1 shapes of the packers + the taps' rows; a conv1 wider than the tap launch's LDS bound is refused
            blob = split_pyramid_blob(blob, *cfg, taps, PYR_MAX_COUT);
        } catch (const PackRefusal&) {
            return nullptr;
        }
    }
    warn_ignored_switches();
    std::unique_ptr<asep_aru> m(new asep_aru());
    m->cfg = *cfg;
    m->bf16 = cfg->compute_dtype == 1;
    m->split = cfg->compute_dtype == 2;
    // Engine switches (environment, read at load): each selects an INDEPENDENT implementation of the same arithmetic that the test suite
    // compares with the default one (fused against unfused, vector-ALU against MFMA form), or a schedule knob of the bench; the switches of
    // experiments that lost left the tree in round 5 (table: DESIGN.md section 4.5).
    if (const char* e = getenv("ASEP_FUSE_POOL")) m->fuse_pool = atoi(e) != 0;
    if (const char* e = getenv("ASEP_FUSE_ACT")) m->fuse_act = atoi(e) != 0;
    if (const char* e = getenv("ASEP_C12")) m->use_c12 = atoi(e) != 0;
    if (const char* e = getenv("ASEP_FUSED8")) m->use_fused8 = atoi(e) != 0;
    m->fused8_wanted = m->use_fused8;
    if (variant) m->use_fused8 = false;                      // the fused level-0 blocks / attention head are ReLU residual kernels
    if (const char* e = getenv("ASEP_R8_VALU")) m->r8_valu = atoi(e) != 0;
    m->fused8_var = variant && !cfg->plain_u && cfg->activation != 0 && m->fused8_wanted && m->r8_valu && m->fuse_act && !m->bf16;
    if (const char* e = getenv("ASEP_XCD_SCHED")) m->use_xcd_sched = atoi(e) != 0;
    if (const char* e = getenv("ASEP_BF_RES32")) m->use_res32 = atoi(e) != 0;
    if (const char* e = getenv("ASEP_BF_CONVR")) m->use_convr = atoi(e) != 0;
    if (const char* e = getenv("ASEP_SPLIT_DECONV")) m->use_deconvs = atoi(e) != 0;
    if (const char* e = getenv("ASEP_SPLIT_WALK")) m->use_split_walk = atoi(e) != 0;
    if (const char* e = getenv("ASEP_BF_WALK")) { m->walk_mode = atoi(e); m->use_walk = m->walk_mode != 0; }
    if (const char* e = getenv("ASEP_LANES")) { m->num_lanes = std::max(1, std::min(4, atoi(e))); m->lanes_forced = true; }
    for (int l = 0; l < m->num_lanes; ++l) {
        std::unique_ptr<asep_aru::Lane> L(new asep_aru::Lane());
        bool ok = hipStreamCreateWithFlags(&L->side, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&L->bside, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&L->ev_fork, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&L->ev_bfork, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&L->ev_bjoin, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&L->ev_join, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&L->ev_begin, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&L->ev_done, hipEventDisableTiming) == hipSuccess;
        if (ok && l > 0) { ok = hipStreamCreateWithFlags(&L->s, hipStreamNonBlocking) == hipSuccess; L->own_stream = ok; }
        if (!ok) { set_error("asep_aru_load: cannot create streams/events for lane %d", l); return nullptr; }
        m->lanes.push_back(std::move(L));
    }
    m->cur = m->lanes[0].get();
    for (const auto& t : taps) m->taps[t.first] = m->put(t.second);
    try {
        load_weights(m.get(), blob, variant);
    } catch (const PackRefusal&) {                           // (the error text is set)
        return nullptr;
    }
    {
        hipDeviceProp_t prop;
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            m->num_cus = prop.multiProcessorCount;
    }
    m->d_stats = m->alloc<float>(2);
    m->d_sums = m->alloc<double>(2);
    m->d_zero_trash = m->alloc<unsigned char>(8192);
    ASEP_HIP_CHECK_THROW(hipMemset(m->d_zero_trash, 0, 8192));
    return m.release();
    ASEP_GUARD_END_PTR
}

void asep_aru_free(asep_aru* m) { delete m; }

// splits the pages over the lanes (lane 0 = the caller's stream), forks / joins with events
static int forward_lanes(asep_aru* m, int n_pages, const float* const* d_imgs, const int32_t* Hs, const int32_t* Ws, float* const* d_outs,
                         uint8_t* const* d_u8, uint8_t* const* d_mask, float threshold, hipStream_t stream) {
    m->endpoints.clear();
    // (per-launch profiling runs on one lane in every mode: the isolated mode brackets one kernel at a time, the in-situ mode keeps the side
    //  stream and whatever the caller runs beside the net, but not a second launch of the SAME kernel beside the bracketed one)
    // a lane takes at least four pages (= one full 12-problem launch per layer with three scales): fewer pages per launch cost the deep levels
    // more than a second lane returns; ASEP_LANES (lanes_forced) keeps the plain split for the measurement scripts and tests
    const int by_pages = m->lanes_forced ? n_pages : n_pages / 4;
    const int nl = (m->profiling || n_pages < 2) ? 1 : std::max(1, std::min<int>((int)m->lanes.size(), by_pages));
    asep_aru::Lane& L0 = *m->lanes[0];
    L0.s = stream;
    // A lane's arena keeps the buffers of the largest call it has served.  When the number of lanes of a call changes (16 pages on two lanes, then
    // the same 16 pages on one lane while launch times are recorded) the arenas would add up to 1.5 x the pages in flight -- 144 GB instead of 96 for
    // 16 fp32 pages, and a second process of the same size beside it no longer fits into 288 GB (round 6: the children of the default bench line
    // ran out of memory).  A change of the lane count therefore releases every arena first (hipFree waits for the device: nothing is in use).
    if (nl != m->last_nl && n_pages > 1) {
        if (m->last_nl != 0)
            for (auto& Lp : m->lanes) Lp->pool.release();
        m->last_nl = nl;
    }
    if (nl == 1) return forward_impl(m, L0, 0, n_pages, d_imgs, Hs, Ws, d_outs, d_u8, d_mask, threshold);
    ASEP_HIP_CHECK(hipEventRecord(L0.ev_begin, stream));
    int page0 = 0;
    for (int l = 0; l < nl; ++l) {
        asep_aru::Lane& L = *m->lanes[l];
        const int cnt = n_pages / nl + (l < n_pages % nl ? 1 : 0);
        if (l > 0) ASEP_HIP_CHECK(hipStreamWaitEvent(L.s, L0.ev_begin, 0));
        int rc = forward_impl(m, L, page0, cnt, d_imgs + page0, Hs + page0, Ws + page0, d_outs + page0, d_u8 ? d_u8 + page0 : nullptr,
                              d_mask ? d_mask + page0 : nullptr, threshold);
        if (rc) return rc;
        if (l > 0) {
            ASEP_HIP_CHECK(hipEventRecord(L.ev_done, L.s));
            ASEP_HIP_CHECK(hipStreamWaitEvent(stream, L.ev_done, 0));
        }
        page0 += cnt;
    }
    m->stream = stream;
    return ASEP_OK;
}

int asep_aru_forward_dev(asep_aru* m, const float* d_img, int H, int W, float* d_out, uint8_t* d_out_u8,
                         uint8_t* d_out_mask, float threshold, void* stream) {
    ASEP_GUARD_BEGIN
    if (!m || !d_img || !d_out || H < 1 || W < 1) { set_error("asep_aru_forward_dev: bad argument"); return ASEP_ERR_ARG; }
    const int32_t h1 = H, w1 = W;
    return forward_lanes(m, 1, &d_img, &h1, &w1, &d_out, d_out_u8 ? &d_out_u8 : nullptr, d_out_mask ? &d_out_mask : nullptr,
                         threshold, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_aru_forward_batch_dev(asep_aru* m, int n_pages, const float* const* d_imgs, int H, int W, float* const* d_outs,
                               uint8_t* const* d_out_u8, uint8_t* const* d_out_mask, float threshold, void* stream) {
    ASEP_GUARD_BEGIN
    if (!m || !d_imgs || !d_outs || n_pages < 1 || H < 1 || W < 1) { set_error("asep_aru_forward_batch_dev: bad argument"); return ASEP_ERR_ARG; }
    for (int b = 0; b < n_pages; ++b)
        if (!d_imgs[b] || !d_outs[b] || (d_out_u8 && !d_out_u8[b]) || (d_out_mask && !d_out_mask[b])) {
            set_error("asep_aru_forward_batch_dev: null page pointer at %d", b);
            return ASEP_ERR_ARG;
        }
    const std::vector<int32_t> hs(n_pages, H), ws(n_pages, W);
    return forward_lanes(m, n_pages, d_imgs, hs.data(), ws.data(), d_outs, d_out_u8, d_out_mask, threshold, (hipStream_t)stream);
    ASEP_GUARD_END
}

// ABI 6: the same for pages of DIFFERENT sizes (the reference runs page by page on whatever size --fixed_height / --scaling_factor leave:
// ARU_v1.py:64, run_net_post_processing.py:61-82; real scans differ in width).  Every grouped launch already carries per-problem dims (the
// three scales of a page), so pages of any sizes share the launches of a layer.
int asep_aru_forward_batch_dev2(asep_aru* m, int n_pages, const float* const* d_imgs, const int32_t* H, const int32_t* W, float* const* d_outs,
                                uint8_t* const* d_out_u8, uint8_t* const* d_out_mask, float threshold, void* stream) {
    ASEP_GUARD_BEGIN
    if (!m || !d_imgs || !d_outs || !H || !W || n_pages < 1) { set_error("asep_aru_forward_batch_dev2: bad argument"); return ASEP_ERR_ARG; }
    for (int b = 0; b < n_pages; ++b)
        if (!d_imgs[b] || !d_outs[b] || (d_out_u8 && !d_out_u8[b]) || (d_out_mask && !d_out_mask[b]) || H[b] < 1 || W[b] < 1) {
            set_error("asep_aru_forward_batch_dev2: null page pointer or empty page at %d", b);
            return ASEP_ERR_ARG;
        }
    return forward_lanes(m, n_pages, d_imgs, H, W, d_outs, d_out_u8, d_out_mask, threshold, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_aru_forward(asep_aru* m, const float* img_hw, int H, int W, float* out_hwc, uint8_t* out_u8,
                     uint8_t* out_mask, float threshold) {
    ASEP_GUARD_BEGIN
    if (!m || !img_hw || !out_hwc || H < 1 || W < 1) { set_error("asep_aru_forward: bad argument"); return ASEP_ERR_ARG; }
    const size_t npix = (size_t)H * W, nin = npix * m->cfg.channels, nout = npix * m->cfg.n_classes;
    // staging buffers live in the handle and only grow (a page-sized hipMalloc / hipFree pair per call costs
    // milliseconds, comparable to the net itself on small inputs)
    float *d_img = nullptr, *d_out = nullptr;
    uint8_t *d_u8 = nullptr, *d_mask = nullptr;
    try {
        m->host_stage.begin();
        d_img = (float*)m->host_stage.get(nin * sizeof(float));
        d_out = (float*)m->host_stage.get(nout * sizeof(float));
        d_u8 = (uint8_t*)m->host_stage.get(nout);
        d_mask = (uint8_t*)m->host_stage.get(nout);
    } catch (const HipError&) {
        return ASEP_ERR_HIP;
    }
    // All transfers and the forward are queued on one stream, one synchronisation at the end.  Page-locked caller buffers
    // (asep_host_alloc / asep_host_register) are device-visible: the net's last kernel then writes its outputs straight
    // into them over the link (no staging buffer, no separate download: 108 MB of probabilities leave while the kernel
    // runs); the input is still copied once (it is read by several kernels).  Pageable buffers take staged copies.
    if (!m->host_stream) ASEP_HIP_CHECK(hipStreamCreateWithFlags(&m->host_stream, hipStreamNonBlocking));
    hipStream_t hs = m->host_stream;
    auto device_view = [](void* host) -> void* {
        if (!host) return nullptr;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
    };
    float* v_out = (float*)device_view(out_hwc);
    uint8_t* v_u8 = (uint8_t*)device_view(out_u8);
    uint8_t* v_mask = (uint8_t*)device_view(out_mask);
    ASEP_HIP_CHECK(hipMemcpyAsync(d_img, img_hw, nin * sizeof(float), hipMemcpyHostToDevice, hs));
    const int rc = asep_aru_forward_dev(m, d_img, H, W, v_out ? v_out : d_out, out_u8 ? (v_u8 ? v_u8 : d_u8) : nullptr,
                                        out_mask ? (v_mask ? v_mask : d_mask) : nullptr, threshold, hs);
    if (rc) return rc;
    if (out_u8 && !v_u8) ASEP_HIP_CHECK(hipMemcpyAsync(out_u8, d_u8, nout, hipMemcpyDeviceToHost, hs));
    if (out_mask && !v_mask) ASEP_HIP_CHECK(hipMemcpyAsync(out_mask, d_mask, nout, hipMemcpyDeviceToHost, hs));
    if (!v_out) ASEP_HIP_CHECK(hipMemcpyAsync(out_hwc, d_out, nout * sizeof(float), hipMemcpyDeviceToHost, hs));
    ASEP_HIP_CHECK(hipStreamSynchronize(hs));
    return ASEP_OK;
    ASEP_GUARD_END
}

long asep_aru_get_endpoint(asep_aru* m, const char* name, float* out, size_t max_floats, int32_t dims[3]) {
    ASEP_GUARD_BEGIN
    if (!m || !name) { set_error("asep_aru_get_endpoint: bad argument"); return ASEP_ERR_ARG; }
    auto it = m->endpoints.find(name);
    if (it == m->endpoints.end()) { set_error("asep_aru_get_endpoint: unknown end point '%s'", name); return ASEP_ERR_ARG; }
    const Tensor& t = it->second;
    if (dims) { dims[0] = t.H; dims[1] = t.W; dims[2] = t.C; }
    if (!out) return (long)t.count();
    if (max_floats < t.count()) { set_error("asep_aru_get_endpoint: buffer too small"); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipStreamSynchronize(m->stream));
    if (t.bf) {                                             // bf16 tensor: widened on the host
        std::vector<bf16_t> tmp(t.count());
        ASEP_HIP_CHECK(hipMemcpy(tmp.data(), t.p, t.count() * sizeof(bf16_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) {
            const uint32_t u = (uint32_t)tmp[i] << 16;
            memcpy(out + i, &u, 4);
        }
        return (long)t.count();
    }
    ASEP_HIP_CHECK(hipMemcpy(out, t.p, t.count() * sizeof(float), hipMemcpyDeviceToHost));
    return (long)t.count();
    ASEP_GUARD_END
}

// ABI 6: give the handle's device arenas back (they are rebuilt by the next forward call): a process that holds a model and starts another
// GPU process of its size beside it calls this first
int asep_aru_trim(asep_aru* m) {
    ASEP_GUARD_BEGIN
    if (!m) { set_error("asep_aru_trim: null handle"); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipDeviceSynchronize());
    m->endpoints.clear();
    for (auto& Lp : m->lanes) Lp->pool.release();
    m->host_stage.release();
    m->last_nl = 0;
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_aru_profile(asep_aru* m, int enable) {
    ASEP_GUARD_BEGIN
    if (!m) { set_error("asep_aru_profile: null handle"); return ASEP_ERR_ARG; }
    m->profiling = enable != 0;
    m->prof_detail = enable == 2;
    m->prof_in_situ = enable == 3;
    if (enable) { m->prof_recs.clear(); m->ev_next = 0; m->prof_names.clear(); }
    return ASEP_OK;
    ASEP_GUARD_END
}

long asep_aru_profile_report(asep_aru* m, char* buf, size_t buflen) {
    ASEP_GUARD_BEGIN
    if (!m || !buf || buflen < 2) { set_error("asep_aru_profile_report: bad argument"); return ASEP_ERR_ARG; }
    ASEP_HIP_CHECK(hipStreamSynchronize(m->stream));
    const size_t nk = m->prof_names.size();
    std::vector<double> ms(nk, 0.0), fl(nk, 0.0), by(nk, 0.0), xf(nk, 0.0);
    std::vector<long> calls(nk, 0);
    for (const auto& r : m->prof_recs) {
        float t = 0.f;
        ASEP_HIP_CHECK(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.kid] += t; fl[r.kid] += r.flops; by[r.kid] += r.bytes; xf[r.kid] += r.xflops; calls[r.kid] += 1;
    }
    std::string js = "[";
    for (size_t i = 0; i < nk; ++i) {
        if (!calls[i]) continue;
        char line[512];
        snprintf(line, sizeof(line), "%s{\"kernel\":\"%s\",\"calls\":%ld,\"total_ms\":%.6f,\"flops\":%.6e,\"bytes\":%.6e,\"executed_flops\":%.6e}",
                 js.size() > 1 ? "," : "", m->prof_names[i].c_str(), calls[i], ms[i], fl[i], by[i], xf[i]);
        js += line;
    }
    js += "]";
    if (js.size() + 1 > buflen) { set_error("asep_aru_profile_report: buffer too small (%zu needed)", js.size() + 1); return ASEP_ERR_ARG; }
    memcpy(buf, js.c_str(), js.size() + 1);
    return (long)js.size();
    ASEP_GUARD_END
}

double asep_aru_flops(const asep_aru* m, int H, int W) {
    if (!m) return 0.0;
    return flops_impl(m->cfg, H, W);
}

int asep_aru_walker_occupancy(int up) {
    ASEP_GUARD_BEGIN
    int blocks = 0;
    if (up) { ASEP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, res8ws_kernel<true>, 64, 0)); }
    else { ASEP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, res8ws_kernel<false>, 64, 0)); }
    return blocks;
    ASEP_GUARD_END
}

}  // extern "C"

// The colour first layer's instantiations come last in this file, and with that last in its code object: every other kernel keeps the place it
// has without them.  (Known open fault of the bf16 engine, older than these kernels and independent of their code: on gray pages whose level-3
// map is one row high (13 x 45 in tests/test_bf16_batch_fuzz_gpu.py: scale_1_unet_up_3_conv, 1 x 3 pixels, 64 channels) a forward
// intermittently gives another result, 5 % of max|ref| off.  How often depends on the build: never seen in ten runs without these kernels in the
// library, five of six runs with them emitted in the middle of the code object, one of four with them last.  DESIGN.md section 7.)
namespace {
void launch_conv_c3(asep_aru* m, const C1Args& a, int cout, bool bf, int tiles) {
    if (bf) hipLaunchKernelGGL((conv_c3_kernel<8, true>), dim3(tiles), dim3(256), 0, m->stream, a);
    else if (cout == 16) hipLaunchKernelGGL((conv_c3_kernel<16, false>), dim3(tiles), dim3(256), 0, m->stream, a);
    else hipLaunchKernelGGL((conv_c3_kernel<8, false>), dim3(tiles), dim3(256), 0, m->stream, a);
}
// The RU_v2 kernels (pyr_kernels.h) and the feat_root 12 forms of the first layer and the logits kernel follow them for the same reason.
void launch_avgpool_c3(asep_aru* m, const PoolArgs& a, dim3 grid) { hipLaunchKernelGGL(avgpool2_cn_kernel<3>, grid, dim3(256), 0, m->stream, a); }
void launch_pyr_tap(asep_aru* m, const TapArgs& a, int ch, int tiles) {
    if (ch == 3) hipLaunchKernelGGL(pyr_tap_kernel<3>, dim3(tiles), dim3(256), pyr_tap_lds(3, a.cout), m->stream, a);
    else hipLaunchKernelGGL(pyr_tap_kernel<1>, dim3(tiles), dim3(256), pyr_tap_lds(1, a.cout), m->stream, a);
}
void launch_conv_c1_12(asep_aru* m, const C1Args& a, int tiles) { hipLaunchKernelGGL((conv_c1_kernel<3, 12>), dim3(tiles), dim3(256), 0, m->stream, a); }
void launch_combine12(const CombineArgs& ca, dim3 grid, int nsct, hipStream_t stream) {
    if (nsct == 1) hipLaunchKernelGGL((combine_kernel<12, 2, false, 1>), grid, dim3(256), 0, stream, ca);
    else hipLaunchKernelGGL((combine_kernel<12, 2, false, 0>), grid, dim3(256), 0, stream, ca);
}
}  // namespace

#if defined(R8F_TRACE)
// debug builds only (see R8F_MARK in bf16_kernels.h); not part of include/asep_hip.h
extern "C" int asep_debug_r8f_trace(int up, unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(asep::g_r8f_trace), sizeof(unsigned long long) * n, (size_t)(up ? 1 : 0) * 4096 * 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}
#endif

#if defined(CVR_TRACE)
extern "C" int asep_debug_cvr_trace(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(asep::g_cvr_trace), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
#endif
#if defined(CVB_TRACE)
// debug builds only (see CVB_MARK in bf16_kernels.h); not part of include/asep_hip.h
extern "C" int asep_debug_cvb_trace(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(asep::g_cvb_trace), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
#endif
