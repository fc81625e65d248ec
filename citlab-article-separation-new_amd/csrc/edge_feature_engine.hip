// Host side of the edge feature engine (include/asep_hip.h, "edge features" block): one entry point on the asep_post handle (its stream
// and buffer pool).  Integer work only, so no floating-point flags are needed for this object.
#include <algorithm>
#include <string>
#include <vector>

#include "asep_common.h"
#include "edge_tables.h"
#include "edge_feature_kernels.h"

using namespace asep;

static_assert(ASEP_EDGE_COORD_MAX == EDGE_COORD_MAX, "coordinate bound of the header and of edge_tables.h");
static_assert(ASEP_EDGE_RULE_BB == EF_RULE_BB && ASEP_EDGE_RULE_LINE == EF_RULE_LINE, "rule codes");
static_assert(ASEP_SEP_NONE == EF_SEP_NONE && ASEP_SEP_HORIZONTAL == EF_SEP_HORIZONTAL && ASEP_SEP_VERTICAL == EF_SEP_VERTICAL &&
                  ASEP_SEP_OTHER == EF_SEP_OTHER, "orientation codes");
static_assert(sizeof(EfBox) == 16 && sizeof(int2) == 8 && sizeof(uchar2) == 2, "layouts the tables are uploaded in");

namespace {

thread_local double g_kernel_us = 0.0;     // device time of this thread's last call (all its kernels)
thread_local std::string g_launches = "[]";   // what that call launched

struct LaunchLog {
    std::string js = "[";
    void add(const char* kernel, unsigned blocks) {
        if (js.size() > 1) js += ", ";
        js += std::string("{\"kernel\": \"") + kernel + "\", \"blocks\": " + std::to_string(blocks) + "}";
    }
    std::string done() const { return js + "]"; }
};

// blocks of EF_BLOCK threads per page for `count(k)` items of page k -> prefix table; false if the grid does not fit an int32
template <class F>
bool block_table(int n_pages, F count, std::vector<int32_t>& blk_off) {
    blk_off.assign((size_t)n_pages + 1, 0);
    int64_t total = 0;
    for (int k = 0; k < n_pages; ++k) {
        total += (count(k) + EF_BLOCK - 1) / EF_BLOCK;
        if (total > INT32_MAX) return false;
        blk_off[k + 1] = (int32_t)total;
    }
    return true;
}

}  // namespace

double asep_edge_features_last_kernel_us(void) { return g_kernel_us; }

long asep_edge_features_last_launches(char* buf, size_t buflen) {
    if (!buf || buflen < g_launches.size() + 1) {
        set_error("asep_edge_features_last_launches: buffer too small (%zu needed)", g_launches.size() + 1);
        return ASEP_ERR_ARG;
    }
    std::memcpy(buf, g_launches.c_str(), g_launches.size() + 1);
    return (long)g_launches.size();
}

int asep_edge_features_run(asep_post* p, int n_pages, const int32_t* node_off, const int32_t* node_pt_off, const int32_t* node_pts,
                           const uint8_t* node_heading, const int32_t* sep_off, const int32_t* sep_pt_off, const int32_t* sep_pts,
                           const uint8_t* sep_orient, const int32_t* edge_off, const int32_t* edges, int rule, uint8_t* out_flags,
                           int32_t* out_hull, int32_t* out_hull_n, int hull_cap, long long hull_budget_bytes, uint8_t* out_pairs) {
    const char* const FN = "asep_edge_features_run";
    g_kernel_us = 0.0;
    g_launches = "[]";
    if (!p || n_pages < 0 || !node_off || !sep_off || !edge_off) {
        set_error("%s: bad arguments (n_pages %d >= 0, handle, node_off, sep_off and edge_off given)", FN, n_pages);
        return ASEP_ERR_ARG;
    }
    if (rule != ASEP_EDGE_RULE_BB && rule != ASEP_EDGE_RULE_LINE) {
        set_error("%s: unknown rule %d, not ASEP_EDGE_RULE_BB (0) or ASEP_EDGE_RULE_LINE (1)", FN, rule);
        return ASEP_ERR_ARG;
    }
    if (!check_polygons(FN, "region", "node_off", "node_pt_off", n_pages, node_off, node_pt_off, node_pts) ||
        !check_polygons(FN, "separator", "sep_off", "sep_pt_off", n_pages, sep_off, sep_pt_off, sep_pts) ||
        !check_edges(FN, n_pages, node_off, edge_off, edges))
        return ASEP_ERR_ARG;
    const int n_nodes = node_off[n_pages], n_seps = sep_off[n_pages], n_edges = edge_off[n_pages];
    if ((n_seps && !sep_orient) || (out_pairs && n_nodes && !node_heading)) {
        set_error("%s: null argument (sep_orient, or node_heading for the pair bits)", FN);
        return ASEP_ERR_ARG;
    }
    for (int s = 0; s < n_seps; ++s)
        if (sep_orient[s] > ASEP_SEP_OTHER) {
            set_error("%s: separator %d has the orientation code %d, not one of ASEP_SEP_* (0 .. 3)", FN, s, sep_orient[s]);
            return ASEP_ERR_ARG;
        }
    const bool hulls = out_hull || out_hull_n;
    if (hulls) {
        if (!out_hull || !out_hull_n) {
            set_error("%s: out_hull and out_hull_n come together", FN);
            return ASEP_ERR_ARG;
        }
        if (!check_hull_room(FN, n_pages, node_off, node_pt_off, edge_off, edges, hull_cap, hull_budget_bytes)) return ASEP_ERR_ARG;
    }
    std::vector<int64_t> pair_off((size_t)n_pages + 1, 0);
    for (int k = 0; k < n_pages; ++k) {
        const int64_t n = node_off[k + 1] - node_off[k];
        pair_off[k + 1] = pair_off[k] + n * n;
    }
    std::vector<int32_t> edge_blk, pair_blk;
    if (!block_table(n_pages, [&](int k) { return (int64_t)edge_off[k + 1] - edge_off[k]; }, edge_blk) ||
        (out_pairs && !block_table(n_pages, [&](int k) { return pair_off[k + 1] - pair_off[k]; }, pair_blk))) {
        set_error("%s: more than 2^31 blocks of %d edges or pairs in one call", FN, EF_BLOCK);
        return ASEP_ERR_ARG;
    }
    const bool flags = out_flags && n_edges, do_hulls = hulls && n_edges && hull_cap, pairs = out_pairs && pair_off[n_pages];
    if (!flags && !do_hulls && !pairs) return ASEP_OK;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    const int n_node_pts = n_nodes ? node_pt_off[n_nodes] : 0, n_sep_pts = n_seps ? sep_pt_off[n_seps] : 0;
    const int32_t zero = 0;
    int32_t* d_node_off = upload(pool, st, node_off, (size_t)n_pages + 1);
    int32_t* d_node_pt_off = upload(pool, st, n_nodes ? node_pt_off : &zero, (size_t)n_nodes + 1);
    int2* d_node_pts = (int2*)upload(pool, st, node_pts, (size_t)n_node_pts * 2);
    int32_t* d_sep_off = upload(pool, st, sep_off, (size_t)n_pages + 1);
    int32_t* d_sep_pt_off = upload(pool, st, n_seps ? sep_pt_off : &zero, (size_t)n_seps + 1);
    int2* d_sep_pts = (int2*)upload(pool, st, sep_pts, (size_t)n_sep_pts * 2);
    uint8_t* d_sep_orient = upload(pool, st, sep_orient, (size_t)n_seps);
    int32_t* d_edge_off = upload(pool, st, edge_off, (size_t)n_pages + 1);
    int2* d_edges = (int2*)upload(pool, st, edges, (size_t)n_edges * 2);
    EfBox* d_node_box = (EfBox*)pool.get(std::max<size_t>(1, (size_t)n_nodes) * sizeof(EfBox));
    EfBox* d_sep_box = (EfBox*)pool.get(std::max<size_t>(1, (size_t)n_seps) * sizeof(EfBox));
    int32_t* d_edge_blk = upload(pool, st, edge_blk.data(), edge_blk.size());
    uchar2* d_flags = flags ? (uchar2*)pool.get((size_t)n_edges * 2) : nullptr;
    uint8_t *d_heading = nullptr, *d_pairs = nullptr;
    int32_t* d_pair_blk = nullptr;
    int64_t* d_pair_off = nullptr;
    if (pairs) {
        d_heading = upload(pool, st, node_heading, (size_t)n_nodes);
        d_pair_blk = upload(pool, st, pair_blk.data(), pair_blk.size());
        d_pair_off = upload(pool, st, pair_off.data(), pair_off.size());
        d_pairs = (uint8_t*)pool.get((size_t)pair_off[n_pages]);
    }
    int2 *d_sorted = nullptr, *d_work = nullptr;
    int32_t* d_hull_n = nullptr;
    if (do_hulls) {
        d_sorted = (int2*)pool.get((size_t)n_node_pts * sizeof(int2));
        d_work = (int2*)pool.get((size_t)n_edges * 2 * hull_cap * sizeof(int2));
        d_hull_n = (int32_t*)pool.get((size_t)n_edges * sizeof(int32_t));
    }
    LaunchLog log;
    KernelTimer tm;
    tm.start(st);
    if (n_nodes && (flags || pairs)) {
        const unsigned blocks = (unsigned)cdiv(n_nodes, EF_BLOCK);
        edge_boxes_kernel<<<blocks, EF_BLOCK, 0, st>>>(d_node_pt_off, d_node_pts, n_nodes, d_node_box);
        ASEP_HIP_CHECK(hipGetLastError());
        log.add("edge_boxes_kernel", blocks);
    }
    if (n_seps && (flags || pairs)) {
        const unsigned blocks = (unsigned)cdiv(n_seps, EF_BLOCK);
        edge_boxes_kernel<<<blocks, EF_BLOCK, 0, st>>>(d_sep_pt_off, d_sep_pts, n_seps, d_sep_box);
        ASEP_HIP_CHECK(hipGetLastError());
        log.add("edge_boxes_kernel", blocks);
    }
    if (flags) {
        const unsigned blocks = (unsigned)edge_blk[n_pages];
        if (rule == ASEP_EDGE_RULE_BB)
            edge_flags_kernel<EF_RULE_BB><<<blocks, EF_BLOCK, 0, st>>>(d_edge_blk, n_pages, d_node_off, d_node_box, d_sep_off, d_sep_box,
                                                                     d_sep_pt_off, d_sep_pts, d_sep_orient, d_edge_off, d_edges, d_flags);
        else
            edge_flags_kernel<EF_RULE_LINE><<<blocks, EF_BLOCK, 0, st>>>(d_edge_blk, n_pages, d_node_off, d_node_box, d_sep_off, d_sep_box,
                                                                       d_sep_pt_off, d_sep_pts, d_sep_orient, d_edge_off, d_edges, d_flags);
        ASEP_HIP_CHECK(hipGetLastError());
        log.add(rule == ASEP_EDGE_RULE_BB ? "edge_flags_kernel<bb>" : "edge_flags_kernel<line>", blocks);
    }
    if (pairs) {
        const unsigned blocks = (unsigned)pair_blk[n_pages];
        edge_pair_bits_kernel<<<blocks, EF_BLOCK, 0, st>>>(d_pair_blk, n_pages, d_node_off, d_node_box, d_heading, d_sep_off, d_sep_box,
                                                         d_sep_pt_off, d_sep_orient, d_pair_off, d_pairs);
        ASEP_HIP_CHECK(hipGetLastError());
        log.add("edge_pair_bits_kernel", blocks);
    }
    if (do_hulls) {
        edge_sort_points_kernel<<<(unsigned)n_nodes, EF_WAVE, 0, st>>>(d_node_pt_off, d_node_pts, d_sorted);
        ASEP_HIP_CHECK(hipGetLastError());
        log.add("edge_sort_points_kernel", (unsigned)n_nodes);
        const unsigned blocks = (unsigned)cdiv(n_edges, EF_BLOCK);
        edge_hull_kernel<<<blocks, EF_BLOCK, 0, st>>>(d_edge_off, n_pages, d_node_off, d_node_pt_off, d_sorted, d_edges, hull_cap, d_work,
                                                    d_hull_n);
        ASEP_HIP_CHECK(hipGetLastError());
        log.add("edge_hull_kernel", blocks);
    }
    tm.stop(st);
    if (flags) ASEP_HIP_CHECK(hipMemcpyAsync(out_flags, d_flags, (size_t)n_edges * 2, hipMemcpyDeviceToHost, st));
    if (pairs) ASEP_HIP_CHECK(hipMemcpyAsync(out_pairs, d_pairs, (size_t)pair_off[n_pages], hipMemcpyDeviceToHost, st));
    if (do_hulls) {
        // the output rows are the first hull_cap entries of the 2 * hull_cap wide working rows
        const size_t row = (size_t)hull_cap * sizeof(int2);
        ASEP_HIP_CHECK(hipMemcpy2DAsync(out_hull, row, d_work, 2 * row, row, (size_t)n_edges, hipMemcpyDeviceToHost, st));
        ASEP_HIP_CHECK(hipMemcpyAsync(out_hull_n, d_hull_n, (size_t)n_edges * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tm.read(g_kernel_us);
    g_launches = log.done();
    return ASEP_OK;
    ASEP_GUARD_END
}
