// Host side of the clustering grid (include/asep_hip.h, "clustering grid" block): two entry points on the asep_post handle
// (its stream and buffer pool), dbscan alone and the three methods mixed.  Compiled with -ffp-contract=off, like the kernels it launches.
#include <algorithm>
#include <vector>

#include "asep_common.h"
#include "batch_tables.h"
#include "cluster_grid_kernels.h"

using namespace asep;

static_assert(sizeof(asep_cluster_setting) == sizeof(ClgSetting) && sizeof(ClgSetting) == 24, "asep_cluster_setting layout");
static_assert(sizeof(asep_cluster_method_setting) == sizeof(ClgMethodSetting) && sizeof(ClgMethodSetting) == 32,
              "asep_cluster_method_setting layout");

namespace {

thread_local double g_kernel_us = 0.0;   // device time of this thread's last clustering grid call (all its kernels)

// The pages of a call: node_off checked, the largest page, the offsets of the pages' matrices in a matrix set.
struct Pages {
    int n_nodes = 0, max_n = 0;
    bool two_nodes = false;             // some page follows calc()'s rule for two nodes
    std::vector<int64_t> conf_off;
};

bool check_pages(const char* fn, int n_pages, const int32_t* node_off, Pages& pg) {
    if (!check_offsets(fn, "node_off", node_off, n_pages)) return false;
    pg.n_nodes = node_off[n_pages];
    pg.conf_off.assign((size_t)n_pages + 1, 0);
    for (int k = 0; k < n_pages; ++k) {
        const int n = node_off[k + 1] - node_off[k];
        if (n > CLG_MAX_NODES) {
            set_error("%s: page %d has %d nodes, the engine clusters at most %d (labels, owner queue and member values of a page "
                      "sit in LDS)", fn, k, n, CLG_MAX_NODES);
            return false;
        }
        pg.max_n = std::max(pg.max_n, n);
        pg.two_nodes = pg.two_nodes || n == 2;
        pg.conf_off[k + 1] = pg.conf_off[k] + (int64_t)n * n;
    }
    return true;
}

// The six comparison tables of a call (all or none) and their device copies.
struct CompareTables {
    const int32_t *line_off, *line_node, *line_gt, *gtblk_off, *gtblk_line_off, *gtblk_lines;
    int n_lines = 0, n_blk = 0, n_ent = 0;
    int32_t *d_line_off = nullptr, *d_line_node = nullptr, *d_line_gt = nullptr, *d_blk_off = nullptr, *d_blk_line_off = nullptr,
            *d_blk_lines = nullptr;

    bool given(const int32_t* out_counts) const {
        return line_off || line_node || line_gt || gtblk_off || gtblk_line_off || gtblk_lines || out_counts;
    }

    bool check(const char* fn, int n_pages, const int32_t* node_off, bool want_counts, const int32_t* out_counts) {
        if (!line_off || !gtblk_off || !gtblk_line_off || (want_counts && !out_counts)) {
            set_error("%s: the comparison needs line_off, gtblk_off, gtblk_line_off and out_counts (all six tables or none)", fn);
            return false;
        }
        if (!check_offsets(fn, "line_off", line_off, n_pages) || !check_offsets(fn, "gtblk_off", gtblk_off, n_pages)) return false;
        n_lines = line_off[n_pages];
        n_blk = gtblk_off[n_pages];
        if (!check_offsets(fn, "gtblk_line_off", gtblk_line_off, n_blk)) return false;
        n_ent = gtblk_line_off[n_blk];
        if ((n_lines && (!line_node || !line_gt)) || (n_ent && !gtblk_lines)) {
            set_error("%s: null argument (line_node, line_gt or gtblk_lines)", fn);
            return false;
        }
        for (int k = 0; k < n_pages; ++k) {
            const int n = node_off[k + 1] - node_off[k], l0 = line_off[k], nl = line_off[k + 1] - l0;
            for (int i = 0; i < nl; ++i) {
                if (line_node[l0 + i] < 0 || line_node[l0 + i] >= n) {
                    set_error("%s: line %d of page %d hangs in node %d, the page has %d nodes", fn, i, k, line_node[l0 + i], n);
                    return false;
                }
                if (line_gt[l0 + i] < -1 || line_gt[l0 + i] >= nl) {
                    set_error("%s: line %d of page %d has ground truth article %d, not a dense index below its %d lines or -1", fn, i,
                              k, line_gt[l0 + i], nl);
                    return false;
                }
            }
        }
        return check_members(fn, "ground truth block", n_pages, line_off, gtblk_off, gtblk_line_off, gtblk_lines);
    }

    void upload_all(BufferPool& pool, hipStream_t st, int n_pages) {
        d_line_off = upload(pool, st, line_off, (size_t)n_pages + 1);
        d_line_node = upload(pool, st, line_node, (size_t)n_lines);
        d_line_gt = upload(pool, st, line_gt, (size_t)n_lines);
        d_blk_off = upload(pool, st, gtblk_off, (size_t)n_pages + 1);
        d_blk_line_off = upload(pool, st, gtblk_line_off, (size_t)n_blk + 1);
        d_blk_lines = upload(pool, st, gtblk_lines, (size_t)n_ent);
    }

    void launch(hipStream_t st, unsigned blocks, const int32_t* d_labels, const int32_t* d_node_off, int n_settings, int n_pages,
                int max_n, int4* d_counts) const {
        cluster_compare_kernel<<<blocks, CLG_WAVE, (size_t)(max_n + 2) * 8, st>>>(d_labels, d_node_off, d_line_off, d_line_node,
                                                                                d_line_gt, d_blk_off, d_blk_line_off, d_blk_lines,
                                                                                n_settings, n_pages, max_n, d_counts);
    }
};

// one matrix set of the pages on the device (nullptr for a set the caller left out)
void* upload_mats(BufferPool& pool, hipStream_t st, const void* host, int64_t count, size_t esz) {
    if (!host) return nullptr;
    void* d = pool.get(std::max<size_t>(1, (size_t)count * esz));
    if (count) ASEP_HIP_CHECK_THROW(hipMemcpyAsync(d, host, (size_t)count * esz, hipMemcpyHostToDevice, st));
    return d;
}

// The kernels of asep_cluster_grid_run_methods in the matrix dtype T: each method over its own settings (sel_*: their indices
// in the call's list, on the device), then the comparison and rel_LLH over all of them.
template <class T>
void launch_methods(hipStream_t st, const Pages& pg, int n_pages, const T* d_conf, const T* d_dist, const T* d_delta,
                    const int64_t* d_conf_off, const int32_t* d_node_off, const ClgSetting* d_dbscan, const ClgMethodSetting* d_set,
                    const int32_t* const d_sel[3], const int n_sel[3], T* d_work, int32_t* d_labels) {
    const int max_n = pg.max_n;
    if (n_sel[CLG_DBSCAN])
        cluster_grid_kernel<T><<<(unsigned)n_pages * n_sel[CLG_DBSCAN], CLG_WAVE, (size_t)max_n * (sizeof(T) + 8), st>>>(
            d_conf, d_conf_off, d_node_off, d_dbscan, n_sel[CLG_DBSCAN], n_pages, max_n, d_sel[CLG_DBSCAN], d_labels);
    if (n_sel[CLG_DBSCAN_STD])
        cluster_std_kernel<T><<<(unsigned)n_pages * n_sel[CLG_DBSCAN_STD], CLG_WAVE, (size_t)max_n * 9, st>>>(
            d_conf, d_dist, d_conf_off, d_node_off, d_set, d_sel[CLG_DBSCAN_STD], n_sel[CLG_DBSCAN_STD], n_pages, max_n, d_labels);
    if (n_sel[CLG_GREEDY])
        cluster_greedy_kernel<T><<<(unsigned)n_pages * n_sel[CLG_GREEDY], CLG_WAVE, (size_t)max_n * (sizeof(T) + 8), st>>>(
            d_conf, d_delta, d_conf_off, d_node_off, d_set, d_sel[CLG_GREEDY], n_sel[CLG_GREEDY], n_pages, max_n, d_work, d_labels);
}

}  // namespace

double asep_cluster_grid_last_kernel_us(void) { return g_kernel_us; }

int asep_cluster_grid_max_nodes(void) { return CLG_MAX_NODES; }

int asep_cluster_grid_run(asep_post* p, int n_pages, const int32_t* node_off, const void* conf, int conf_is_f64, int n_settings,
                          const asep_cluster_setting* settings, const int32_t* line_off, const int32_t* line_node,
                          const int32_t* line_gt, const int32_t* gtblk_off, const int32_t* gtblk_line_off,
                          const int32_t* gtblk_lines, int32_t* out_labels, int32_t* out_counts) {
    const char* const FN = "asep_cluster_grid_run";
    g_kernel_us = 0.0;
    if (!p || n_pages < 0 || n_settings < 0 || !node_off || (n_settings && !settings)) {
        set_error("%s: bad arguments (n_pages %d >= 0, n_settings %d >= 0, handle, node_off and settings given)", FN, n_pages,
                  n_settings);
        return ASEP_ERR_ARG;
    }
    if ((long long)n_pages * n_settings > CLG_MAX_PROBLEMS) {
        set_error("%s: %d pages x %d settings are more than the %d problems one launch holds", FN, n_pages, n_settings,
                  CLG_MAX_PROBLEMS);
        return ASEP_ERR_ARG;
    }
    Pages pg;
    if (!check_pages(FN, n_pages, node_off, pg)) return ASEP_ERR_ARG;
    const int n_nodes = pg.n_nodes, max_n = pg.max_n;
    const std::vector<int64_t>& conf_off = pg.conf_off;
    CompareTables tb{line_off, line_node, line_gt, gtblk_off, gtblk_line_off, gtblk_lines};
    const bool compare = tb.given(out_counts);
    if ((conf_off[n_pages] && !conf) || (n_settings && n_nodes && !out_labels && !compare)) {
        set_error("%s: null argument (conf or out_labels)", FN);
        return ASEP_ERR_ARG;
    }
    if (compare && !tb.check(FN, n_pages, node_off, n_settings && n_pages, out_counts)) return ASEP_ERR_ARG;
    if (n_settings == 0 || n_pages == 0) return ASEP_OK;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    const size_t esz = conf_is_f64 ? sizeof(double) : sizeof(float);
    void* d_conf = pool.get(std::max<size_t>(1, (size_t)conf_off[n_pages] * esz));
    if (conf_off[n_pages])
        ASEP_HIP_CHECK(hipMemcpyAsync(d_conf, conf, (size_t)conf_off[n_pages] * esz, hipMemcpyHostToDevice, st));
    int64_t* d_conf_off = upload(pool, st, conf_off.data(), conf_off.size());
    int32_t* d_node_off = upload(pool, st, node_off, (size_t)n_pages + 1);
    ClgSetting* d_set = upload(pool, st, (const ClgSetting*)settings, (size_t)n_settings);
    const size_t label_bytes = (size_t)n_settings * n_nodes * sizeof(int32_t);
    int32_t* d_labels = (int32_t*)pool.get(std::max<size_t>(4, label_bytes));
    int4* d_counts = nullptr;
    const size_t count_bytes = (size_t)n_settings * n_pages * 4 * sizeof(int32_t);
    if (compare) {
        tb.upload_all(pool, st, n_pages);
        d_counts = (int4*)pool.get(count_bytes);
    }
    const unsigned blocks = (unsigned)n_pages * (unsigned)n_settings;
    KernelTimer tm;
    tm.start(st);
    if (conf_is_f64)
        cluster_grid_kernel<double><<<blocks, CLG_WAVE, (size_t)max_n * (sizeof(double) + 8), st>>>(
            (const double*)d_conf, d_conf_off, d_node_off, d_set, n_settings, n_pages, max_n, nullptr, d_labels);
    else
        cluster_grid_kernel<float><<<blocks, CLG_WAVE, (size_t)max_n * (sizeof(float) + 8), st>>>(
            (const float*)d_conf, d_conf_off, d_node_off, d_set, n_settings, n_pages, max_n, nullptr, d_labels);
    ASEP_HIP_CHECK(hipGetLastError());
    if (compare) {
        tb.launch(st, blocks, d_labels, d_node_off, n_settings, n_pages, max_n, d_counts);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    tm.stop(st);
    if (out_labels && label_bytes) ASEP_HIP_CHECK(hipMemcpyAsync(out_labels, d_labels, label_bytes, hipMemcpyDeviceToHost, st));
    if (compare) ASEP_HIP_CHECK(hipMemcpyAsync(out_counts, d_counts, count_bytes, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tm.read(g_kernel_us);
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_cluster_grid_run_methods(asep_post* p, int n_pages, const int32_t* node_off, int mats_are_f64, const void* conf,
                                  const void* dist, const void* delta, int n_settings,
                                  const asep_cluster_method_setting* settings, const int32_t* line_off, const int32_t* line_node,
                                  const int32_t* line_gt, const int32_t* gtblk_off, const int32_t* gtblk_line_off,
                                  const int32_t* gtblk_lines, int32_t* out_labels, int32_t* out_counts, double* out_llh) {
    const char* const FN = "asep_cluster_grid_run_methods";
    g_kernel_us = 0.0;
    if (!p || n_pages < 0 || n_settings < 0 || !node_off || (n_settings && !settings)) {
        set_error("%s: bad arguments (n_pages %d >= 0, n_settings %d >= 0, handle, node_off and settings given)", FN, n_pages,
                  n_settings);
        return ASEP_ERR_ARG;
    }
    if ((long long)n_pages * n_settings > CLG_MAX_PROBLEMS) {
        set_error("%s: %d pages x %d settings are more than the %d problems one launch holds", FN, n_pages, n_settings,
                  CLG_MAX_PROBLEMS);
        return ASEP_ERR_ARG;
    }
    // the settings of each method, in the order of the list
    std::vector<int32_t> sel[3];
    std::vector<ClgSetting> dbscan;
    for (int s = 0; s < n_settings; ++s) {
        const asep_cluster_method_setting& m = settings[s];
        if (m.method != CLG_DBSCAN && m.method != CLG_DBSCAN_STD && m.method != CLG_GREEDY) {
            set_error("%s: setting %d has method %d, not ASEP_CLUSTER_DBSCAN (0), _DBSCAN_STD (1) or _GREEDY (2)", FN, s, m.method);
            return ASEP_ERR_ARG;
        }
        sel[m.method].push_back(s);
        if (m.method == CLG_DBSCAN) dbscan.push_back(ClgSetting{m.count, m.assign_noise, m.conf_thr, m.param});
    }
    Pages pg;
    if (!check_pages(FN, n_pages, node_off, pg)) return ASEP_ERR_ARG;
    const int64_t n_values = pg.conf_off[n_pages];
    CompareTables tb{line_off, line_node, line_gt, gtblk_off, gtblk_line_off, gtblk_lines};
    const bool compare = tb.given(out_counts);
    if (n_values) {
        const char* missing = nullptr;
        if (!conf && (!sel[CLG_DBSCAN].empty() || (n_settings && pg.two_nodes)))
            missing = "conf (a dbscan setting, or a page of two nodes under any setting, reads it)";
        else if (!dist && !sel[CLG_DBSCAN_STD].empty())
            missing = "dist (_dist_mat: a dbscan_std setting reads it)";
        else if (!delta && !sel[CLG_GREEDY].empty())
            missing = "delta (_delta_mat: a greedy setting reads it)";
        else if (!delta && out_llh && n_settings)
            missing = "delta (_delta_mat: out_llh is computed from it)";
        if (missing) {
            set_error("%s: missing matrix set %s", FN, missing);
            return ASEP_ERR_ARG;
        }
    }
    if (n_settings && pg.n_nodes && !out_labels && !compare && !out_llh) {
        set_error("%s: null argument (out_labels, and neither out_counts nor out_llh asked for)", FN);
        return ASEP_ERR_ARG;
    }
    if (compare && !tb.check(FN, n_pages, node_off, n_settings && n_pages, out_counts)) return ASEP_ERR_ARG;
    if (n_settings == 0 || n_pages == 0) return ASEP_OK;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    const size_t esz = mats_are_f64 ? sizeof(double) : sizeof(float);
    void* d_conf = upload_mats(pool, st, conf, n_values, esz);
    void* d_dist = upload_mats(pool, st, dist, n_values, esz);
    void* d_delta = upload_mats(pool, st, delta, n_values, esz);
    int64_t* d_conf_off = upload(pool, st, pg.conf_off.data(), pg.conf_off.size());
    int32_t* d_node_off = upload(pool, st, node_off, (size_t)n_pages + 1);
    ClgMethodSetting* d_set = upload(pool, st, (const ClgMethodSetting*)settings, (size_t)n_settings);
    ClgSetting* d_dbscan = upload(pool, st, dbscan.data(), dbscan.size());
    const int32_t* d_sel[3];
    int n_sel[3];
    for (int m = 0; m < 3; ++m) {
        d_sel[m] = upload(pool, st, sel[m].data(), sel[m].size());
        n_sel[m] = (int)sel[m].size();
    }
    // greedy's working matrices: one copy of the page's _delta_mat per greedy setting
    void* d_work = pool.get(std::max<size_t>(1, (size_t)n_values * sel[CLG_GREEDY].size() * esz));
    const size_t label_bytes = (size_t)n_settings * pg.n_nodes * sizeof(int32_t);
    int32_t* d_labels = (int32_t*)pool.get(std::max<size_t>(4, label_bytes));
    int4* d_counts = nullptr;
    const size_t count_bytes = (size_t)n_settings * n_pages * 4 * sizeof(int32_t);
    if (compare) {
        tb.upload_all(pool, st, n_pages);
        d_counts = (int4*)pool.get(count_bytes);
    }
    const size_t llh_bytes = (size_t)n_settings * n_pages * sizeof(double);
    double* d_llh = out_llh ? (double*)pool.get(llh_bytes) : nullptr;
    const unsigned blocks = (unsigned)n_pages * (unsigned)n_settings;
    KernelTimer tm;
    tm.start(st);
    if (mats_are_f64)
        launch_methods<double>(st, pg, n_pages, (const double*)d_conf, (const double*)d_dist, (const double*)d_delta,
                               d_conf_off, d_node_off, d_dbscan, d_set, d_sel, n_sel, (double*)d_work, d_labels);
    else
        launch_methods<float>(st, pg, n_pages, (const float*)d_conf, (const float*)d_dist, (const float*)d_delta,
                              d_conf_off, d_node_off, d_dbscan, d_set, d_sel, n_sel, (float*)d_work, d_labels);
    ASEP_HIP_CHECK(hipGetLastError());
    if (compare) {
        tb.launch(st, blocks, d_labels, d_node_off, n_settings, n_pages, pg.max_n, d_counts);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    if (out_llh) {
        if (mats_are_f64)
            cluster_llh_kernel<double><<<blocks, CLG_WAVE, 0, st>>>(d_labels, (const double*)d_delta, d_conf_off, d_node_off,
                                                                    n_settings, n_pages, d_llh);
        else
            cluster_llh_kernel<float><<<blocks, CLG_WAVE, 0, st>>>(d_labels, (const float*)d_delta, d_conf_off, d_node_off, n_settings,
                                                                   n_pages, d_llh);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    tm.stop(st);
    if (out_labels && label_bytes) ASEP_HIP_CHECK(hipMemcpyAsync(out_labels, d_labels, label_bytes, hipMemcpyDeviceToHost, st));
    if (compare) ASEP_HIP_CHECK(hipMemcpyAsync(out_counts, d_counts, count_bytes, hipMemcpyDeviceToHost, st));
    if (out_llh) ASEP_HIP_CHECK(hipMemcpyAsync(out_llh, d_llh, llh_bytes, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tm.read(g_kernel_us);
    return ASEP_OK;
    ASEP_GUARD_END
}
