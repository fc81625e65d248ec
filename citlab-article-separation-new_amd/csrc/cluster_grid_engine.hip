// Host side of the clustering grid (include/asep_hip.h, "clustering grid" block): one entry point on the asep_post handle
// (its stream and buffer pool).  Compiled with -ffp-contract=off, like the kernels it launches.
#include <algorithm>
#include <vector>

#include "asep_common.h"
#include "batch_tables.h"
#include "cluster_grid_kernels.h"

using namespace asep;

static_assert(sizeof(asep_cluster_setting) == sizeof(ClgSetting) && sizeof(ClgSetting) == 24, "asep_cluster_setting layout");

namespace {

const char* const FN = "asep_cluster_grid_run";

thread_local double g_kernel_us = 0.0;   // device time of this thread's last asep_cluster_grid_run (both kernels)

}  // namespace

double asep_cluster_grid_last_kernel_us(void) { return g_kernel_us; }

int asep_cluster_grid_max_nodes(void) { return CLG_MAX_NODES; }

int asep_cluster_grid_run(asep_post* p, int n_pages, const int32_t* node_off, const void* conf, int conf_is_f64, int n_settings,
                          const asep_cluster_setting* settings, const int32_t* line_off, const int32_t* line_node,
                          const int32_t* line_gt, const int32_t* gtblk_off, const int32_t* gtblk_line_off,
                          const int32_t* gtblk_lines, int32_t* out_labels, int32_t* out_counts) {
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
    if (!check_offsets(FN, "node_off", node_off, n_pages)) return ASEP_ERR_ARG;
    const int n_nodes = node_off[n_pages];
    int max_n = 0;
    std::vector<int64_t> conf_off((size_t)n_pages + 1, 0);
    for (int k = 0; k < n_pages; ++k) {
        const int n = node_off[k + 1] - node_off[k];
        if (n > CLG_MAX_NODES) {
            set_error("%s: page %d has %d nodes, the engine clusters at most %d (labels, owner queue and member values of a page "
                      "sit in LDS)", FN, k, n, CLG_MAX_NODES);
            return ASEP_ERR_ARG;
        }
        max_n = std::max(max_n, n);
        conf_off[k + 1] = conf_off[k] + (int64_t)n * n;
    }
    const bool compare = line_off || line_node || line_gt || gtblk_off || gtblk_line_off || gtblk_lines || out_counts;
    if ((conf_off[n_pages] && !conf) || (n_settings && n_nodes && !out_labels && !compare)) {
        set_error("%s: null argument (conf or out_labels)", FN);
        return ASEP_ERR_ARG;
    }
    int n_lines = 0, n_blk = 0, n_ent = 0;
    if (compare) {
        if (!line_off || !gtblk_off || !gtblk_line_off || (n_settings && n_pages && !out_counts)) {
            set_error("%s: the comparison needs line_off, gtblk_off, gtblk_line_off and out_counts (all six tables or none)", FN);
            return ASEP_ERR_ARG;
        }
        if (!check_offsets(FN, "line_off", line_off, n_pages) || !check_offsets(FN, "gtblk_off", gtblk_off, n_pages))
            return ASEP_ERR_ARG;
        n_lines = line_off[n_pages];
        n_blk = gtblk_off[n_pages];
        if (!check_offsets(FN, "gtblk_line_off", gtblk_line_off, n_blk)) return ASEP_ERR_ARG;
        n_ent = gtblk_line_off[n_blk];
        if ((n_lines && (!line_node || !line_gt)) || (n_ent && !gtblk_lines)) {
            set_error("%s: null argument (line_node, line_gt or gtblk_lines)", FN);
            return ASEP_ERR_ARG;
        }
        for (int k = 0; k < n_pages; ++k) {
            const int n = node_off[k + 1] - node_off[k], l0 = line_off[k], nl = line_off[k + 1] - l0;
            for (int i = 0; i < nl; ++i) {
                if (line_node[l0 + i] < 0 || line_node[l0 + i] >= n) {
                    set_error("%s: line %d of page %d hangs in node %d, the page has %d nodes", FN, i, k, line_node[l0 + i], n);
                    return ASEP_ERR_ARG;
                }
                if (line_gt[l0 + i] < -1 || line_gt[l0 + i] >= nl) {
                    set_error("%s: line %d of page %d has ground truth article %d, not a dense index below its %d lines or -1", FN, i,
                              k, line_gt[l0 + i], nl);
                    return ASEP_ERR_ARG;
                }
            }
        }
        if (!check_members(FN, "ground truth block", n_pages, line_off, gtblk_off, gtblk_line_off, gtblk_lines)) return ASEP_ERR_ARG;
    }
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
    int32_t *d_line_off = nullptr, *d_line_node = nullptr, *d_line_gt = nullptr, *d_blk_off = nullptr, *d_blk_line_off = nullptr,
            *d_blk_lines = nullptr;
    int4* d_counts = nullptr;
    const size_t count_bytes = (size_t)n_settings * n_pages * 4 * sizeof(int32_t);
    if (compare) {
        d_line_off = upload(pool, st, line_off, (size_t)n_pages + 1);
        d_line_node = upload(pool, st, line_node, (size_t)n_lines);
        d_line_gt = upload(pool, st, line_gt, (size_t)n_lines);
        d_blk_off = upload(pool, st, gtblk_off, (size_t)n_pages + 1);
        d_blk_line_off = upload(pool, st, gtblk_line_off, (size_t)n_blk + 1);
        d_blk_lines = upload(pool, st, gtblk_lines, (size_t)n_ent);
        d_counts = (int4*)pool.get(count_bytes);
    }
    const unsigned blocks = (unsigned)n_pages * (unsigned)n_settings;
    KernelTimer tm;
    tm.start(st);
    if (conf_is_f64)
        cluster_grid_kernel<double><<<blocks, CLG_WAVE, (size_t)max_n * (sizeof(double) + 8), st>>>(
            (const double*)d_conf, d_conf_off, d_node_off, d_set, n_settings, n_pages, max_n, d_labels);
    else
        cluster_grid_kernel<float><<<blocks, CLG_WAVE, (size_t)max_n * (sizeof(float) + 8), st>>>(
            (const float*)d_conf, d_conf_off, d_node_off, d_set, n_settings, n_pages, max_n, d_labels);
    ASEP_HIP_CHECK(hipGetLastError());
    if (compare) {
        cluster_compare_kernel<<<blocks, CLG_WAVE, (size_t)(max_n + 2) * 8, st>>>(d_labels, d_node_off, d_line_off, d_line_node,
                                                                                d_line_gt, d_blk_off, d_blk_line_off, d_blk_lines,
                                                                                n_settings, n_pages, max_n, d_counts);
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
