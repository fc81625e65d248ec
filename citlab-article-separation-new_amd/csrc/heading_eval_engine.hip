// Host side of the heading detection grid scoring (include/asep_hip.h, "heading detection evaluation" block): one entry
// point on the asep_post handle (its stream and buffer pool).  Compiled with -ffp-contract=off, like the kernel it launches.
#include <vector>

#include "asep_common.h"
#include "batch_tables.h"
#include "heading_eval_kernels.h"

using namespace asep;

namespace {

const char* const FN = "asep_heading_grid_eval";

thread_local double g_kernel_us = 0.0;   // device time of this thread's last asep_heading_grid_eval launch

}  // namespace

double asep_heading_grid_last_kernel_us(void) { return g_kernel_us; }

int asep_heading_grid_eval(asep_post* p, int n_pages, const int32_t* line_off, const double* sw_conf, const double* th_conf,
                           const double* net_conf, const uint8_t* line_tagged, const uint8_t* use_swt, const int32_t* reg_off,
                           const int32_t* reg_line_off, const int32_t* reg_lines, const uint8_t* gt_heading, int n_settings,
                           const int32_t* settings, int32_t* out_counts) {
    g_kernel_us = 0.0;
    if (!p || n_pages < 0 || n_pages > 65535 || n_settings < 0 || !line_off || !reg_off || !reg_line_off) {
        set_error("asep_heading_grid_eval: bad arguments (n_pages %d in 0..65535, n_settings %d >= 0, offsets given)", n_pages,
                  n_settings);
        return ASEP_ERR_ARG;
    }
    const int n_lines = line_off[n_pages], n_regs = reg_off[n_pages];
    if (n_lines < 0 || n_regs < 0 || !check_offsets(FN, "line_off", line_off, n_pages) ||
        !check_offsets(FN, "reg_off", reg_off, n_pages))
        return ASEP_ERR_ARG;
    const int n_ent = reg_line_off[n_regs];
    if (n_ent < 0 || !check_offsets(FN, "reg_line_off", reg_line_off, n_regs)) return ASEP_ERR_ARG;
    if ((n_lines && (!sw_conf || !th_conf || !net_conf)) || (n_ent && !reg_lines) || (n_regs && !gt_heading) ||
        (n_pages && !use_swt) || (n_settings && (!settings || (n_pages && !out_counts)))) {
        set_error("asep_heading_grid_eval: null argument");
        return ASEP_ERR_ARG;
    }
    for (long long i = 0; i < (long long)n_settings * HEVAL_FIELDS; ++i)
        if (settings[i] < 0 || settings[i] > 10) {
            set_error("asep_heading_grid_eval: setting %lld field %lld is %d, not a number of tenths in 0..10", i / HEVAL_FIELDS,
                      i % HEVAL_FIELDS, settings[i]);
            return ASEP_ERR_ARG;
        }
    if (!check_members(FN, "region", n_pages, line_off, reg_off, reg_line_off, reg_lines)) return ASEP_ERR_ARG;
    ASEP_GUARD_BEGIN
    // the lines of each region, in region order, as entries the kernel walks from front to back (a page's regions are consecutive)
    std::vector<HevalEntry> ent((size_t)n_ent);
    for (int k = 0; k < n_pages; ++k) {
        const int l0 = line_off[k];
        for (int e = reg_line_off[reg_off[k]]; e < reg_line_off[reg_off[k + 1]]; ++e) {
            const int i = l0 + reg_lines[e];
            ent[e] = HevalEntry{sw_conf[i], th_conf[i], net_conf[i], line_tagged ? (line_tagged[i] != 0) : 0, 0};
        }
    }
    if (n_settings == 0 || n_pages == 0) return ASEP_OK;
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    HevalEntry* d_ent = upload(pool, st, ent.data(), ent.size());
    int32_t* d_reg_ent = upload(pool, st, reg_line_off, (size_t)n_regs + 1);
    int32_t* d_reg_page = upload(pool, st, reg_off, (size_t)n_pages + 1);
    std::vector<uint8_t> gt((size_t)n_regs), swt((size_t)n_pages);
    for (int r = 0; r < n_regs; ++r) gt[r] = gt_heading[r] != 0;
    for (int k = 0; k < n_pages; ++k) swt[k] = use_swt[k] != 0;
    uint8_t* d_gt = upload(pool, st, gt.data(), gt.size());
    uint8_t* d_swt = upload(pool, st, swt.data(), swt.size());
    int32_t* d_set = upload(pool, st, settings, (size_t)n_settings * HEVAL_FIELDS);
    const size_t out_bytes = (size_t)n_settings * n_pages * 4 * sizeof(int32_t);
    int4* d_out = (int4*)pool.get(out_bytes);
    KernelTimer tm;
    tm.start(st);
    heval_grid_kernel<<<dim3((unsigned)cdiv(n_settings, HEVAL_BLOCK), (unsigned)n_pages), HEVAL_BLOCK, 0, st>>>(
        d_ent, d_reg_ent, d_reg_page, d_gt, d_swt, d_set, n_settings, n_pages, d_out);
    ASEP_HIP_CHECK(hipGetLastError());
    tm.stop(st);
    ASEP_HIP_CHECK(hipMemcpyAsync(out_counts, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tm.read(g_kernel_us);
    return ASEP_OK;
    ASEP_GUARD_END
}
