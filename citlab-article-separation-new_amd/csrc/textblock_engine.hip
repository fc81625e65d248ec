// Host side of the text block detection stage (include/asep_hip.h, "text block detection" block): batched entry points
// on the asep_post handle (its stream and buffer pool).  Compiled with -ffp-contract=off, like the kernels it launches.
#include <vector>

#include "asep_common.h"
#include "textblock_kernels.h"

using namespace asep;

namespace {

// page_off must start at 0, never decrease and end at n_polys; poly_off likewise over the points, every polygon
// holding at least one point (the reference indexes x_points[0] / x_points[-1]).
bool check_offsets(const char* fn, const int32_t* off, int n, int total, bool nonempty) {
    if (off[0] != 0 || off[n] != total) {
        set_error("%s: offsets must run from 0 to %d", fn, total);
        return false;
    }
    for (int k = 0; k < n; ++k) {
        if (off[k + 1] < off[k] + (nonempty ? 1 : 0)) {
            set_error("%s: offset %d (%d -> %d) is %s", fn, k, off[k], off[k + 1], nonempty ? "empty or decreasing" : "decreasing");
            return false;
        }
    }
    return true;
}

// device time of the last kernel of each kind launched by this thread (0 interline distances, 1 neighbours), microseconds
thread_local double g_kernel_us[2] = {0.0, 0.0};

struct KernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~KernelTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int start(hipStream_t st) {
        ASEP_HIP_CHECK(hipEventCreate(&e0));
        ASEP_HIP_CHECK(hipEventCreate(&e1));
        ASEP_HIP_CHECK(hipEventRecord(e0, st));
        return ASEP_OK;
    }
    int stop(hipStream_t st) {
        ASEP_HIP_CHECK(hipEventRecord(e1, st));
        return ASEP_OK;
    }
    int read(double& us) {                             // after the stream has been synchronised
        float ms = 0.f;
        ASEP_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        us = 1000.0 * ms;
        return ASEP_OK;
    }
};

}  // namespace

double asep_textblock_last_kernel_us(int which) { return (which == 0 || which == 1) ? g_kernel_us[which] : -1.0; }

int asep_textblock_interline_dists(asep_post* p, int n_pages, const int32_t* page_off, const int32_t* poly_off,
                                   const int32_t* points, const int32_t* boxes, const double* orient, double des_dist,
                                   double max_d, double* out_dist) {
    if (!p || n_pages < 0 || !page_off || (n_pages > 0 && (!poly_off))) {
        set_error("asep_textblock_interline_dists: bad arguments");
        return ASEP_ERR_ARG;
    }
    const int n_polys = page_off[n_pages];
    if (n_polys < 0 || !check_offsets("asep_textblock_interline_dists", page_off, n_pages, n_polys, false))
        return ASEP_ERR_ARG;
    if (n_polys == 0) return ASEP_OK;
    if (!points || !boxes || !orient || !out_dist) {
        set_error("asep_textblock_interline_dists: null argument");
        return ASEP_ERR_ARG;
    }
    const int n_points = poly_off[n_polys];
    if (!check_offsets("asep_textblock_interline_dists", poly_off, n_polys, n_points, true)) return ASEP_ERR_ARG;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    std::vector<int32_t> range(2 * (size_t)n_polys);
    for (int pg = 0; pg < n_pages; ++pg)
        for (int i = page_off[pg]; i < page_off[pg + 1]; ++i) {
            range[2 * (size_t)i] = page_off[pg];
            range[2 * (size_t)i + 1] = page_off[pg + 1];
        }
    pool.begin();
    int2* d_pts = (int2*)pool.get((size_t)n_points * sizeof(int2));
    int* d_off = (int*)pool.get((size_t)(n_polys + 1) * sizeof(int));
    int4* d_box = (int4*)pool.get((size_t)n_polys * sizeof(int4));
    double2* d_or = (double2*)pool.get((size_t)n_polys * sizeof(double2));
    int2* d_rng = (int2*)pool.get((size_t)n_polys * sizeof(int2));
    double* d_out = (double*)pool.get((size_t)n_polys * sizeof(double));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_pts, points, (size_t)n_points * sizeof(int2), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_off, poly_off, (size_t)(n_polys + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_box, boxes, (size_t)n_polys * sizeof(int4), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_or, orient, (size_t)n_polys * sizeof(double2), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_rng, range.data(), (size_t)n_polys * sizeof(int2), hipMemcpyHostToDevice, st));
    const unsigned blocks = (unsigned)(((size_t)n_polys + 3) / 4);      // four waves (polygons) per 256-thread block
    KernelTimer tm;
    if (int rc = tm.start(st)) return rc;
    tb_interline_kernel<<<blocks, 256, 0, st>>>(d_pts, d_off, d_box, d_or, d_rng, n_polys, 2.0 * des_dist, max_d, d_out);
    ASEP_HIP_CHECK(hipGetLastError());
    if (int rc = tm.stop(st)) return rc;
    ASEP_HIP_CHECK(hipMemcpyAsync(out_dist, d_out, (size_t)n_polys * sizeof(double), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));          // range is stack-owned and the distances are the caller's next input
    return tm.read(g_kernel_us[0]);
    ASEP_GUARD_END
}

long long asep_textblock_neighbour_words(int n_pages, const int32_t* page_off) {
    if (n_pages < 0 || !page_off) return ASEP_ERR_ARG;
    long long total = 0;
    for (int pg = 0; pg < n_pages; ++pg) {
        const long long n = (long long)page_off[pg + 1] - page_off[pg];
        if (n < 0) return ASEP_ERR_ARG;
        total += n * ((n + 31) / 32);
    }
    return total;
}

int asep_textblock_neighbours(asep_post* p, int n_pages, const int32_t* page_off, const int32_t* boxes,
                              const double* dists, const double* avg, double fac, uint32_t* out_bits,
                              long long capacity_words) {
    if (!p || n_pages < 0 || !page_off) {
        set_error("asep_textblock_neighbours: bad arguments");
        return ASEP_ERR_ARG;
    }
    const int n_polys = page_off[n_pages];
    if (n_polys < 0 || !check_offsets("asep_textblock_neighbours", page_off, n_pages, n_polys, false)) return ASEP_ERR_ARG;
    const long long words = asep_textblock_neighbour_words(n_pages, page_off);
    if (words > capacity_words) {
        set_error("asep_textblock_neighbours: %lld words needed, capacity %lld", words, capacity_words);
        return ASEP_ERR_ARG;
    }
    if (n_polys == 0) return ASEP_OK;
    if (!boxes || !dists || !avg || !out_bits) {
        set_error("asep_textblock_neighbours: null argument");
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    std::vector<int32_t> rows(2 * (size_t)n_polys);
    std::vector<long long> bits_off(n_pages);
    long long acc = 0;
    for (int pg = 0; pg < n_pages; ++pg) {
        const long long n = page_off[pg + 1] - page_off[pg];
        bits_off[pg] = acc;
        acc += n * ((n + 31) / 32);
        for (int i = page_off[pg]; i < page_off[pg + 1]; ++i) {
            rows[2 * (size_t)i] = i;
            rows[2 * (size_t)i + 1] = pg;
        }
    }
    pool.begin();
    int4* d_box = (int4*)pool.get((size_t)n_polys * sizeof(int4));
    double* d_dist = (double*)pool.get((size_t)n_polys * sizeof(double));
    double* d_avg = (double*)pool.get((size_t)n_pages * sizeof(double));
    int* d_poff = (int*)pool.get((size_t)(n_pages + 1) * sizeof(int));
    int2* d_rows = (int2*)pool.get((size_t)n_polys * sizeof(int2));
    long long* d_boff = (long long*)pool.get((size_t)n_pages * sizeof(long long));
    uint32_t* d_bits = (uint32_t*)pool.get((size_t)words * sizeof(uint32_t));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_box, boxes, (size_t)n_polys * sizeof(int4), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_dist, dists, (size_t)n_polys * sizeof(double), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_avg, avg, (size_t)n_pages * sizeof(double), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_poff, page_off, (size_t)(n_pages + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_rows, rows.data(), (size_t)n_polys * sizeof(int2), hipMemcpyHostToDevice, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(d_boff, bits_off.data(), (size_t)n_pages * sizeof(long long), hipMemcpyHostToDevice, st));
    KernelTimer tm;
    if (int rc = tm.start(st)) return rc;
    tb_neighbour_kernel<<<(unsigned)n_polys, 64, 0, st>>>(d_box, d_dist, d_avg, d_poff, d_rows, d_boff, fac, d_bits);
    ASEP_HIP_CHECK(hipGetLastError());
    if (int rc = tm.stop(st)) return rc;
    ASEP_HIP_CHECK(hipMemcpyAsync(out_bits, d_bits, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    return tm.read(g_kernel_us[1]);
    ASEP_GUARD_END
}
