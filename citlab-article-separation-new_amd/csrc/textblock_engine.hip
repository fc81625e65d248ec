// Host side of the text block detection stage (include/asep_hip.h, "text block detection" block): batched entry points
// on the asep_post handle (its stream and buffer pool).  Compiled with -ffp-contract=off, like the kernels it launches.
#include <vector>

#include "asep_common.h"
#include "batch_tables.h"
#include "textblock_kernels.h"

using namespace asep;

namespace {

// device time of the last kernel of each kind launched by this thread (0 interline distances, 1 neighbours), microseconds
thread_local double g_kernel_us[2] = {0.0, 0.0};

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
    if (n_polys < 0 || !check_offsets("asep_textblock_interline_dists", "page_off", page_off, n_pages)) return ASEP_ERR_ARG;
    if (n_polys == 0) return ASEP_OK;
    if (!points || !boxes || !orient || !out_dist) {
        set_error("asep_textblock_interline_dists: null argument");
        return ASEP_ERR_ARG;
    }
    // every polygon holds at least one point (the reference indexes x_points[0] / x_points[-1])
    if (!check_offsets("asep_textblock_interline_dists", "poly_off", poly_off, n_polys, true)) return ASEP_ERR_ARG;
    const int n_points = poly_off[n_polys];
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
    int2* d_pts = upload(pool, st, (const int2*)points, (size_t)n_points);
    int* d_off = upload(pool, st, poly_off, (size_t)n_polys + 1);
    int4* d_box = upload(pool, st, (const int4*)boxes, (size_t)n_polys);
    double2* d_or = upload(pool, st, (const double2*)orient, (size_t)n_polys);
    int2* d_rng = upload(pool, st, (const int2*)range.data(), (size_t)n_polys);
    double* d_out = (double*)pool.get((size_t)n_polys * sizeof(double));
    const unsigned blocks = (unsigned)(((size_t)n_polys + 3) / 4);      // four waves (polygons) per 256-thread block
    KernelTimer tm;
    tm.start(st);
    tb_interline_kernel<<<blocks, 256, 0, st>>>(d_pts, d_off, d_box, d_or, d_rng, n_polys, 2.0 * des_dist, max_d, d_out);
    ASEP_HIP_CHECK(hipGetLastError());
    tm.stop(st);
    ASEP_HIP_CHECK(hipMemcpyAsync(out_dist, d_out, (size_t)n_polys * sizeof(double), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));          // range is stack-owned and the distances are the caller's next input
    tm.read(g_kernel_us[0]);
    return ASEP_OK;
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
    if (n_polys < 0 || !check_offsets("asep_textblock_neighbours", "page_off", page_off, n_pages)) return ASEP_ERR_ARG;
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
    int4* d_box = upload(pool, st, (const int4*)boxes, (size_t)n_polys);
    double* d_dist = upload(pool, st, dists, (size_t)n_polys);
    double* d_avg = upload(pool, st, avg, (size_t)n_pages);
    int* d_poff = upload(pool, st, page_off, (size_t)n_pages + 1);
    int2* d_rows = upload(pool, st, (const int2*)rows.data(), (size_t)n_polys);
    long long* d_boff = upload(pool, st, bits_off.data(), (size_t)n_pages);
    uint32_t* d_bits = (uint32_t*)pool.get((size_t)words * sizeof(uint32_t));
    KernelTimer tm;
    tm.start(st);
    tb_neighbour_kernel<<<(unsigned)n_polys, 64, 0, st>>>(d_box, d_dist, d_avg, d_poff, d_rows, d_boff, fac, d_bits);
    ASEP_HIP_CHECK(hipGetLastError());
    tm.stop(st);
    ASEP_HIP_CHECK(hipMemcpyAsync(out_bits, d_bits, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tm.read(g_kernel_us[1]);
    return ASEP_OK;
    ASEP_GUARD_END
}
