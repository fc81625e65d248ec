// Host side of the alpha-shape text regions (include/asep_hip.h, "text regions" block): one call for all articles of a
// group of pages, on the asep_post handle (its stream and buffer pool).  Compiled with -ffp-contract=off, like the
// kernels it launches.
#include <climits>

#include "asep_common.h"
#include "batch_tables.h"
#include "alpha_shape_kernels.h"
#include "delaunay_kernels.h"

using namespace asep;

namespace {

// device time of the last kernel of each kind launched by this thread (0 circumradii, 1 boundaries), microseconds
thread_local double g_kernel_us[2] = {0.0, 0.0};
// device time of the last triangulation kernel launched by this thread, microseconds
thread_local double g_delaunay_us = 0.0;

}  // namespace

double asep_alpha_shapes_last_kernel_us(int which) { return (which == 0 || which == 1) ? g_kernel_us[which] : -1.0; }

int asep_alpha_shapes_lds_points(void) { return AS_LDS_POINTS; }

int asep_alpha_shapes(asep_post* p, int n_pages, const int32_t* art_off, const int32_t* pt_off, const int32_t* tri_off,
                      const int32_t* points, const int32_t* simplices, const int32_t* neighbors, const double* alpha0,
                      int max_retries, int32_t* out_ring, int32_t* out_len, int32_t* out_retries, int32_t* out_failed,
                      double* out_circum_r, uint8_t* out_edge_mask) {
    const char* const fn = "asep_alpha_shapes";
    if (!p || n_pages < 0 || !art_off || max_retries < 1) {
        set_error("%s: bad arguments", fn);
        return ASEP_ERR_ARG;
    }
    if (!check_offsets(fn, "art_off", art_off, n_pages)) return ASEP_ERR_ARG;
    const int n_art = art_off[n_pages];
    if (n_art == 0) return ASEP_OK;
    if (!pt_off || !tri_off || !alpha0 || !out_len || !out_retries || !out_failed) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    if (!check_offsets(fn, "pt_off", pt_off, n_art) || !check_offsets(fn, "tri_off", tri_off, n_art)) return ASEP_ERR_ARG;
    const int n_pts = pt_off[n_art], n_tri = tri_off[n_art];
    if (n_tri > INT_MAX / 3) {                       // a half-edge is numbered 3 * t + k in an int
        set_error("%s: %d triangles in one call, at most %d", fn, n_tri, INT_MAX / 3);
        return ASEP_ERR_ARG;
    }
    if ((n_pts > 0 && (!points || !out_ring)) || (n_tri > 0 && (!simplices || !neighbors))) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    if (!check_triangles(fn, n_pages, art_off, pt_off, tri_off, simplices, neighbors)) return ASEP_ERR_ARG;
    bool over_lds = false;
    for (int a = 0; a < n_art; ++a) over_lds |= pt_off[a + 1] - pt_off[a] > AS_LDS_POINTS;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    int2* d_pts = upload(pool, st, (const int2*)points, (size_t)n_pts);
    int* d_simp = upload(pool, st, simplices, 3 * (size_t)n_tri);
    int* d_neigh = upload(pool, st, neighbors, 3 * (size_t)n_tri);
    int* d_poff = upload(pool, st, pt_off, (size_t)n_art + 1);
    int* d_toff = upload(pool, st, tri_off, (size_t)n_art + 1);
    double* d_alpha = upload(pool, st, alpha0, (size_t)n_art);
    double* d_circ = (double*)pool.get(((size_t)n_tri + 1) * sizeof(double));
    int* d_ring = (int*)pool.get(((size_t)n_pts + 1) * sizeof(int));
    int* d_res = (int*)pool.get(3 * (size_t)n_art * sizeof(int));          // len | retries | failed
    uint8_t* d_mask = out_edge_mask ? (uint8_t*)pool.get((size_t)n_tri + 1) : nullptr;
    int* d_scratch = over_lds ? (int*)pool.get(2 * (size_t)n_pts * sizeof(int)) : nullptr;
    KernelTimer tc, tb;
    tc.start(st);
    if (n_tri > 0) {
        as_circum_kernel<<<(unsigned)cdiv(n_tri, AS_THREADS), AS_THREADS, 0, st>>>(d_pts, d_simp, d_poff, d_toff, n_art, n_tri, d_circ);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    tc.stop(st);
    tb.start(st);
    as_boundary_kernel<<<(unsigned)n_art, AS_THREADS, 0, st>>>(d_simp, d_neigh, d_poff, d_toff, d_circ, d_alpha, max_retries, d_scratch,
                                                              d_ring, d_res, d_res + n_art, d_res + 2 * (size_t)n_art, d_mask);
    ASEP_HIP_CHECK(hipGetLastError());
    tb.stop(st);
    if (n_pts) ASEP_HIP_CHECK(hipMemcpyAsync(out_ring, d_ring, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_len, d_res, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_retries, d_res + n_art, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_failed, d_res + 2 * (size_t)n_art, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    if (out_circum_r && n_tri)
        ASEP_HIP_CHECK(hipMemcpyAsync(out_circum_r, d_circ, (size_t)n_tri * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out_edge_mask && n_tri) ASEP_HIP_CHECK(hipMemcpyAsync(out_edge_mask, d_mask, (size_t)n_tri, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tc.read(g_kernel_us[0]);
    tb.read(g_kernel_us[1]);
    return ASEP_OK;
    ASEP_GUARD_END
}

// ---- the triangulation on the device --------------------------------------------------------------------------------------

double asep_delaunay_last_kernel_us(void) { return g_delaunay_us; }

int asep_delaunay_lds_points(void) { return DT_LDS_POINTS; }

int asep_delaunay_max_extent(void) { return DT_MAX_EXTENT; }

namespace {

// the scratch of the articles over DT_LDS_POINTS (null when there is none)
int* delaunay_scratch(BufferPool& pool, const int32_t* pt_off, int n_art) {
    bool over_lds = false;
    for (int a = 0; a < n_art; ++a) over_lds |= pt_off[a + 1] - pt_off[a] > DT_LDS_POINTS;
    return over_lds ? (int*)pool.get((size_t)(DT_WORDS_PER_POINT + 1) * (size_t)pt_off[n_art] * sizeof(int)) : nullptr;
}

}  // namespace

int asep_delaunay(asep_post* p, int n_articles, const int32_t* pt_off, const int32_t* points, const int32_t* tri_off_cap,
                  int32_t* out_simplices, int32_t* out_neighbors, int32_t* out_ntri, int32_t* out_status) {
    const char* const fn = "asep_delaunay";
    if (!p || n_articles < 0 || !pt_off || !tri_off_cap) {
        set_error("%s: bad arguments", fn);
        return ASEP_ERR_ARG;
    }
    if (!check_delaunay_tables(fn, n_articles, pt_off, tri_off_cap)) return ASEP_ERR_ARG;
    if (n_articles == 0) return ASEP_OK;
    const int n_pts = pt_off[n_articles], cap = tri_off_cap[n_articles];
    if (!check_points_total(fn, n_pts)) return ASEP_ERR_ARG;
    if (!out_ntri || !out_status || (n_pts > 0 && !points) || (cap > 0 && (!out_simplices || !out_neighbors))) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    int2* d_pts = upload(pool, st, (const int2*)points, (size_t)n_pts);
    int* d_poff = upload(pool, st, pt_off, (size_t)n_articles + 1);
    int* d_coff = upload(pool, st, tri_off_cap, (size_t)n_articles + 1);
    int* d_simp = (int*)pool.get((3 * (size_t)cap + 1) * sizeof(int));
    int* d_neigh = (int*)pool.get((3 * (size_t)cap + 1) * sizeof(int));
    int* d_res = (int*)pool.get(2 * (size_t)n_articles * sizeof(int));       // n_tri | status
    int* d_scratch = delaunay_scratch(pool, pt_off, n_articles);
    if (cap) {                                       // the entries no triangle fills come back as zeros
        ASEP_HIP_CHECK(hipMemsetAsync(d_simp, 0, 3 * (size_t)cap * sizeof(int), st));
        ASEP_HIP_CHECK(hipMemsetAsync(d_neigh, 0, 3 * (size_t)cap * sizeof(int), st));
    }
    KernelTimer tk;
    tk.start(st);
    dt_kernel<<<(unsigned)n_articles, DT_THREADS, 0, st>>>(d_pts, d_poff, d_coff, d_scratch, d_simp, d_neigh, d_res, d_res + n_articles);
    ASEP_HIP_CHECK(hipGetLastError());
    tk.stop(st);
    if (cap) {
        ASEP_HIP_CHECK(hipMemcpyAsync(out_simplices, d_simp, 3 * (size_t)cap * sizeof(int), hipMemcpyDeviceToHost, st));
        ASEP_HIP_CHECK(hipMemcpyAsync(out_neighbors, d_neigh, 3 * (size_t)cap * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    ASEP_HIP_CHECK(hipMemcpyAsync(out_ntri, d_res, (size_t)n_articles * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_status, d_res + n_articles, (size_t)n_articles * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tk.read(g_delaunay_us);
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_alpha_shapes_points(asep_post* p, int n_pages, const int32_t* art_off, const int32_t* pt_off, const int32_t* points,
                             const double* alpha0, int max_retries, int32_t* out_ring, int32_t* out_len, int32_t* out_retries,
                             int32_t* out_failed, int32_t* out_status) {
    const char* const fn = "asep_alpha_shapes_points";
    if (!p || n_pages < 0 || !art_off || max_retries < 1) {
        set_error("%s: bad arguments", fn);
        return ASEP_ERR_ARG;
    }
    if (!check_offsets(fn, "art_off", art_off, n_pages)) return ASEP_ERR_ARG;
    const int n_art = art_off[n_pages];
    if (n_art == 0) return ASEP_OK;
    if (!pt_off || !alpha0 || !out_len || !out_retries || !out_failed || !out_status) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    if (!check_offsets(fn, "pt_off", pt_off, n_art)) return ASEP_ERR_ARG;
    const int n_pts = pt_off[n_art];
    if (!check_points_total(fn, n_pts)) return ASEP_ERR_ARG;
    if (n_pts > 0 && (!points || !out_ring)) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    bool over_lds = false;
    for (int a = 0; a < n_art; ++a) over_lds |= pt_off[a + 1] - pt_off[a] > AS_LDS_POINTS;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    pool.begin();
    // one point more than the call has: as_circum_kernel below also runs over triangle slots that no article owns (see there)
    int2* d_pts = (int2*)pool.get(((size_t)n_pts + 1) * sizeof(int2));
    ASEP_HIP_CHECK(hipMemsetAsync(d_pts + n_pts, 0, sizeof(int2), st));
    if (n_pts) ASEP_HIP_CHECK(hipMemcpyAsync(d_pts, points, (size_t)n_pts * sizeof(int2), hipMemcpyHostToDevice, st));
    int* d_poff = upload(pool, st, pt_off, (size_t)n_art + 1);
    double* d_alpha = upload(pool, st, alpha0, (size_t)n_art);
    // the roomy tables (article a from 2 * pt_off[a]) and the packed ones the alpha-shape kernels read.  The call's triangle count
    // stays on the device: everything below is sized by its bound, 2 triangles a point.
    const int tri_bound = 2 * n_pts;
    int* d_simp0 = (int*)pool.get((3 * (size_t)tri_bound + 1) * sizeof(int));
    int* d_neigh0 = (int*)pool.get((3 * (size_t)tri_bound + 1) * sizeof(int));
    int* d_simp = (int*)pool.get((3 * (size_t)tri_bound + 1) * sizeof(int));
    int* d_neigh = (int*)pool.get((3 * (size_t)tri_bound + 1) * sizeof(int));
    int* d_toff = (int*)pool.get(((size_t)n_art + 1) * sizeof(int));
    int* d_res = (int*)pool.get(5 * (size_t)n_art * sizeof(int));          // len | retries | failed | n_tri | status
    int* d_ring = (int*)pool.get(((size_t)n_pts + 1) * sizeof(int));
    double* d_circ = (double*)pool.get(((size_t)tri_bound + 1) * sizeof(double));
    int* d_scratch = delaunay_scratch(pool, pt_off, n_art);
    int* d_scratch_as = over_lds ? (int*)pool.get(2 * (size_t)n_pts * sizeof(int)) : nullptr;
    // packed slots behind the call's last triangle read as the triangle (0, 0, 0)
    if (tri_bound) ASEP_HIP_CHECK(hipMemsetAsync(d_simp, 0, 3 * (size_t)tri_bound * sizeof(int), st));
    KernelTimer td, tc, tb;
    td.start(st);
    dt_kernel<<<(unsigned)n_art, DT_THREADS, 0, st>>>(d_pts, d_poff, nullptr, d_scratch, d_simp0, d_neigh0, d_res + 3 * (size_t)n_art,
                                                       d_res + 4 * (size_t)n_art);
    ASEP_HIP_CHECK(hipGetLastError());
    td.stop(st);
    dt_offsets_kernel<<<1, DT_THREADS, 0, st>>>(d_res + 3 * (size_t)n_art, n_art, d_toff);
    ASEP_HIP_CHECK(hipGetLastError());
    dt_pack_kernel<<<(unsigned)n_art, DT_THREADS, 0, st>>>(d_poff, d_toff, d_simp0, d_neigh0, d_simp, d_neigh);
    ASEP_HIP_CHECK(hipGetLastError());
    // as_circum_kernel over the bound, not over the count, which the host does not know: a slot g behind tri_off[n_art] finds the last
    // article, reads the zeroed corners (0, 0, 0) and that article's first point (the padding point when it has none) and writes a
    // circ[g] that as_boundary_kernel, which goes by tri_off, never reads.
    const int n_tri = tri_bound;
    tc.start(st);
    if (n_tri > 0) {
        as_circum_kernel<<<(unsigned)cdiv(n_tri, AS_THREADS), AS_THREADS, 0, st>>>(d_pts, d_simp, d_poff, d_toff, n_art, n_tri, d_circ);
        ASEP_HIP_CHECK(hipGetLastError());
    }
    tc.stop(st);
    tb.start(st);
    as_boundary_kernel<<<(unsigned)n_art, AS_THREADS, 0, st>>>(d_simp, d_neigh, d_poff, d_toff, d_circ, d_alpha, max_retries, d_scratch_as,
                                                              d_ring, d_res, d_res + n_art, d_res + 2 * (size_t)n_art, nullptr);
    ASEP_HIP_CHECK(hipGetLastError());
    tb.stop(st);
    if (n_pts) ASEP_HIP_CHECK(hipMemcpyAsync(out_ring, d_ring, (size_t)n_pts * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_len, d_res, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_retries, d_res + n_art, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_failed, d_res + 2 * (size_t)n_art, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipMemcpyAsync(out_status, d_res + 4 * (size_t)n_art, (size_t)n_art * sizeof(int), hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    td.read(g_delaunay_us);
    tc.read(g_kernel_us[0]);
    tb.read(g_kernel_us[1]);
    return ASEP_OK;
    ASEP_GUARD_END
}
