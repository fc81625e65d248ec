// Host side of the alpha-shape text regions (include/asep_hip.h, "text regions" block): one call for all articles of a
// group of pages, on the asep_post handle (its stream and buffer pool).  Compiled with -ffp-contract=off, like the
// kernels it launches.
#include <climits>

#include "asep_common.h"
#include "batch_tables.h"
#include "alpha_shape_kernels.h"

using namespace asep;

namespace {

// device time of the last kernel of each kind launched by this thread (0 circumradii, 1 boundaries), microseconds
thread_local double g_kernel_us[2] = {0.0, 0.0};

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
