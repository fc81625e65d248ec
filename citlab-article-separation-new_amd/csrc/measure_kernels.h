// Device kernels of the article separation measure (include/asep_hip.h, "article separation measure" block).
// Compiled with -ffp-contract=off (measure_engine.o in the Makefile): the doubles below restate the float operations of
// eval_measure.py:152-175 and must not be fused into an FMA.
//
// Distances are exact int32 (L1 between integer points).  Every relative-hits value is evaluated from a histogram over
// the integer distance 0..dmax (dmax = floor(3 * largest tolerance of the call); larger distances share the overflow
// bin dmax + 1, which never contributes), summed over ascending distance: the result depends on the multiset of
// distances, the point count and the tolerance only, so duplicated baselines give bit-equal values.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace asep {

constexpr int MEASURE_BLOCK = 256;
constexpr int MEASURE_MAX_DMAX = 4094;      // histogram bins 0..dmax+1 <= 4096 ints of LDS
constexpr int MEASURE_MAX_POINTS = 4096;    // points of one truth polygon (two int32 per point of LDS in the recall kernel)

// Boxes are {x, y, w, h} with w = max - min + 1 (polygon.py:91).  The gap between the boxes along one axis is a lower
// bound of the L1 distance of any two of their points, so a pair with a gap above dmax has no distance <= dmax.  The
// reference's early stop (eval_measure.py:147, rectangle.py:132-169: intersection width = 1 - gap for disjoint boxes)
// fires for gap > 3 * tol + 1 only and is implied by this test for every tolerance of the call.
__device__ inline bool ms_candidate(int4 a, int4 b, int dmax) {
    const int gx = max(a.x, b.x) - min(a.x + a.z - 1, b.x + b.z - 1);
    const int gy = max(a.y, b.y) - min(a.y + a.w - 1, b.y + b.w - 1);
    return gx <= dmax && gy <= dmax;
}

// min_q |px - qx| + |py - qy| over the points [q0, q1) (eval_measure.py:158-162), exact in int32
__device__ inline int ms_min_l1(int2 p, const int2* __restrict__ pts, int q0, int q1, int m) {
    for (int q = q0; q < q1; ++q) {
        const int2 r = pts[q];                          // wave-uniform address
        m = min(m, abs(p.x - r.x) + abs(p.y - r.y));
    }
    return m;
}

// sum_p h(d_p) / n over a histogram of the d_p: h = 1 for d <= tol, (3 tol - d) / (2 tol) for tol < d <= 3 tol, else 0
// (eval_measure.py:165-175).  A tolerance that is not positive marks "this polygon is not in that subset": 0.
__device__ inline double ms_rel_hits(const int* hist, int dmax, double tol, int n) {
    if (!(tol > 0.0)) return 0.0;
    double s = 0.0;
    for (int d = 0; d <= dmax; ++d) {
        const int c = hist[d];
        if (c == 0) continue;
        const double dd = (double)d;
        if (dd <= tol) s += (double)c;
        else if (dd <= 3.0 * tol) s += (double)c * ((3.0 * tol - dd) / (2.0 * tol));
        else break;
    }
    return s / (double)n;
}

// One thread per polygon: reco polygon i counts the truth polygons of its file that are candidates, truth polygon j
// counts the reco articles of its file that hold at least one candidate.
//   r_range [n_reco] {first, end} truth polygons of the file; t_arts [n_truth] {first, end} articles of the file;
//   art_off [n_arts + 1] reco polygon index where each article starts (the reco polygons of a file are grouped by article).
__global__ void __launch_bounds__(MEASURE_BLOCK) ms_count_kernel(const int4* __restrict__ t_box, const int4* __restrict__ r_box,
                                                                 const int2* __restrict__ r_range, const int2* __restrict__ t_arts,
                                                                 const int* __restrict__ art_off, int n_truth, int n_reco,
                                                                 int dmax, int* __restrict__ r_count, int* __restrict__ t_count) {
    const int g = (int)(blockIdx.x * (unsigned)blockDim.x + threadIdx.x);
    if (g < n_reco) {
        const int4 bb = r_box[g];
        int c = 0;
        for (int j = r_range[g].x; j < r_range[g].y; ++j) c += ms_candidate(bb, t_box[j], dmax) ? 1 : 0;
        r_count[g] = c;
    } else if (g < n_reco + n_truth) {
        const int j = g - n_reco;
        const int4 bb = t_box[j];
        int c = 0;
        for (int a = t_arts[j].x; a < t_arts[j].y; ++a) {
            bool any = false;
            for (int i = art_off[a]; i < art_off[a + 1] && !any; ++i) any = ms_candidate(bb, r_box[i], dmax);
            c += any ? 1 : 0;
        }
        t_count[j] = c;
    }
}

__device__ inline void ms_zero(int* hist, int bins) {
    for (int k = threadIdx.x; k < bins; k += MEASURE_BLOCK) hist[k] = 0;
}

// hist -> n_tols relative hits (one lane per tolerance) and, for the tests, the histogram itself
__device__ inline void ms_emit(const int* hist, int dmax, const double* __restrict__ tol, int n_tols, int n, double* out,
                               uint32_t* hist_out) {
    for (int c = threadIdx.x; c < n_tols; c += MEASURE_BLOCK) out[c] = ms_rel_hits(hist, dmax, tol[c], n);
    if (hist_out)
        for (int k = threadIdx.x; k < dmax + 2; k += MEASURE_BLOCK) hist_out[k] = (uint32_t)hist[k];
}

// count_rel_hits (eval_measure.py:125-177) for every candidate (reco i, truth j): one workgroup per reco polygon, its
// points over the lanes (the first MEASURE_BLOCK of them stay in registers), candidate truth polygons streamed through
// wave-uniform loads, the distance histogram in LDS.  Pair slot = pair_off[i] + rank of j among i's candidates.
//   tols [n_truth][n_tols]; pair_ij [n_pairs] {i, j}; pair_hits [n_pairs][n_tols]; pair_hist [n_pairs][dmax + 2] or null.
__global__ void __launch_bounds__(MEASURE_BLOCK) ms_pair_kernel(const int2* __restrict__ t_pts, const int* __restrict__ t_off,
                                                                const int4* __restrict__ t_box, const int2* __restrict__ r_pts,
                                                                const int* __restrict__ r_off, const int4* __restrict__ r_box,
                                                                const int2* __restrict__ r_range, const double* __restrict__ tols,
                                                                int n_tols, int dmax, const long long* __restrict__ pair_off,
                                                                int2* __restrict__ pair_ij, double* __restrict__ pair_hits,
                                                                uint32_t* __restrict__ pair_hist) {
    extern __shared__ int ms_lds[];
    int* hist = ms_lds;
    const int i = (int)blockIdx.x;
    const int p0 = r_off[i], n = r_off[i + 1] - p0;
    const int4 bb = r_box[i];
    const int2 first = (int)threadIdx.x < n ? r_pts[p0 + threadIdx.x] : make_int2(0, 0);
    long long slot = pair_off[i];
    for (int j = r_range[i].x; j < r_range[i].y; ++j) {
        if (!ms_candidate(bb, t_box[j], dmax)) continue;            // uniform over the workgroup
        ms_zero(hist, dmax + 2);
        __syncthreads();
        const int q0 = t_off[j], q1 = t_off[j + 1];
        for (int p = threadIdx.x; p < n; p += MEASURE_BLOCK) {
            const int2 pt = p < MEASURE_BLOCK ? first : r_pts[p0 + p];
            atomicAdd(&hist[min(ms_min_l1(pt, t_pts, q0, q1, INT_MAX), dmax + 1)], 1);
        }
        __syncthreads();
        ms_emit(hist, dmax, tols + (size_t)j * n_tols, n_tols, n, pair_hits + (size_t)slot * n_tols,
                pair_hist ? pair_hist + (size_t)slot * (dmax + 2) : nullptr);
        if (threadIdx.x == 0) pair_ij[slot] = make_int2(i, j);
        ++slot;
        __syncthreads();
    }
}

// count_rel_hits_list (eval_measure.py:194-258) of truth polygon j against every reco article of its file that holds a
// candidate, and against the union of all articles / of the articles with an id: one workgroup per truth polygon.  The
// per-point minimum over an article is taken once; the two unions are running minima over the articles (kept per point
// in LDS, clamped to dmax + 1), so one pass serves the all-baselines, the with-id and the article-pair jobs.
//   rec_ja [n_recs] {j, article index within the file}; rec_hits [n_recs][n_tols]; truth_hits [n_truth][2][n_tols]
//   (0: all articles, 1: articles with art_has_id); rec_hist / truth_hist as pair_hist, or null.
__global__ void __launch_bounds__(MEASURE_BLOCK) ms_recall_kernel(const int2* __restrict__ t_pts, const int* __restrict__ t_off,
                                                                  const int4* __restrict__ t_box, const int2* __restrict__ r_pts,
                                                                  const int* __restrict__ r_off, const int4* __restrict__ r_box,
                                                                  const int2* __restrict__ t_arts, const int* __restrict__ art_off,
                                                                  const int* __restrict__ art_has_id,
                                                                  const double* __restrict__ tols, int n_tols, int dmax, int max_points,
                                                                  const long long* __restrict__ rec_off, int2* __restrict__ rec_ja,
                                                                  double* __restrict__ rec_hits, double* __restrict__ truth_hits,
                                                                  uint32_t* __restrict__ rec_hist, uint32_t* __restrict__ truth_hist) {
    extern __shared__ int ms_lds[];
    int* hist = ms_lds;
    int* m_all = ms_lds + (dmax + 2);
    int* m_id = m_all + max_points;
    const int j = (int)blockIdx.x;
    const int p0 = t_off[j], n = t_off[j + 1] - p0;
    const int4 bb = t_box[j];
    const double* tol = tols + (size_t)j * n_tols;
    const int2 first = (int)threadIdx.x < n ? t_pts[p0 + threadIdx.x] : make_int2(0, 0);
    for (int p = threadIdx.x; p < n; p += MEASURE_BLOCK) m_all[p] = m_id[p] = dmax + 1;
    long long slot = rec_off[j];
    const int a0 = t_arts[j].x;
    for (int a = a0; a < t_arts[j].y; ++a) {
        const int i0 = art_off[a], i1 = art_off[a + 1];
        bool any = false;
        for (int i = i0; i < i1 && !any; ++i) any = ms_candidate(bb, r_box[i], dmax);
        if (!any) continue;                                          // uniform over the workgroup
        const bool with_id = art_has_id[a] != 0;
        ms_zero(hist, dmax + 2);
        __syncthreads();
        for (int p = threadIdx.x; p < n; p += MEASURE_BLOCK) {
            const int2 pt = p < MEASURE_BLOCK ? first : t_pts[p0 + p];
            int m = INT_MAX;
            for (int i = i0; i < i1; ++i)
                if (ms_candidate(bb, r_box[i], dmax)) m = ms_min_l1(pt, r_pts, r_off[i], r_off[i + 1], m);
            m = min(m, dmax + 1);
            atomicAdd(&hist[m], 1);
            m_all[p] = min(m_all[p], m);
            if (with_id) m_id[p] = min(m_id[p], m);
        }
        __syncthreads();
        ms_emit(hist, dmax, tol, n_tols, n, rec_hits + (size_t)slot * n_tols,
                rec_hist ? rec_hist + (size_t)slot * (dmax + 2) : nullptr);
        if (threadIdx.x == 0) rec_ja[slot] = make_int2(j, a - a0);
        ++slot;
        __syncthreads();
    }
    for (int u = 0; u < 2; ++u) {
        const int* m = u ? m_id : m_all;
        ms_zero(hist, dmax + 2);
        __syncthreads();
        for (int p = threadIdx.x; p < n; p += MEASURE_BLOCK) atomicAdd(&hist[m[p]], 1);
        __syncthreads();
        ms_emit(hist, dmax, tol, n_tols, n, truth_hits + ((size_t)j * 2 + u) * n_tols,
                truth_hist ? truth_hist + ((size_t)j * 2 + u) * (dmax + 2) : nullptr);
        __syncthreads();
    }
}

}  // namespace asep
