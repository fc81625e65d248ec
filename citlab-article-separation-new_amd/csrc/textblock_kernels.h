// Device kernels of the text block detection stage (include/asep_hip.h, "text block detection" block).
// Compiled with -ffp-contract=off (textblock_engine.o in the Makefile): every double below restates one Python float
// operation of dbscan_baselines.py and must not be fused into an FMA.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace asep {

// get_dist_fast (python_util/geometry/util.py:775-795): L1 distance of a point to a box {x, y, w, h}, accumulated
// from 0.0 term by term as the reference does (the terms are integers, so every partial sum is exact).
__device__ inline double tb_box_dist(int px, int py, int4 bb) {
    double d = 0.0;
    if (px < bb.x) d += (double)(bb.x - px);
    if (px > bb.x + bb.z) d += (double)(px - bb.x - bb.z);
    if (py < bb.y) d += (double)(bb.y - py);
    if (py > bb.y + bb.w) d += (double)(py - bb.y - bb.w);
    return d;
}

// get_in_dist / get_off_dist (util.py:798-828): diff_x = x1 - x2, diff_y = -y1 + y2 (integers), then two products and
// one sum / difference in double.
__device__ inline double tb_in_dist(int2 p1, int2 p2, double ox, double oy) {
    const double dx = (double)(p1.x - p2.x), dy = (double)(-p1.y + p2.y);
    return dx * ox + dy * oy;
}
__device__ inline double tb_off_dist(int2 p1, int2 p2, double ox, double oy) {
    const double dx = (double)(p1.x - p2.x), dy = (double)(-p1.y + p2.y);
    return dx * oy - dy * ox;
}

// dbscan_baselines.py:35-110 (use_java_code=False), one 64-lane wave per poly_a.  The reference scans the pairs
// (p_a, poly_b) in the order "points of poly_a outer, polygons of the page inner"; a pair is skipped when the box
// distance exceeds the RUNNING minimum `dist`, so the result depends on that order.  Each round the lanes take 64
// consecutive pairs of the scan and compute (box distance, m) with m = the pair's own minimum of |off_dist| over the
// points p_b with |in_dist| <= 2*des_dist (+inf when the end-point test skips poly_b or nothing qualifies): that inner
// minimum does not read `dist`.  The wave then applies, in scan order, the lowest lane with box <= dist && m < dist and
// re-ballots.  `dist` only decreases, so a lane that failed once cannot pass later: the sequence of updates is the
// reference's.  A lane whose box distance already exceeds the dist at the start of the round skips its inner loop.
//   pts [n_points] (x, y); poly_off [n_polys + 1]; boxes [n_polys] {x, y, w, h} with w = max - min + 1;
//   orient [n_polys] (cos, sin); range [n_polys] {first, end} polygon indices of the polygon's page.
__global__ void __launch_bounds__(256) tb_interline_kernel(const int2* __restrict__ pts, const int* __restrict__ poly_off,
                                                           const int4* __restrict__ boxes,
                                                           const double2* __restrict__ orient,
                                                           const int2* __restrict__ range, int n_polys, double des2,
                                                           double max_d, double* __restrict__ out) {
    const int a = (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (a >= n_polys) return;                          // uniform per wave
    const int a0 = poly_off[a], a1 = poly_off[a + 1];
    const int Pa = a1 - a0;
    const double ox = orient[a].x, oy = orient[a].y;
    const int b_first = range[a].x, Nb = range[a].y - range[a].x;
    const int2 pt_a1 = pts[a0], pt_a2 = pts[a1 - 1];
    double dist = max_d;
    // lane position in the flat scan t = ia * Nb + jb, advanced by 64 per round
    int ia = lane / Nb, jb = lane % Nb;
    const int step_a = 64 / Nb, step_b = 64 % Nb;
    const long long T = (long long)Pa * Nb;
    for (long long base = 0; base < T; base += 64) {
        double bd = INFINITY, m = INFINITY;
        if (ia < Pa) {
            const int b = b_first + jb;
            if (b != a) {                               // identity, not equality: duplicates still see each other
                const int2 pa = pts[a0 + ia];
                const int4 bb = boxes[b];
                bd = tb_box_dist(pa.x, pa.y, bb);
                if (bd <= dist) {
                    const int b0 = poly_off[b], b1 = poly_off[b + 1];
                    const int2 pt_b1 = pts[b0], pt_b2 = pts[b1 - 1];
                    const double i1 = tb_in_dist(pt_a1, pt_b1, ox, oy), i2 = tb_in_dist(pt_a1, pt_b2, ox, oy);
                    const double i3 = tb_in_dist(pt_a2, pt_b1, ox, oy), i4 = tb_in_dist(pt_a2, pt_b2, ox, oy);
                    const bool skip = (i1 < 0 && i2 < 0 && i3 < 0 && i4 < 0) || (i1 > 0 && i2 > 0 && i3 > 0 && i4 > 0);
                    if (!skip) {
                        for (int k = b0; k < b1; ++k) {
                            const int2 pb = pts[k];
                            if (fabs(tb_in_dist(pa, pb, ox, oy)) <= des2) {
                                const double o = fabs(tb_off_dist(pa, pb, ox, oy));
                                if (o < m) m = o;
                            }
                        }
                    }
                }
            }
        }
        for (;;) {
            const unsigned long long mask = __ballot(bd <= dist && m < dist);
            if (!mask) break;
            dist = __shfl(m, __ffsll((long long)mask) - 1);
        }
        ia += step_a;
        jb += step_b;
        if (jb >= Nb) {
            jb -= Nb;
            ++ia;
        }
    }
    if (lane == 0) out[a] = dist < max_d ? dist : max_d;
}

// DBSCANBaselines.region_query (dbscan_baselines.py:253-307) for every ordered pair of a page: one block per row
// polygon i, one thread per 32-bit word of its row of the neighbour bit matrix (bit j of the row: j is a neighbour
// of i; the diagonal stays 0).  Expanded rectangles: the interline distance clamped to [0.5*avg, 1.5*avg] (else avg),
// y - fac*d and h + 2*fac*d truncated toward zero like Python's int().  Rectangle.intersection (rectangle.py:132-170),
// (w+1)*(h+1) surfaces in 64-bit integers, ">= 0.95 * surface" in double.
__device__ inline void tb_expanded(int4 bb, double d, double avg, double fac, long long& ey, long long& eh) {
    if (!(0.5 * avg <= d && d <= 1.5 * avg)) d = avg;
    ey = (long long)((double)bb.y - fac * d);
    eh = (long long)((double)bb.w + 2.0 * fac * d);
}

__device__ inline long long tb_inter_surface(long long x, long long y, long long w, long long h, int4 r) {
    long long tx1 = x, ty1 = y, tx2 = x + w, ty2 = y + h;
    const long long rx1 = r.x, ry1 = r.y, rx2 = rx1 + r.z, ry2 = ry1 + r.w;
    if (tx1 < rx1) tx1 = rx1;
    if (ty1 < ry1) ty1 = ry1;
    if (tx2 > rx2) tx2 = rx2;
    if (ty2 > ry2) ty2 = ry2;
    tx2 -= tx1;
    ty2 -= ty1;
    return (tx2 >= 0 && ty2 >= 0) ? (tx2 + 1) * (ty2 + 1) : 0;
}

//   rows [n_rows] {global polygon index i, page}; page_off [n_pages + 1]; bits_off [n_pages] word offsets
__global__ void __launch_bounds__(64) tb_neighbour_kernel(const int4* __restrict__ boxes, const double* __restrict__ dists,
                                                          const double* __restrict__ avg, const int* __restrict__ page_off,
                                                          const int2* __restrict__ rows,
                                                          const long long* __restrict__ bits_off, double fac,
                                                          uint32_t* __restrict__ out) {
    const int2 row = rows[blockIdx.x];
    const int i = row.x, pg = row.y;
    const int first = page_off[pg], n = page_off[pg + 1] - first;
    const int words = (n + 31) >> 5;
    const double av = avg[pg];
    const int4 b1 = boxes[i];
    long long ey1, eh1;
    tb_expanded(b1, dists[i], av, fac, ey1, eh1);
    const long long s1 = ((long long)b1.w + 1) * ((long long)b1.z + 1);
    uint32_t* orow = out + bits_off[pg] + (long long)(i - first) * words;
    for (int w = threadIdx.x; w < words; w += blockDim.x) {
        uint32_t bits = 0;
        const int j_end = min(n, (w + 1) * 32);
        for (int jj = w * 32; jj < j_end; ++jj) {
            const int j = first + jj;
            if (j == i) continue;
            const int4 b2 = boxes[j];
            long long ey2, eh2;
            tb_expanded(b2, dists[j], av, fac, ey2, eh2);
            const long long s12 = tb_inter_surface(b1.x, ey1, b1.z, eh1, b2);
            const long long s21 = tb_inter_surface(b2.x, ey2, b2.z, eh2, b1);
            const long long s2 = ((long long)b2.w + 1) * ((long long)b2.z + 1);
            if ((double)s12 >= 0.95 * (double)s2 || (double)s21 >= 0.95 * (double)s1) bits |= 1u << (jj & 31);
        }
        orow[w] = bits;
    }
}

}  // namespace asep
