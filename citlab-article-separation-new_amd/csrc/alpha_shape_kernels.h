// Device kernels of the alpha-shape text regions (include/asep_hip.h, "text regions" block): the part of
// python_util/geometry/util.py:568-697 alpha_shape behind the Delaunay triangulation, for all articles of a call.
// Compiled with -ffp-contract=off (alpha_shape_engine.o in the Makefile): every double below restates one numpy float64
// operation and must not be fused into an FMA.
//
// Why the parallel form gives the reference's result.  The reference (util.py:650-670) keeps a list of
// directed edges and walks the accepted triangles (circum_r < alpha) in index order; for each it offers
// (a,b), (b,c), (c,a), and an edge whose undirected form is already in the list is removed instead of added.  An edge
// of a 2-D Delaunay triangulation lies in at most two triangles, so an edge is offered at most twice:
//   * survivors: the half-edges (t, k) of accepted triangles whose neighbour across that edge is missing (-1) or not
//     accepted.  Edge k = 0, 1, 2 is (a,b), (b,c), (c,a); scipy's Delaunay.neighbors[t][j] is the triangle opposite
//     vertex j, so the neighbour across edge k is neighbors[t][(k + 2) % 3] (opposite c, a, b);
//   * order and direction: an edge offered twice is never offered again, so the list is the survivors in (t, k)
//     ascending order, each in the direction triangle t lists it;
//   * degrees: the survivors are the boundary of a union of triangles, every vertex of it has even degree;
//   * acceptance: get_ordered_circles (util.py:589-615) starts at the first survivor e0 = (u, v) and appends, pass
//     after pass, the unvisited edge that touches the end of the circle; util.py:676-687 retries with
//     alpha + alpha * 0.2 when there is no edge, more than one circle, or a vertex met more than twice.  With every
//     degree exactly 2 the circle from e0 is forced: from v it takes the incident edge it did not come by, and it
//     closes at u.  It holds all edges (one circle) iff it closes after exactly as many steps as there are survivors.
//     A vertex of degree 4 or more either splits the circles or is met more than twice: a retry both ways.  So alpha
//     is accepted iff there is a survivor, every boundary vertex has degree 2, and the walk from e0 returns to u after
//     E steps; the result is the walk's vertices (e[0] of each edge of the circle) with the first appended;
//   * slivers: a negative Heron product gives area = NaN, circum_r = NaN, and NaN < alpha is false for every alpha.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace asep {

// Points whose two vertex tables (degree, xor of the boundary neighbours: 8 bytes a point) a workgroup keeps in LDS:
// 7680 points = 60 KiB of the 64 KiB one workgroup can declare statically; the CU's 160 KiB LDS (MI355X) then holds two
// such workgroups side by side.  Larger articles use a slice of the call's global scratch.
constexpr int AS_LDS_POINTS = 7680;
constexpr int AS_THREADS = 256;

// np.linalg.norm of an integer difference: the squares and their sum are exact, sqrt is the correctly rounded one
// (the compiler expands llvm.sqrt.f64 to v_rsq_f64 plus the fma refinement and the final correction step).
__device__ inline double as_side(int2 p, int2 q) {
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y;
    return sqrt(dx * dx + dy * dy);
}

// util.py:637-648, one triangle per thread over the whole call.  tri_off [n_art + 1], pt_off [n_art + 1];
// simplices [sum T][3] local to their article; circ [sum T].
__global__ void __launch_bounds__(AS_THREADS) as_circum_kernel(const int2* __restrict__ pts, const int* __restrict__ simplices,
                                                               const int* __restrict__ pt_off, const int* __restrict__ tri_off,
                                                               int n_art, int n_tri, double* __restrict__ circ) {
    const int g = (int)(blockIdx.x * (unsigned)AS_THREADS + threadIdx.x);
    if (g >= n_tri) return;
    int lo = 0, hi = n_art - 1;                      // the article with tri_off[lo] <= g < tri_off[lo + 1]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tri_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int2* P = pts + pt_off[lo];
    const int* s = simplices + 3 * (size_t)g;
    const int2 pa = P[s[0]], pb = P[s[1]], pc = P[s[2]];
    const double a = as_side(pa, pb), b = as_side(pb, pc), c = as_side(pc, pa);
    const double sh = (a + b + c) / 2.0;
    const double area = sqrt(sh * (sh - a) * (sh - b) * (sh - c));
    circ[g] = a * b * c / (4.0 * (area + 1e-8));
}

// The retry rounds of one article; deg / nbx [N] are the vertex tables (LDS or global scratch).
__device__ __forceinline__ void as_rounds(int* deg, int* nbx, int N, int T, const int* __restrict__ simp, const int* __restrict__ neigh,
                                 const double* __restrict__ circ, double alpha, int max_retries, int* __restrict__ ring,
                                 uint8_t* __restrict__ mask, int* out_len, int* out_retries, int* out_failed) {
    __shared__ int s_first, s_edges, s_bad, s_ok, s_len;
    const int tid = threadIdx.x;
    int retries = 0, failed = 0;
    for (;;) {
        for (int i = tid; i < N; i += AS_THREADS) {
            deg[i] = 0;
            nbx[i] = 0;
        }
        if (tid == 0) {
            s_first = INT32_MAX;
            s_edges = 0;
            s_bad = 0;
        }
        __syncthreads();
        // 1-3: boundary half-edges, vertex degrees and neighbours, the first half-edge
        int first = INT32_MAX, cnt = 0;
        for (int t = tid; t < T; t += AS_THREADS) {
            int m = 0;
            if (circ[t] < alpha) {
                const int v3[3] = {simp[3 * (size_t)t], simp[3 * (size_t)t + 1], simp[3 * (size_t)t + 2]};
                for (int k = 0; k < 3; ++k) {
                    const int nb = neigh[3 * (size_t)t + (k + 2) % 3];
                    if (nb >= 0 && circ[nb] < alpha) continue;
                    const int u = v3[k], v = v3[(k + 1) % 3];
                    atomicAdd(&deg[u], 1);
                    atomicXor(&nbx[u], v);
                    atomicAdd(&deg[v], 1);
                    atomicXor(&nbx[v], u);
                    m |= 1 << k;
                    if (first == INT32_MAX) first = 3 * t + k;
                    ++cnt;
                }
            }
            if (mask) mask[t] = (uint8_t)m;
        }
        if (cnt) {
            atomicMin(&s_first, first);
            atomicAdd(&s_edges, cnt);
        }
        __syncthreads();
        // 4: degree 2 at every boundary vertex
        int bad = 0;
        for (int i = tid; i < N; i += AS_THREADS) {
            const int d = deg[i];
            bad |= (d != 0 && d != 2);
        }
        if (bad) atomicOr(&s_bad, 1);
        __syncthreads();
        // 5: one lane walks the cycle from e0 = (u, v): at each vertex the xor of its two neighbours and the vertex it came
        // from give the other one.  With every degree 2 there are as many edges as boundary vertices, so E <= N entries.
        if (tid == 0) {
            int ok = 0;
            const int E = s_edges;
            if (E > 0 && !s_bad && E <= N) {
                const int t = s_first / 3, k = s_first % 3;
                const int u = simp[3 * (size_t)t + k];
                int prev = u, cur = simp[3 * (size_t)t + (k + 1) % 3], len = 1;
                ring[0] = u;
                while (cur != u && len < E && (unsigned)cur < (unsigned)N) {
                    ring[len++] = cur;
                    const int nxt = nbx[cur] ^ prev;
                    prev = cur;
                    cur = nxt;
                }
                ok = (cur == u && len == E);
                s_len = len;
            }
            s_ok = ok;
        }
        __syncthreads();
        if (s_ok) break;
        ++retries;
        if (retries >= max_retries) {
            failed = 1;
            break;
        }
        alpha = alpha + alpha * 0.2;                 // util.py:678 / 687, in that form
    }
    if (tid == 0) {
        *out_len = failed ? 0 : s_len;
        *out_retries = retries;
        *out_failed = failed;
    }
}

// util.py:650-697 without the triangulation, one workgroup per article, the retries inside.
//   simplices / neighbors [sum T][3] local to the article (-1 = no neighbour); alpha0 [n_art];
//   scratch: 2 ints per point of the call (read only by articles over AS_LDS_POINTS; may be null when there is none);
//   ring [sum N] (article a owns pt_off[a] ..), len / retries / failed [n_art]; mask [sum T] or null: bit k = half-edge
//   (t, k) is on the boundary, of the last round that ran.
__global__ void __launch_bounds__(AS_THREADS) as_boundary_kernel(const int* __restrict__ simplices, const int* __restrict__ neighbors,
                                                                 const int* __restrict__ pt_off, const int* __restrict__ tri_off,
                                                                 const double* __restrict__ circ, const double* __restrict__ alpha0,
                                                                 int max_retries, int* __restrict__ scratch, int* __restrict__ ring,
                                                                 int* __restrict__ len, int* __restrict__ retries,
                                                                 int* __restrict__ failed, uint8_t* __restrict__ mask) {
    __shared__ int s_deg[AS_LDS_POINTS], s_nbx[AS_LDS_POINTS];
    const int a = blockIdx.x;
    const int p0 = pt_off[a], N = pt_off[a + 1] - p0;
    const int t0 = tri_off[a], T = tri_off[a + 1] - t0;
    const int* simp = simplices + 3 * (size_t)t0;
    const int* neigh = neighbors + 3 * (size_t)t0;
    uint8_t* m = mask ? mask + t0 : nullptr;
    if (N <= AS_LDS_POINTS)
        as_rounds(s_deg, s_nbx, N, T, simp, neigh, circ + t0, alpha0[a], max_retries, ring + p0, m, len + a, retries + a, failed + a);
    else
        as_rounds(scratch + 2 * (size_t)p0, scratch + 2 * (size_t)p0 + N, N, T, simp, neigh, circ + t0, alpha0[a], max_retries,
                  ring + p0, m, len + a, retries + a, failed + a);
}

}  // namespace asep
