// Delaunay triangulation of the integer points of every article of a call, one workgroup per article (include/asep_hip.h, "text
// regions" block): the tables scipy.spatial.Delaunay gives the alpha shapes (alpha_shape_kernels.h), built on the device.
//
// Algorithm: incremental Bowyer-Watson with ghost triangles, exact integer predicates (delaunay_tables.h has the bound).
//   * Order.  Exact duplicates are dropped (the first of equal points stays, as in scipy, where the later ones are in no simplex).
//     The distinct points are sorted by (x, y); the first point off the line through the first two moves to the third place.  The
//     order depends on the article's points alone.  Every inserted point then lies strictly outside the closed hull of the points
//     before it: the ones on the first line lie beyond its last point, every later one is lexicographically largest.
//   * Ghosts.  A hull edge u -> v (interior on its left) carries the ghost triangle (v, u, G).  With them the triangulation is a
//     closed surface of 2n - 2 triangles and every edge has two sides.  A real triangle is in conflict with a point p when p is
//     strictly inside its circumcircle, a ghost when p is strictly on the outer side of its hull edge.  A point on the line of a hull
//     edge (beyond its end) leaves that ghost alone, so the edge's end becomes a collinear hull vertex of a proper triangle.
//   * One insertion = four passes of all lanes over the slots: the conflict test; the cavity's boundary edges and a block scan that
//     gives every new triangle its slot; the new triangles (u, v, p) on the boundary edges with their outer neighbours; the links
//     between consecutive new triangles through one table entry per boundary vertex.  The cavity of c triangles has c + 2 boundary
//     edges, so the new triangles fill the cavity's slots and two more: every slot below the count is live.  A conflict triangle's
//     first boundary edge reuses the triangle's own slot (its owner has the record in registers), further ones take the slots of
//     conflict triangles without a boundary edge, whose records nobody reads, or the two new ones: no pass reads what it overwrites.
//   * Strict in-circle tests make any valid triangulation of cocircular points; which one depends on the order above only.
//   * Slots are given by scans in lane order, not by atomics: the tables do not depend on timing or on what shares the call.
// Cost: m insertions, each with four passes over up to 2m slots and six barriers, and an O(N^2 / 256) rank sort in front: quadratic
// in the article's points (MI355X: 0.9 ms at 280 points, 4.4 ms at 896, 22 ms at 2,000, 255 ms at 7,681).  The call is as slow as its
// largest article; textblock.py keeps articles over 4,096 points on the host for that reason.
// Every loop is a counted loop over slots or points; an inconsistent table (c + 2 != boundary edges, an index out of range) ends the
// article with DT_INTERNAL.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "delaunay_tables.h"

namespace asep {

constexpr int DT_THREADS = 256;
constexpr int DT_WAVES = DT_THREADS / 64;

// the tables of one article of N points, in LDS or in the article's slice of the call's scratch (DT_WORDS_PER_POINT * N + 1 words)
struct DtTables {
    int* key;        // [N]      (x << 14 | y) of the kept points, translated to the box origin, in insertion order
    int* perm;       // [N]      insertion position -> index of the point in the article
    int* vst;        // [N + 1]  per vertex (the ghost vertex is m): the new triangle whose boundary edge starts there
    int* tv;         // [2N][3]  corners, counter-clockwise
    int* tn;         // [2N][3]  the triangle opposite corner j
    int* fre;        // [2N]     slots of conflict triangles without a boundary edge; at the end slot -> output index
    uint8_t* fa;     // [2N]     1 in conflict, 2 new
    uint8_t* fb;     // [2N]     bit j: the edge opposite corner j of a conflict triangle is on the cavity's boundary
};

__device__ inline DtTables dt_tables(int* base, int N) {
    DtTables d;
    d.key = base;
    d.perm = d.key + N;
    d.vst = d.perm + N;
    d.tv = d.vst + N + 1;
    d.tn = d.tv + 6 * (size_t)N;
    d.fre = d.tn + 6 * (size_t)N;
    d.fa = (uint8_t*)(d.fre + 2 * (size_t)N);
    d.fb = d.fa + 2 * (size_t)N;
    return d;
}

// exclusive prefix of (a, b) over the workgroup in lane order, and the totals; every lane calls it
__device__ inline int2 dt_scan2(int a, int b, int2* s_wave, int2& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int ia = a, ib = b;
    for (int d = 1; d < 64; d <<= 1) {
        const int ua = __shfl_up(ia, d, 64), ub = __shfl_up(ib, d, 64);
        if (lane >= d) {
            ia += ua;
            ib += ub;
        }
    }
    __syncthreads();                                 // the last call's readers are through
    if (lane == 63) s_wave[w] = make_int2(ia, ib);
    __syncthreads();
    int2 pre = make_int2(ia - a, ib - b);
    total = make_int2(0, 0);
    for (int k = 0; k < DT_WAVES; ++k) {
        const int2 s = s_wave[k];
        if (k < w) {
            pre.x += s.x;
            pre.y += s.y;
        }
        total.x += s.x;
        total.y += s.y;
    }
    return pre;
}

__device__ inline int dt_x(int key) { return key >> DT_EXTENT_BITS; }
__device__ inline int dt_y(int key) { return key & DT_MAX_EXTENT; }

// > 0: a, b, c counter-clockwise.  |value| < 2^29.
__device__ inline int64_t dt_orient(int a, int b, int c) {
    const int64_t abx = dt_x(b) - dt_x(a), aby = dt_y(b) - dt_y(a), acx = dt_x(c) - dt_x(a), acy = dt_y(c) - dt_y(a);
    return abx * acy - aby * acx;
}

// > 0: p strictly inside the circle through the counter-clockwise a, b, c.  |value| < 3 * 2^58.
__device__ inline int64_t dt_incircle(int a, int b, int c, int p) {
    const int px = dt_x(p), py = dt_y(p);
    const int64_t adx = dt_x(a) - px, ady = dt_y(a) - py, bdx = dt_x(b) - px, bdy = dt_y(b) - py, cdx = dt_x(c) - px, cdy = dt_y(c) - py;
    return (adx * adx + ady * ady) * (bdx * cdy - cdx * bdy) + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy) +
           (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady);
}

// One article: P its N points, d its tables; simp / neigh its slice of the output with room for `room` triangles.
// Returns (in every lane) the status; *n_tri is written by lane 0.
__device__ __forceinline__ int dt_article(const int2* __restrict__ P, int N, DtTables d, int* __restrict__ simp, int* __restrict__ neigh,
                                          int room, int* n_tri) {
    __shared__ int s_box[4], s_m, s_k, s_err;
    __shared__ int2 s_wave[DT_WAVES];
    const int tid = threadIdx.x;
    if (tid == 0) *n_tri = 0;
    if (N < 3) return DT_FEW_POINTS;
    // the bounding box
    if (tid == 0) {
        s_box[0] = s_box[1] = INT32_MAX;
        s_box[2] = s_box[3] = INT32_MIN;
        s_m = 0;
        s_k = INT32_MAX;
        s_err = 0;
    }
    __syncthreads();
    {
        int x0 = INT32_MAX, y0 = INT32_MAX, x1 = INT32_MIN, y1 = INT32_MIN;
        for (int i = tid; i < N; i += DT_THREADS) {
            const int2 p = P[i];
            x0 = min(x0, p.x), y0 = min(y0, p.y), x1 = max(x1, p.x), y1 = max(y1, p.y);
        }
        if (tid < N) {
            atomicMin(&s_box[0], x0);
            atomicMin(&s_box[1], y0);
            atomicMax(&s_box[2], x1);
            atomicMax(&s_box[3], y1);
        }
    }
    __syncthreads();
    const int bx = s_box[0], by = s_box[1];
    if ((int64_t)s_box[2] - bx > DT_MAX_EXTENT || (int64_t)s_box[3] - by > DT_MAX_EXTENT) return DT_BOX_TOO_LARGE;
    // keys; a later copy of an equal point becomes -1; the kept ones go to their rank.  raw and kept borrow the triangle tables.
    int* raw = d.tv;
    int* kept = d.tn;
    for (int i = tid; i < N; i += DT_THREADS) {
        const int2 p = P[i];
        raw[i] = ((p.x - bx) << DT_EXTENT_BITS) | (p.y - by);
    }
    __syncthreads();
    for (int i = tid; i < N; i += DT_THREADS) {
        const int k = raw[i];
        bool dup = false;
        for (int j = 0; j < i; ++j) dup |= raw[j] == k;
        kept[i] = dup ? -1 : k;
    }
    __syncthreads();
    {
        int mine = 0;
        for (int i = tid; i < N; i += DT_THREADS) {
            const int k = kept[i];
            if (k < 0) continue;
            int rank = 0;
            for (int j = 0; j < N; ++j) {
                const int kj = kept[j];
                rank += (kj >= 0) & (kj < k);
            }
            d.key[rank] = k;                          // distinct keys: every rank 0 .. m - 1 once
            d.perm[rank] = i;
            ++mine;
        }
        if (mine) atomicAdd(&s_m, mine);
    }
    __syncthreads();
    const int m = s_m, G = m;
    if (m < 3) return DT_FEW_POINTS;
    // the first point off the line through the first two
    {
        const int k0 = d.key[0], k1 = d.key[1];
        int first = INT32_MAX;
        for (int i = 2 + tid; i < m && first == INT32_MAX; i += DT_THREADS)
            if (dt_orient(k0, k1, d.key[i]) != 0) first = i;
        if (first != INT32_MAX) atomicMin(&s_k, first);
    }
    __syncthreads();
    const int kf = s_k;
    if (kf == INT32_MAX) return DT_COLLINEAR;
    if (tid == 0) {
        // ... to the third place, the collinear ones in front of it one up; then the first triangle and its three ghosts
        const int kk = d.key[kf], pk = d.perm[kf];
        for (int i = kf; i > 2; --i) {
            d.key[i] = d.key[i - 1];
            d.perm[i] = d.perm[i - 1];
        }
        d.key[2] = kk;
        d.perm[2] = pk;
        const bool ccw = dt_orient(d.key[0], d.key[1], kk) > 0;
        const int a = ccw ? 0 : 1, b = ccw ? 1 : 0, c = 2;
        const int v[12] = {a, b, c, b, a, G, c, b, G, a, c, G};
        const int n[12] = {2, 3, 1, 3, 2, 0, 1, 3, 0, 2, 1, 0};
        for (int i = 0; i < 12; ++i) {
            d.tv[i] = v[i];
            d.tn[i] = n[i];
        }
    }
    __syncthreads();
    int T = 4;                                       // 2 * (points inserted) - 2, ghosts included
    for (int ip = 3; ip < m; ++ip) {
        const int p = d.key[ip];
        // A: conflicts
        for (int t = tid; t < T; t += DT_THREADS) {
            const int v0 = d.tv[3 * t], v1 = d.tv[3 * t + 1], v2 = d.tv[3 * t + 2];
            bool bad;
            if (v0 == G) bad = dt_orient(d.key[v1], d.key[v2], p) > 0;
            else if (v1 == G) bad = dt_orient(d.key[v2], d.key[v0], p) > 0;
            else if (v2 == G) bad = dt_orient(d.key[v0], d.key[v1], p) > 0;
            else bad = dt_incircle(d.key[v0], d.key[v1], d.key[v2], p) > 0;
            d.fa[t] = bad;
        }
        __syncthreads();
        // B: boundary edges of the cavity; slots for the new triangles
        int f0 = 0, extra = 0, err = 0;
        for (int t = tid; t < T; t += DT_THREADS) {
            if (!d.fa[t]) continue;
            int mask = 0;
            for (int j = 0; j < 3; ++j) {
                const int nb = d.tn[3 * t + j];
                if ((unsigned)nb >= (unsigned)T) err = 1;
                else if (!d.fa[nb]) mask |= 1 << j;
            }
            d.fb[t] = (uint8_t)mask;
            const int b = __popc(mask);
            if (b == 0) ++f0; else extra += b - 1;
        }
        int2 total;
        const int2 pre = dt_scan2(f0, extra, s_wave, total);
        if (err || total.y != total.x + 2) s_err = 1;
        {
            int r = pre.x;
            for (int t = tid; t < T; t += DT_THREADS)
                if (d.fa[t] && d.fb[t] == 0) d.fre[r++] = t;
        }
        __syncthreads();
        if (s_err) return DT_INTERNAL;
        // C: the new triangles (u, v, p) with the neighbour across (u, v); that neighbour learns its new side
        {
            int r = pre.y;
            const int F0 = total.x;
            for (int t = tid; t < T; t += DT_THREADS) {
                if (!d.fa[t]) continue;
                const int mask = d.fb[t];
                if (!mask) continue;
                const int v[3] = {d.tv[3 * t], d.tv[3 * t + 1], d.tv[3 * t + 2]};
                const int nb[3] = {d.tn[3 * t], d.tn[3 * t + 1], d.tn[3 * t + 2]};
                bool first = true;
                for (int j = 0; j < 3; ++j) {
                    if (!(mask >> j & 1)) continue;
                    int slot = t;
                    if (!first) {
                        slot = r < F0 ? d.fre[r] : T + (r - F0);
                        ++r;
                    }
                    first = false;
                    const int u = v[(j + 1) % 3], w = v[(j + 2) % 3], out = nb[j];
                    d.tv[3 * slot] = u;
                    d.tv[3 * slot + 1] = w;
                    d.tv[3 * slot + 2] = ip;
                    d.tn[3 * slot + 2] = out;
                    d.fa[slot] = 2;
                    d.vst[u] = slot;
                    // the corner of `out` that is neither u nor w faces the shared edge
                    const int o0 = d.tv[3 * out], o1 = d.tv[3 * out + 1];
                    const int jo = (o0 != u && o0 != w) ? 0 : (o1 != u && o1 != w) ? 1 : 2;
                    d.tn[3 * out + jo] = slot;
                }
            }
        }
        __syncthreads();
        // D: new triangle s = (u, w, p) meets, across (w, p), the new triangle whose boundary edge starts at w
        T += 2;
        for (int s = tid; s < T; s += DT_THREADS) {
            if (d.fa[s] != 2) continue;
            const int s2 = d.vst[d.tv[3 * s + 1]];
            if ((unsigned)s2 >= (unsigned)T) {
                s_err = 1;
                continue;
            }
            d.tn[3 * s] = s2;
            d.tn[3 * s2 + 1] = s;
        }
        __syncthreads();
        if (s_err) return DT_INTERNAL;
    }
    // the real triangles in slot order, ghosts as -1
    int n_out = 0;
    for (int base = 0; base < T; base += DT_THREADS) {
        const int t = base + tid;
        const bool real = t < T && d.tv[3 * t] != G && d.tv[3 * t + 1] != G && d.tv[3 * t + 2] != G;
        int2 total;
        const int2 pre = dt_scan2(real, 0, s_wave, total);
        if (t < T) d.fre[t] = real ? n_out + pre.x : -1;
        n_out += total.x;
    }
    __syncthreads();
    if (n_out > room) return DT_NO_ROOM;
    for (int t = tid; t < T; t += DT_THREADS) {
        const int o = d.fre[t];
        if (o < 0) continue;
        for (int j = 0; j < 3; ++j) {
            simp[3 * (size_t)o + j] = d.perm[d.tv[3 * t + j]];
            neigh[3 * (size_t)o + j] = d.fre[d.tn[3 * t + j]];
        }
    }
    if (tid == 0) *n_tri = n_out;
    return DT_OK;
}

// pts [sum N] the call's points, pt_off [n_art + 1]; article a writes its triangles from tri_off_cap[a] on (2 * pt_off[a] when
// tri_off_cap is null) into simplices / neighbors [.][3] (indices local to the article, -1 = no neighbour), their number into
// n_tri[a] and its status into status[a].  scratch: DT_WORDS_PER_POINT + 1 words per point of the call, read only by articles over
// DT_LDS_POINTS (may be null when there is none).
__global__ void __launch_bounds__(DT_THREADS) dt_kernel(const int2* __restrict__ pts, const int* __restrict__ pt_off,
                                                        const int* __restrict__ tri_off_cap, int* __restrict__ scratch,
                                                        int* __restrict__ simplices, int* __restrict__ neighbors, int* __restrict__ n_tri,
                                                        int* __restrict__ status) {
    __shared__ int s_tab[DT_WORDS_PER_POINT * DT_LDS_POINTS + 1];
    const int a = blockIdx.x;
    const int p0 = pt_off[a], N = pt_off[a + 1] - p0;
    const size_t t0 = tri_off_cap ? (size_t)tri_off_cap[a] : 2 * (size_t)p0;
    const int room = tri_off_cap ? tri_off_cap[a + 1] - tri_off_cap[a] : 2 * N;
    int* base = N <= DT_LDS_POINTS ? s_tab : scratch + (size_t)(DT_WORDS_PER_POINT + 1) * p0;
    const int st = dt_article(pts + p0, N, dt_tables(base, N), simplices + 3 * t0, neighbors + 3 * t0, room, n_tri + a);
    if (threadIdx.x == 0) status[a] = st;
}

// tri_off [n_art + 1]: the exclusive sums of n_tri, by one workgroup
__global__ void __launch_bounds__(DT_THREADS) dt_offsets_kernel(const int* __restrict__ n_tri, int n_art, int* __restrict__ tri_off) {
    __shared__ int2 s_wave[DT_WAVES];
    int run = 0;
    for (int base = 0; base < n_art; base += DT_THREADS) {
        const int a = base + (int)threadIdx.x;
        const int v = a < n_art ? n_tri[a] : 0;
        int2 total;
        const int2 pre = dt_scan2(v, 0, s_wave, total);
        if (a < n_art) tri_off[a] = run + pre.x;
        run += total.x;
    }
    if (threadIdx.x == 0) tri_off[n_art] = run;
}

// the triangles of article a from 2 * pt_off[a] of the roomy tables to tri_off[a] of the packed ones
__global__ void __launch_bounds__(DT_THREADS) dt_pack_kernel(const int* __restrict__ pt_off, const int* __restrict__ tri_off,
                                                             const int* __restrict__ simp_in, const int* __restrict__ neigh_in,
                                                             int* __restrict__ simp_out, int* __restrict__ neigh_out) {
    const int a = blockIdx.x;
    const size_t src = 6 * (size_t)pt_off[a], dst = 3 * (size_t)tri_off[a];
    const int n = 3 * (tri_off[a + 1] - tri_off[a]);
    for (int i = threadIdx.x; i < n; i += DT_THREADS) {
        simp_out[dst + i] = simp_in[src + i];
        neigh_out[dst + i] = neigh_in[src + i];
    }
}

}  // namespace asep
