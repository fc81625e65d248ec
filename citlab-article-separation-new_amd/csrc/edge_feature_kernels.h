// Kernels of the edge feature engine (include/asep_hip.h, "edge features" block): feature_generation.py's per-edge and per-pair rules as
// integer geometry.  Coordinates lie in [-2^20, 2^20] (edge_tables.h), a box centre is a half-integer, so every comparison against a
// centre or a mean is made in DOUBLED coordinates (|v| <= 2^22, differences <= 2^23, cross products <= 2^47 in int64): the signs and
// closed ranges come out as the host's doubles give them, which are exact at these sizes.  No floating point.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace asep {

constexpr int EF_BLOCK = 256;       // threads of the flag and pair kernels: one edge / one matrix element each
constexpr int EF_SEP_CHUNK = 64;    // separators of a page staged through LDS at a time
constexpr int EF_WAVE = 64;

enum { EF_RULE_BB = 0, EF_RULE_LINE = 1 };
enum { EF_SEP_NONE = 0, EF_SEP_HORIZONTAL = 1, EF_SEP_VERTICAL = 2, EF_SEP_OTHER = 3 };

struct EfBox { int32_t min_x, max_x, min_y, max_y; };   // get_bounding_box's order

// largest k with off[k] <= x, for 0 <= x < off[n]
template <class T>
__device__ inline int ef_find(const T* __restrict__ off, int n, T x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// get_bounding_box of every polygon of one ragged list, one thread per polygon
__global__ void __launch_bounds__(EF_BLOCK) edge_boxes_kernel(const int32_t* __restrict__ pt_off, const int2* __restrict__ pts, int n,
                                                              EfBox* __restrict__ boxes) {
    const int r = blockIdx.x * EF_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int i0 = pt_off[r], i1 = pt_off[r + 1];
    int2 p = pts[i0];
    EfBox b{p.x, p.x, p.y, p.y};
    for (int i = i0 + 1; i < i1; ++i) {
        p = pts[i];
        b.min_x = min(b.min_x, p.x); b.max_x = max(b.max_x, p.x);
        b.min_y = min(b.min_y, p.y); b.max_y = max(b.max_y, p.y);
    }
    boxes[r] = b;
}

// _sep_orientation(...) == "vertical": the tag, or without one height / width >= 5 with both clamped to >= 1
__device__ inline bool ef_ratio_vertical(const EfBox& s) {
    const int w = max(s.max_x - s.min_x, 1), h = max(s.max_y - s.min_y, 1);
    return !(h < 5 * w);
}
__device__ inline bool ef_bb_vertical(const EfBox& s, int orient) {
    return orient == EF_SEP_NONE ? ef_ratio_vertical(s) : orient == EF_SEP_VERTICAL;
}

// is_vertically_separated / is_horizontally_separated, the separator's means doubled
__device__ inline bool ef_vertically_separated(const EfBox& a, const EfBox& b, const EfBox& s) {
    const int mx = s.min_x + s.max_x;
    if (!((2 * a.max_x <= mx && mx <= 2 * b.min_x) || (2 * b.max_x <= mx && mx <= 2 * a.min_x))) return false;
    return (a.max_y >= s.min_y && a.min_y <= s.max_y) || (b.max_y >= s.min_y && b.min_y <= s.max_y);
}
__device__ inline bool ef_horizontally_separated(const EfBox& a, const EfBox& b, const EfBox& s) {
    const int my = s.min_y + s.max_y;
    if (!((2 * a.min_y <= my && my <= 2 * b.max_y) || (2 * b.min_y <= my && my <= 2 * a.max_y))) return false;
    return !((a.max_x <= s.min_x && b.max_x <= s.min_x) || (a.min_x >= s.max_x && b.min_x >= s.max_x));
}

// _orient, _on_segment and segments_intersect on points in doubled coordinates
__device__ inline int ef_orient(int2 p, int2 q, int2 r) {
    const int64_t v = (int64_t)(q.x - p.x) * (r.y - p.y) - (int64_t)(q.y - p.y) * (r.x - p.x);
    return (v > 0) - (v < 0);
}
__device__ inline bool ef_on_segment(int2 p, int2 q, int2 r) {
    return min(p.x, q.x) <= r.x && r.x <= max(p.x, q.x) && min(p.y, q.y) <= r.y && r.y <= max(p.y, q.y);
}
__device__ inline bool ef_segments_intersect(int2 a1, int2 a2, int2 b1, int2 b2) {
    const int o1 = ef_orient(a1, a2, b1), o2 = ef_orient(a1, a2, b2), o3 = ef_orient(b1, b2, a1), o4 = ef_orient(b1, b2, a2);
    if (o1 != o2 && o3 != o4) return true;
    return (o1 == 0 && ef_on_segment(a1, a2, b1)) || (o2 == 0 && ef_on_segment(a1, a2, b2)) || (o3 == 0 && ef_on_segment(b1, b2, a1)) ||
           (o4 == 0 && ef_on_segment(b1, b2, a2));
}

__device__ inline int2 ef_doubled(int2 p) { return int2{2 * p.x, 2 * p.y}; }

// line_poly_intersection(segment, polygon): the polygon is closed on the fly unless its first point equals its last
__device__ inline bool ef_line_poly(int2 p, int2 q, const int2* __restrict__ poly, int n) {
    const int2 first = poly[0], last = poly[n - 1];
    const int n_seg = (first.x != last.x || first.y != last.y) ? n : n - 1;
    int2 v = ef_doubled(first);
    for (int i = 0; i < n_seg; ++i) {
        const int2 w = ef_doubled(poly[i + 1 < n ? i + 1 : 0]);
        if (ef_segments_intersect(p, q, v, w)) return true;
        v = w;
    }
    return false;
}

// the prior test of get_edge_separator_feature_line: the box corners in the reference's order (a bow-tie), or line_in_bounding_box
__device__ inline bool ef_line_meets_box(int2 p, int2 q, const EfBox& s) {
    const int2 c[4] = {{2 * s.min_x, 2 * s.min_y}, {2 * s.max_x, 2 * s.min_y}, {2 * s.min_x, 2 * s.max_y}, {2 * s.max_x, 2 * s.max_y}};
    const int n_seg = (c[0].x != c[3].x || c[0].y != c[3].y) ? 4 : 3;
    for (int i = 0; i < n_seg; ++i)
        if (ef_segments_intersect(p, q, c[i], c[(i + 1) & 3])) return true;
    return min(p.x, q.x) > 2 * s.min_x && max(p.x, q.x) < 2 * s.max_x && min(p.y, q.y) > 2 * s.min_y && max(p.y, q.y) < 2 * s.max_y;
}

// The separators sep_off[page] + c0 .. of one page in LDS: boxes, orientation, and where their points start
struct EfSepStage {
    EfBox box[EF_SEP_CHUNK];
    int32_t pt0[EF_SEP_CHUNK], npt[EF_SEP_CHUNK];
    uint8_t orient[EF_SEP_CHUNK];
};
__device__ inline void ef_stage(EfSepStage& st, int s0, int cnt, const EfBox* __restrict__ sep_box, const int32_t* __restrict__ sep_pt_off,
                                const uint8_t* __restrict__ sep_orient) {
    __syncthreads();   // the chunk before has been read
    if ((int)threadIdx.x < cnt) {
        const int s = s0 + threadIdx.x;
        st.box[threadIdx.x] = sep_box[s];
        st.pt0[threadIdx.x] = sep_pt_off[s];
        st.npt[threadIdx.x] = sep_pt_off[s + 1] - sep_pt_off[s];
        st.orient[threadIdx.x] = sep_orient[s];
    }
    __syncthreads();
}

// (horizontally_separated, vertically_separated) of every edge.  Block blk_off[k] .. blk_off[k+1]-1 take the edges of page k, one
// thread each; the page's separators pass through LDS in chunks.  A thread whose two flags are set skips the rest (the host breaks).
template <int RULE>
__global__ void __launch_bounds__(EF_BLOCK)
edge_flags_kernel(const int32_t* __restrict__ blk_off, int n_pages, const int32_t* __restrict__ node_off, const EfBox* __restrict__ node_box,
                  const int32_t* __restrict__ sep_off, const EfBox* __restrict__ sep_box, const int32_t* __restrict__ sep_pt_off,
                  const int2* __restrict__ sep_pts, const uint8_t* __restrict__ sep_orient, const int32_t* __restrict__ edge_off,
                  const int2* __restrict__ edges, uchar2* __restrict__ out_flags) {
    __shared__ EfSepStage st;
    const int k = ef_find(blk_off, n_pages, (int32_t)blockIdx.x);
    const int e = edge_off[k] + ((int)blockIdx.x - blk_off[k]) * EF_BLOCK + (int)threadIdx.x;
    const bool live = e < edge_off[k + 1];
    EfBox a{}, b{};
    int2 p{}, q{};
    if (live) {
        const int2 ab = edges[e];
        a = node_box[node_off[k] + ab.x];
        b = node_box[node_off[k] + ab.y];
        p = int2{a.min_x + a.max_x, a.min_y + a.max_y};   // the two box centres, doubled
        q = int2{b.min_x + b.max_x, b.min_y + b.max_y};
    }
    bool hor = false, ver = false;
    const int s_begin = sep_off[k], s_end = sep_off[k + 1];
    for (int s0 = s_begin; s0 < s_end; s0 += EF_SEP_CHUNK) {
        const int cnt = min(EF_SEP_CHUNK, s_end - s0);
        ef_stage(st, s0, cnt, sep_box, sep_pt_off, sep_orient);
        if (!live || (hor && ver)) continue;
        for (int i = 0; i < cnt && !(hor && ver); ++i) {
            const EfBox s = st.box[i];
            const int orient = st.orient[i];
            if (RULE == EF_RULE_BB) {
                if (ef_bb_vertical(s, orient)) ver = ver || ef_vertically_separated(a, b, s);
                else hor = hor || ef_horizontally_separated(a, b, s);
            } else {
                if (!ef_line_meets_box(p, q, s) || !ef_line_poly(p, q, sep_pts + st.pt0[i], st.npt[i])) continue;
                if (orient == EF_SEP_HORIZONTAL || !ef_ratio_vertical(s)) hor = true;
                else ver = true;
            }
        }
    }
    if (live) out_flags[e] = uchar2{(unsigned char)hor, (unsigned char)ver};
}

// The pair bits of every page: blocks blk_off[k] .. take the N_k x N_k elements of page k's matrix, one thread each; element (r, c)
// holds the bits of the pair (min, max), the diagonal 0.
__global__ void __launch_bounds__(EF_BLOCK)
edge_pair_bits_kernel(const int32_t* __restrict__ blk_off, int n_pages, const int32_t* __restrict__ node_off, const EfBox* __restrict__ node_box,
                      const uint8_t* __restrict__ node_heading, const int32_t* __restrict__ sep_off, const EfBox* __restrict__ sep_box,
                      const int32_t* __restrict__ sep_pt_off, const uint8_t* __restrict__ sep_orient, const int64_t* __restrict__ pair_off,
                      uint8_t* __restrict__ out_pairs) {
    __shared__ EfSepStage st;
    const int k = ef_find(blk_off, n_pages, (int32_t)blockIdx.x);
    const int n = node_off[k + 1] - node_off[k];
    const int idx = ((int)blockIdx.x - blk_off[k]) * EF_BLOCK + (int)threadIdx.x;
    const int row = idx / max(n, 1), col = idx - row * n;
    const bool live = idx < n * n;
    const bool pair = live && row != col;
    EfBox a{}, b{};
    unsigned bits = 0;
    if (pair) {
        const int i = node_off[k] + min(row, col), j = node_off[k] + max(row, col);
        a = node_box[i];
        b = node_box[j];
        const bool ha = node_heading[i] != 0, hb = node_heading[j] != 0;
        // is_aligned_heading_separated: exactly one heading, the boxes overlap in x, the heading lies below the other's lower edge
        if (ha != hb && a.min_x <= b.max_x && b.min_x <= a.max_x && (ha ? a.min_y >= b.max_y : b.min_y >= a.max_y)) bits = 1;
    }
    const int s_begin = sep_off[k], s_end = sep_off[k + 1];
    for (int s0 = s_begin; s0 < s_end; s0 += EF_SEP_CHUNK) {
        const int cnt = min(EF_SEP_CHUNK, s_end - s0);
        ef_stage(st, s0, cnt, sep_box, sep_pt_off, sep_orient);
        if (!pair || (bits & 2)) continue;
        for (int i = 0; i < cnt; ++i) {
            const EfBox s = st.box[i];
            if (ef_bb_vertical(s, st.orient[i])) continue;
            const int my = s.min_y + s.max_y;
            if (!((2 * a.min_y <= my && my <= 2 * b.max_y) || (2 * b.min_y <= my && my <= 2 * a.max_y))) continue;
            if (!(a.max_x >= s.min_x && b.max_x >= s.min_x && a.min_x <= s.max_x && b.min_x <= s.max_x)) continue;
            bits |= 2;
            break;
        }
    }
    if (live) out_pairs[pair_off[k] + idx] = (uint8_t)bits;
}

__device__ inline bool ef_less(int2 a, int2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

// The points of every region in convex_hull's sorting order, one wavefront per region: a point's place is the number of points
// that sort before it (equal points in their order of input, which no result can tell apart).
__global__ void __launch_bounds__(EF_WAVE) edge_sort_points_kernel(const int32_t* __restrict__ pt_off, const int2* __restrict__ pts,
                                                                 int2* __restrict__ sorted) {
    const int i0 = pt_off[blockIdx.x], n = pt_off[blockIdx.x + 1] - i0;
    for (int i = threadIdx.x; i < n; i += EF_WAVE) {
        const int2 p = pts[i0 + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int2 o = pts[i0 + j];
            rank += (ef_less(o, p) || (o.x == p.x && o.y == p.y && j < i)) ? 1 : 0;
        }
        sorted[i0 + rank] = p;
    }
}

__device__ inline bool ef_turn_left(int2 p, int2 q, int2 r) {
    return (int64_t)(q.x - p.x) * (r.y - p.y) - (int64_t)(r.x - p.x) * (q.y - p.y) > 0;
}

// One monotone chain over the merge of two sorted point lists, forwards (lower) or backwards (upper); the stack is `row`.
template <bool REVERSED>
__device__ inline int ef_chain(int2* __restrict__ row, const int2* __restrict__ A, int na, const int2* __restrict__ B, int nb) {
    int ia = REVERSED ? na - 1 : 0, ib = REVERSED ? nb - 1 : 0, len = 0;
    for (int t = 0; t < na + nb; ++t) {
        const bool has_a = REVERSED ? ia >= 0 : ia < na, has_b = REVERSED ? ib >= 0 : ib < nb;
        bool take_a = has_a;
        if (has_a && has_b) take_a = REVERSED ? !ef_less(A[ia], B[ib]) : !ef_less(B[ib], A[ia]);
        const int2 pt = take_a ? A[ia] : B[ib];
        if (take_a) ia += REVERSED ? -1 : 1; else ib += REVERSED ? -1 : 1;
        while (len > 1 && !ef_turn_left(row[len - 2], row[len - 1], pt)) --len;
        row[len++] = pt;
    }
    return len;
}

// convex_hull(points of a + points of b) of every edge, one thread per edge.  `work` [E][2 * cap] is the thread's stack: the lower chain
// from its start, the upper chain from the lower chain's last point (the same point, pts[-1]); lower[:-1] + upper[:-1] then stands at
// the start of the row.  A chain never holds more than the na + nb <= cap points it has seen, so 2 * cap entries suffice.  The first
// `cap` entries of the row are the output row (the hull has at most na + nb points), entries behind the count are zeroed.
__global__ void __launch_bounds__(EF_BLOCK)
edge_hull_kernel(const int32_t* __restrict__ edge_off, int n_pages, const int32_t* __restrict__ node_off,
                 const int32_t* __restrict__ node_pt_off, const int2* __restrict__ sorted, const int2* __restrict__ edges, int cap,
                 int2* __restrict__ work, int32_t* __restrict__ out_n) {
    const int e = blockIdx.x * EF_BLOCK + threadIdx.x;
    if (e >= edge_off[n_pages]) return;
    const int k = ef_find(edge_off, n_pages, (int32_t)e);
    const int2 ab = edges[e];
    const int ra = node_off[k] + ab.x, rb = node_off[k] + ab.y;
    const int2* A = sorted + node_pt_off[ra];
    const int2* B = sorted + node_pt_off[rb];
    const int na = node_pt_off[ra + 1] - node_pt_off[ra], nb = node_pt_off[rb + 1] - node_pt_off[rb];
    int2* row = work + (int64_t)e * 2 * cap;
    const int lower = ef_chain<false>(row, A, na, B, nb);
    const int upper = ef_chain<true>(row + lower - 1, A, na, B, nb);
    const int count = lower - 1 + upper - 1;
    for (int i = count; i < cap; ++i) row[i] = int2{0, 0};
    out_n[e] = count;
}

}  // namespace asep
