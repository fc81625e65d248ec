// Host checks of the tables a caller hands to the edge feature engine (edge_feature_engine.hip), whose kernels index with them
// unchecked, and the sizes the engine derives from them.  Plain C++17 without HIP: tests/edge_tables_check.cpp runs them on the CPU
// under the sanitizers.
#pragma once
#include <cstdint>

#include "batch_tables.h"

namespace asep {

constexpr int32_t EDGE_COORD_MAX = 1 << 20;   // ASEP_EDGE_COORD_MAX: doubled coordinates below 2^22, cross products below 2^47

// One ragged list of polygons over pages: page k holds the polygons poly_off[k] .. poly_off[k+1]-1, polygon r the points
// pts[pt_off[r] .. pt_off[r+1]-1][2].  Every polygon has a point, every coordinate lies within the bound.
inline bool check_polygons(const char* fn, const char* what, const char* off_name, const char* pt_off_name, int n_pages,
                           const int32_t* poly_off, const int32_t* pt_off, const int32_t* pts) {
    if (!check_offsets(fn, off_name, poly_off, n_pages)) return false;
    const int n = poly_off[n_pages];
    if (n && !pt_off) {
        set_error("%s: null argument (%s)", fn, pt_off_name);
        return false;
    }
    if (!n) return true;
    if (pt_off[0] != 0) {
        set_error("%s: %s must start at 0 (starts at %d)", fn, pt_off_name, pt_off[0]);
        return false;
    }
    for (int k = 0; k < n_pages; ++k)
        for (int r = poly_off[k]; r < poly_off[k + 1]; ++r)
            if ((int64_t)pt_off[r + 1] - pt_off[r] < 1) {
                set_error("%s: %s %d of page %d has no points (%s %d -> %d)", fn, what, r - poly_off[k], k, pt_off_name, pt_off[r],
                          pt_off[r + 1]);
                return false;
            }
    if (!pts) {
        set_error("%s: null argument (the points of the %ss)", fn, what);
        return false;
    }
    for (int k = 0; k < n_pages; ++k)
        for (int r = poly_off[k]; r < poly_off[k + 1]; ++r)
            for (int i = pt_off[r]; i < pt_off[r + 1]; ++i)
                for (int c = 0; c < 2; ++c) {
                    const int32_t v = pts[2 * (int64_t)i + c];
                    if (v < -EDGE_COORD_MAX || v > EDGE_COORD_MAX) {
                        set_error("%s: point %d of %s %d of page %d has the coordinate %d, outside [-%d, %d] (the bound that keeps the "
                                  "int64 cross products exact)", fn, i - pt_off[r], what, r - poly_off[k], k, v, EDGE_COORD_MAX,
                                  EDGE_COORD_MAX);
                        return false;
                    }
                }
    return true;
}

// The edges of the pages: both ends are regions of the edge's own page.  node_off has been checked.
inline bool check_edges(const char* fn, int n_pages, const int32_t* node_off, const int32_t* edge_off, const int32_t* edges) {
    if (!check_offsets(fn, "edge_off", edge_off, n_pages)) return false;
    if (edge_off[n_pages] && !edges) {
        set_error("%s: null argument (edges)", fn);
        return false;
    }
    for (int k = 0; k < n_pages; ++k) {
        const int n = node_off[k + 1] - node_off[k];
        for (int e = edge_off[k]; e < edge_off[k + 1]; ++e)
            for (int c = 0; c < 2; ++c) {
                const int32_t v = edges[2 * (int64_t)e + c];
                if (v < 0 || v >= n) {
                    set_error("%s: edge %d of page %d names region %d, the page has %d regions", fn, e - edge_off[k], k, v, n);
                    return false;
                }
            }
    }
    return true;
}

// The widest hull row of a call: the largest number of points the two regions of one edge have together (0 without edges);
// *which = that edge.  The tables have been checked.
inline int64_t widest_edge(int n_pages, const int32_t* node_off, const int32_t* node_pt_off, const int32_t* edge_off,
                           const int32_t* edges, int* which_page, int* which_edge) {
    int64_t widest = 0;
    for (int k = 0; k < n_pages; ++k)
        for (int e = edge_off[k]; e < edge_off[k + 1]; ++e) {
            const int a = node_off[k] + edges[2 * (int64_t)e], b = node_off[k] + edges[2 * (int64_t)e + 1];
            const int64_t m = ((int64_t)node_pt_off[a + 1] - node_pt_off[a]) + ((int64_t)node_pt_off[b + 1] - node_pt_off[b]);
            if (m > widest) {
                widest = m;
                *which_page = k;
                *which_edge = e - edge_off[k];
            }
        }
    return widest;
}

// out_hull [E][hull_cap][2] against the edges and the byte budget of a call.
inline bool check_hull_room(const char* fn, int n_pages, const int32_t* node_off, const int32_t* node_pt_off, const int32_t* edge_off,
                            const int32_t* edges, int hull_cap, long long budget) {
    if (hull_cap < 0 || budget <= 0) {
        set_error("%s: hull_cap %d must not be negative and hull_budget_bytes %lld must be positive", fn, hull_cap, budget);
        return false;
    }
    int k = 0, e = 0;
    const int64_t widest = widest_edge(n_pages, node_off, node_pt_off, edge_off, edges, &k, &e);
    if (widest * 8 > budget) {
        set_error("%s: edge %d of page %d joins regions of %lld points: its hull row of %lld bytes alone exceeds the budget of %lld "
                  "bytes, no split of the edges helps", fn, e, k, (long long)widest, (long long)widest * 8, budget);
        return false;
    }
    if (widest > hull_cap) {
        set_error("%s: edge %d of page %d joins regions of %lld points, hull_cap is %d", fn, e, k, (long long)widest, hull_cap);
        return false;
    }
    const int64_t bytes = (int64_t)edge_off[n_pages] * hull_cap * 8;
    if (bytes > budget) {
        set_error("%s: %d edges x hull_cap %d x 8 bytes = %lld bytes exceed the budget of %lld bytes: split the edges over several "
                  "calls", fn, edge_off[n_pages], hull_cap, (long long)bytes, budget);
        return false;
    }
    return true;
}

}  // namespace asep
