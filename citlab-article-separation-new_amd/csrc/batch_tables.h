// Host checks of the offset and member tables a caller hands to the batched evaluation engines (text block detection, measure,
// heading grid, clustering grid), whose kernels index with them unchecked.  Plain C++17 without HIP:
// tests/batch_tables_check.cpp and tests/alpha_shape_tables_check.cpp (the triangulations of the alpha-shape engine) run them on the CPU
// under the sanitizers.
#pragma once
#include <cstdint>

namespace asep {

void set_error(const char* fmt, ...);

// off[0 .. n] starts at 0 and never decreases; with `nonempty`, every entry holds at least one element.
inline bool check_offsets(const char* fn, const char* what, const int32_t* off, int n, bool nonempty = false) {
    if (off[0] != 0) {
        set_error("%s: %s must start at 0 (starts at %d)", fn, what, off[0]);
        return false;
    }
    for (int k = 0; k < n; ++k)
        if ((int64_t)off[k + 1] - off[k] < (nonempty ? 1 : 0)) {
            set_error("%s: %s %d (%d -> %d) is %s", fn, what, k, off[k], off[k + 1], nonempty ? "empty or decreasing" : "decreasing");
            return false;
        }
    return true;
}

// Two levels: page k holds the groups group_off[k] .. group_off[k + 1], group g lists the entries member_off[g] .. member_off[g + 1]
// of `members`, each an index into the page's item_off[k + 1] - item_off[k] lines.  The three offset tables have been checked.
inline bool check_members(const char* fn, const char* group_name, int n_pages, const int32_t* item_off, const int32_t* group_off,
                          const int32_t* member_off, const int32_t* members) {
    for (int k = 0; k < n_pages; ++k) {
        const int n = item_off[k + 1] - item_off[k];
        for (int g = group_off[k]; g < group_off[k + 1]; ++g)
            for (int e = member_off[g]; e < member_off[g + 1]; ++e)
                if (members[e] < 0 || members[e] >= n) {
                    set_error("%s: %s %d of page %d lists line %d, the page has %d lines", fn, group_name, g - group_off[k], k,
                              members[e], n);
                    return false;
                }
    }
    return true;
}

// Triangulations of the alpha-shape engine: page k holds the articles art_off[k] .. art_off[k + 1], article a the points
// pt_off[a] .. pt_off[a + 1] and the triangles tri_off[a] .. tri_off[a + 1] of `simplices` / `neighbors` ([.][3], indices local to the
// article).  A corner is one of the article's points, a neighbour one of its triangles or -1.  The three offset tables have been checked.
inline bool check_triangles(const char* fn, int n_pages, const int32_t* art_off, const int32_t* pt_off, const int32_t* tri_off,
                            const int32_t* simplices, const int32_t* neighbors) {
    for (int k = 0; k < n_pages; ++k)
        for (int a = art_off[k]; a < art_off[k + 1]; ++a) {
            const int n = pt_off[a + 1] - pt_off[a], nt = tri_off[a + 1] - tri_off[a];
            for (int64_t e = 3 * (int64_t)tri_off[a]; e < 3 * (int64_t)tri_off[a + 1]; ++e) {
                const int t = (int)(e / 3 - tri_off[a]);
                if (simplices[e] < 0 || simplices[e] >= n) {
                    set_error("%s: triangle %d of article %d of page %d has corner %d, the article has %d points", fn, t, a - art_off[k], k,
                              simplices[e], n);
                    return false;
                }
                if (neighbors[e] < -1 || neighbors[e] >= nt) {
                    set_error("%s: triangle %d of article %d of page %d has neighbour %d, the article has %d triangles", fn, t,
                              a - art_off[k], k, neighbors[e], nt);
                    return false;
                }
            }
        }
    return true;
}

}  // namespace asep
