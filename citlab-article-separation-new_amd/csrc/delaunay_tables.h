// Limits of the device Delaunay triangulation (delaunay_kernels.h) and the host checks of the tables a caller hands to
// asep_delaunay / asep_alpha_shapes_points, whose kernel indexes with them unchecked.  Plain C++17 without HIP:
// tests/delaunay_tables_check.cpp runs the checks on the CPU under the sanitizers.
#pragma once
#include <climits>
#include <cstdint>

#include "batch_tables.h"

namespace asep {

// ---- the exact predicates' bound ----------------------------------------------------------------------------------------
// Points are translated to the article's bounding-box origin; an article is triangulated on the device only when both
// extents (max - min) are at most DT_MAX_EXTENT = 2^14 - 1.  Then, for any two points, |dx|, |dy| <= 2^14 - 1 < 2^14:
//   * a difference fits 15 bits signed;
//   * a 2x2 minor dx1 * dy2 - dx2 * dy1 is below 2 * 2^28 = 2^29 in magnitude (orientation test, int64 with room);
//   * a squared length dx^2 + dy^2 is below 2^29;
//   * the in-circle determinant is a sum of three (squared length) * (minor) products, below 3 * 2^58 < 2^63: int64.
constexpr int DT_EXTENT_BITS = 14;
constexpr int DT_MAX_EXTENT = (1 << DT_EXTENT_BITS) - 1;
constexpr int64_t DT_MINOR_BOUND = 2 * ((int64_t)1 << (2 * DT_EXTENT_BITS));         // 2^29
constexpr int64_t DT_LENGTH_BOUND = 2 * ((int64_t)1 << (2 * DT_EXTENT_BITS));        // 2^29
static_assert(DT_MAX_EXTENT < (1 << DT_EXTENT_BITS), "a coordinate difference must stay below 2^14");
static_assert(DT_LENGTH_BOUND <= INT64_MAX / 3 / DT_MINOR_BOUND, "the in-circle determinant must fit int64");
static_assert(2 * DT_EXTENT_BITS <= 30, "the packed (x << 14 | y) sort key must fit a non-negative int");

// ---- the working tables of one article ----------------------------------------------------------------------------------
// n points give at most 2n - 2 triangles counting the ghost triangles of the hull edges (2n - 2 - h real ones, h ghosts), so
// 2n slots.  In 32-bit words: sort keys n, sorted position -> point n, one slot per vertex n + 1, corners 3 * 2n, neighbours
// 3 * 2n, free-slot list 2n, two flag bytes per slot n: 18n + 1, plus DT_LDS_RESERVED words of scan and control variables.
constexpr int DT_WORDS_PER_POINT = 18;
constexpr int DT_LDS_RESERVED = 64;
constexpr int DT_LDS_WORDS = 64 * 1024 / 4;          // the 64 KiB one workgroup can declare statically
// 896 points = 16,129 words = 63.0 KiB; the CU's 160 KiB LDS (MI355X) then holds two such workgroups side by side.
constexpr int DT_LDS_POINTS = 896;
static_assert(DT_WORDS_PER_POINT * DT_LDS_POINTS + 1 + DT_LDS_RESERVED <= DT_LDS_WORDS, "the tables must fit 64 KiB of LDS");
static_assert(DT_WORDS_PER_POINT * (DT_LDS_POINTS + 32) + 1 + DT_LDS_RESERVED > DT_LDS_WORDS, "DT_LDS_POINTS is the budget's, to 32 points");

// out_status of an article
enum : int32_t {
    DT_OK = 0,
    DT_FEW_POINTS = 1,       // fewer than 3 distinct points
    DT_COLLINEAR = 2,        // all distinct points on one line
    DT_BOX_TOO_LARGE = 3,    // the bounding box is wider or taller than DT_MAX_EXTENT
    DT_INTERNAL = 4,         // a table went inconsistent (never seen; the loops end on it instead of trusting it)
    DT_NO_ROOM = 5,          // more triangles than the caller's slice holds
};

// the most triangles n points can give: 2n - 2 - h with a hull of h >= 3
inline int64_t dt_max_triangles(int64_t n) { return n >= 3 ? 2 * n - 5 : 0; }

// asep_delaunay: article a holds the points pt_off[a] .. pt_off[a + 1] and owns the triangles tri_off_cap[a] .. tri_off_cap[a + 1] of
// the output tables, which must have room for every triangulation of that many points.
inline bool check_delaunay_tables(const char* fn, int n_art, const int32_t* pt_off, const int32_t* tri_off_cap) {
    if (!check_offsets(fn, "pt_off", pt_off, n_art) || !check_offsets(fn, "tri_off_cap", tri_off_cap, n_art)) return false;
    if (tri_off_cap[n_art] > INT_MAX / 3) {
        set_error("%s: room for %d triangles in one call, at most %d", fn, tri_off_cap[n_art], INT_MAX / 3);
        return false;
    }
    for (int a = 0; a < n_art; ++a) {
        const int64_t n = pt_off[a + 1] - pt_off[a], room = tri_off_cap[a + 1] - tri_off_cap[a];
        if (room < dt_max_triangles(n)) {
            set_error("%s: article %d has room for %lld triangles, its %lld points can give %lld", fn, a, (long long)room, (long long)n,
                      (long long)dt_max_triangles(n));
            return false;
        }
    }
    return true;
}

// asep_alpha_shapes_points: the engine gives article a the triangles 2 * pt_off[a] .. of its own tables and DT_WORDS_PER_POINT words
// of scratch a point, so the call's point count is bounded by what an int indexes.
inline bool check_points_total(const char* fn, int64_t n_pts) {
    const int64_t most = INT_MAX / (3 * 2) < INT_MAX / (DT_WORDS_PER_POINT + 1) ? INT_MAX / (3 * 2) : INT_MAX / (DT_WORDS_PER_POINT + 1);
    if (n_pts > most) {
        set_error("%s: %lld points in one call, at most %lld", fn, (long long)n_pts, (long long)most);
        return false;
    }
    return true;
}

}  // namespace asep
