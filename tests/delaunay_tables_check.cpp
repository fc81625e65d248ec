// Host check of check_delaunay_tables / check_points_total (csrc/delaunay_tables.h): which offset tables asep_delaunay and
// asep_alpha_shapes_points accept before they allocate or launch, and what the refusals say.  Every table is a heap array of exactly
// its length, so a read outside it stops the program under the address sanitizer.  Stand-alone: built and run by
// tests/test_delaunay_host.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "delaunay_tables.h"

namespace {
char g_msg[512];
int g_cases = 0;
}  // namespace

void asep::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
}

namespace {

using Table = std::vector<int32_t>;

#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            std::fprintf(stderr, "%s:%d: %s (message: \"%s\")\n", __FILE__, __LINE__, #cond, g_msg);      \
            std::exit(1);                                                                                 \
        }                                                                                                 \
    } while (0)
#define ACCEPTED(call)                                                                                    \
    do {                                                                                                  \
        g_msg[0] = 0;                                                                                     \
        CHECK(call);                                                                                      \
        CHECK(g_msg[0] == 0);                                                                             \
        ++g_cases;                                                                                        \
    } while (0)
#define REFUSED(call, want)                                                                               \
    do {                                                                                                  \
        g_msg[0] = 0;                                                                                     \
        CHECK(!(call));                                                                                   \
        CHECK(std::strcmp(g_msg, want) == 0);                                                             \
        ++g_cases;                                                                                        \
    } while (0)

bool tables(const Table& pt_off, const Table& cap_off) {
    return asep::check_delaunay_tables("fn", (int)pt_off.size() - 1, pt_off.data(), cap_off.data());
}

}  // namespace

int main() {
    static_assert(asep::DT_MAX_EXTENT == 16383 && asep::DT_LDS_POINTS == 896, "the documented limits");
    CHECK(asep::dt_max_triangles(0) == 0 && asep::dt_max_triangles(2) == 0 && asep::dt_max_triangles(3) == 1 &&
          asep::dt_max_triangles(4) == 3 && asep::dt_max_triangles(1000) == 1995);
    ACCEPTED(tables({0}, {0}));                                                              // no articles
    ACCEPTED(tables({0, 0, 2}, {0, 0, 0}));                                                  // nothing to triangulate needs no room
    ACCEPTED(tables({0, 3, 7, 7, 107}, {0, 1, 4, 4, 199}));                                  // exactly 2n - 5 each
    ACCEPTED(tables({0, 3, 7}, {0, 6, 14}));                                                 // the 2n the Python side gives
    REFUSED(tables({0, 3, 7}, {0, 0, 3}), "fn: article 0 has room for 0 triangles, its 3 points can give 1");
    REFUSED(tables({0, 3, 7}, {0, 1, 3}), "fn: article 1 has room for 2 triangles, its 4 points can give 3");
    REFUSED(tables({0, 3, 103}, {0, 1, 195}), "fn: article 1 has room for 194 triangles, its 100 points can give 195");
    REFUSED(tables({1, 3}, {0, 6}), "fn: pt_off must start at 0 (starts at 1)");
    REFUSED(tables({0, 5, 3}, {0, 10, 10}), "fn: pt_off 1 (5 -> 3) is decreasing");
    REFUSED(tables({0, 3, 6}, {0, 6, 2}), "fn: tri_off_cap 1 (6 -> 2) is decreasing");
    REFUSED(tables({0, 3}, {2, 8}), "fn: tri_off_cap must start at 0 (starts at 2)");
    REFUSED(tables({0, 3, INT32_MAX}, {0, 6, INT32_MAX}), "fn: room for 2147483647 triangles in one call, at most 715827882");
    // a difference of offsets that does not fit an int is still compared, not wrapped
    REFUSED(tables({0, INT32_MAX}, {0, 715827882}), "fn: article 0 has room for 715827882 triangles, its 2147483647 points can give 4294967289");
    ACCEPTED(asep::check_points_total("fn", 0));
    ACCEPTED(asep::check_points_total("fn", INT32_MAX / 19));
    REFUSED(asep::check_points_total("fn", INT32_MAX / 19 + 1), "fn: 113025456 points in one call, at most 113025455");
    std::printf("delaunay tables ok: %d cases\n", g_cases);
    return 0;
}
