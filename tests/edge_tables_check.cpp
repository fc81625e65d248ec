// Host check of csrc/edge_tables.h: which tables the edge feature engine accepts, and what the refusals say.  Every table is a heap
// array of exactly its length, so a read outside it stops the program under the address sanitizer.
// Stand-alone: built and run by tests/test_edge_features_host.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "edge_tables.h"

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
constexpr int32_t LIM = 1 << 20;

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

const int32_t* ptr(const Table& t) { return t.empty() ? nullptr : t.data(); }

bool polygons(const Table& poly_off, const Table& pt_off, const Table& pts) {
    return asep::check_polygons("fn", "region", "node_off", "node_pt_off", (int)poly_off.size() - 1, poly_off.data(), ptr(pt_off), ptr(pts));
}

void check_polygon_tables() {
    ACCEPTED(polygons({0}, {}, {}));                                                       // no pages
    ACCEPTED(polygons({0, 0, 0}, {}, {}));                                                 // pages without polygons: pt_off is not read
    ACCEPTED(polygons({0, 1}, {0, 1}, {7, -7}));                                           // one polygon of one point
    ACCEPTED(polygons({0, 2, 2, 3}, {0, 3, 4, 6}, {0, 0, 5, 0, 5, 5, 9, 9, 1, 2, 3, 4}));  // an empty page in the middle
    ACCEPTED(polygons({0, 1}, {0, 2}, {LIM, -LIM, -LIM, LIM}));                            // the bound itself

    REFUSED(polygons({1, 2}, {0, 1}, {0, 0}), "fn: node_off must start at 0 (starts at 1)");
    REFUSED(polygons({0, 2, 1}, {0, 1, 2}, {0, 0, 1, 1}), "fn: node_off 1 (2 -> 1) is decreasing");
    REFUSED(polygons({0, 1}, {}, {}), "fn: null argument (node_pt_off)");
    REFUSED(polygons({0, 1}, {1, 2}, {0, 0, 1, 1}), "fn: node_pt_off must start at 0 (starts at 1)");
    REFUSED(polygons({0, 2}, {0, 0, 1}, {0, 0}), "fn: region 0 of page 0 has no points (node_pt_off 0 -> 0)");
    REFUSED(polygons({0, 1, 3}, {0, 1, 2, 2}, {0, 0, 1, 1}), "fn: region 1 of page 1 has no points (node_pt_off 2 -> 2)");   // the last
    REFUSED(polygons({0, 2}, {0, 2, 1}, {0, 0, 1, 1}), "fn: region 1 of page 0 has no points (node_pt_off 2 -> 1)");        // decreasing
    REFUSED(polygons({0, 1}, {0, 1}, {}), "fn: null argument (the points of the regions)");
    REFUSED(polygons({0, 1, 2}, {0, 2, 3}, {0, 0, 1, 1, 5, LIM + 1}),
            "fn: point 0 of region 0 of page 1 has the coordinate 1048577, outside [-1048576, 1048576] (the bound that keeps the int64 cross "
            "products exact)");
    REFUSED(polygons({0, 1}, {0, 2}, {0, 0, -LIM - 1, 1}),
            "fn: point 1 of region 0 of page 0 has the coordinate -1048577, outside [-1048576, 1048576] (the bound that keeps the int64 cross "
            "products exact)");
    REFUSED(polygons({0, 1}, {0, 1}, {INT32_MIN, 0}),
            "fn: point 0 of region 0 of page 0 has the coordinate -2147483648, outside [-1048576, 1048576] (the bound that keeps the int64 "
            "cross products exact)");
}

bool edges(const Table& node_off, const Table& edge_off, const Table& e) {
    return asep::check_edges("fn", (int)node_off.size() - 1, node_off.data(), edge_off.data(), ptr(e));
}

void check_edge_tables() {
    ACCEPTED(edges({0}, {0}, {}));
    ACCEPTED(edges({0, 2, 5}, {0, 0, 0}, {}));                                             // no edges
    ACCEPTED(edges({0, 2, 2, 5}, {0, 2, 2, 4}, {0, 1, 1, 0, 2, 0, 1, 1}));                 // indices within the page; a self loop
    REFUSED(edges({0, 2}, {0, 1}, {}), "fn: null argument (edges)");
    REFUSED(edges({0, 2}, {0, -1}, {}), "fn: edge_off 0 (0 -> -1) is decreasing");
    REFUSED(edges({0, 2, 5}, {0, 1, 2}, {0, 2, 0, 1}), "fn: edge 0 of page 0 names region 2, the page has 2 regions");
    REFUSED(edges({0, 2, 5}, {0, 1, 3}, {0, 1, 0, 1, 3, 2}), "fn: edge 1 of page 1 names region 3, the page has 3 regions");   // not a global index
    REFUSED(edges({0, 2, 5}, {0, 1, 2}, {0, 1, -1, 0}), "fn: edge 0 of page 1 names region -1, the page has 3 regions");
    REFUSED(edges({0, 0}, {0, 1}, {0, 0}), "fn: edge 0 of page 0 names region 0, the page has 0 regions");
}

bool room(const Table& node_off, const Table& node_pt_off, const Table& edge_off, const Table& e, int cap, long long budget) {
    return asep::check_hull_room("fn", (int)node_off.size() - 1, node_off.data(), ptr(node_pt_off), edge_off.data(), ptr(e), cap, budget);
}

void check_hull_tables() {
    // two pages: regions of 3 and 4 points; of 2, 10 and 1 points
    const Table node_off{0, 2, 5}, pt_off{0, 3, 7, 9, 19, 20}, edge_off{0, 2, 4}, e{0, 1, 1, 1, 0, 2, 2, 1};
    ACCEPTED(room({0}, {}, {0}, {}, 0, 1));                                                // nothing to do
    ACCEPTED(room(node_off, pt_off, edge_off, e, 11, 4 * 11 * 8));                         // exactly enough
    ACCEPTED(room(node_off, pt_off, edge_off, e, 64, 1 << 20));
    REFUSED(room(node_off, pt_off, edge_off, e, 10, 1 << 20), "fn: edge 1 of page 1 joins regions of 11 points, hull_cap is 10");
    REFUSED(room(node_off, pt_off, edge_off, e, 11, 4 * 11 * 8 - 1),
            "fn: 4 edges x hull_cap 11 x 8 bytes = 352 bytes exceed the budget of 351 bytes: split the edges over several calls");
    REFUSED(room(node_off, pt_off, edge_off, e, 11, 87),
            "fn: edge 1 of page 1 joins regions of 11 points: its hull row of 88 bytes alone exceeds the budget of 87 bytes, no split of the "
            "edges helps");
    REFUSED(room(node_off, pt_off, edge_off, e, -1, 100), "fn: hull_cap -1 must not be negative and hull_budget_bytes 100 must be positive");
    REFUSED(room(node_off, pt_off, edge_off, e, 11, 0), "fn: hull_cap 11 must not be negative and hull_budget_bytes 0 must be positive");
}

}  // namespace

int main() {
    check_polygon_tables();
    check_edge_tables();
    check_hull_tables();
    std::printf("edge tables ok: %d cases\n", g_cases);
    return 0;
}
