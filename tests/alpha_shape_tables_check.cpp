// Host check of check_triangles (csrc/batch_tables.h): which triangulations asep_alpha_shapes accepts before it allocates or launches,
// and what the refusals say.  Every table is a heap array of exactly its length, so a read outside it stops the program under the
// address sanitizer.  Stand-alone: built and run by tests/test_alpha_shape_host.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_tables.h"

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

bool triangles(const Table& art_off, const Table& pt_off, const Table& tri_off, const Table& simplices, const Table& neighbors) {
    return asep::check_triangles("fn", (int)art_off.size() - 1, art_off.data(), pt_off.data(), tri_off.data(),
                                 simplices.empty() ? nullptr : simplices.data(), neighbors.empty() ? nullptr : neighbors.data());
}

}  // namespace

int main() {
    ACCEPTED(triangles({0}, {0}, {0}, {}, {}));                                              // no pages
    ACCEPTED(triangles({0, 0, 0}, {0}, {0}, {}, {}));                                        // pages without articles
    ACCEPTED(triangles({0, 2}, {0, 0, 5}, {0, 0, 0}, {}, {}));                               // articles without triangles
    // two pages: one article of 4 points and 2 triangles; then one of 3 points and 1 triangle and one of 5 points and 2 triangles
    const Table art = {0, 1, 3}, pt = {0, 4, 7, 12}, tri = {0, 2, 3, 5};
    const Table simp = {0, 1, 2, 2, 3, 0, 0, 1, 2, 4, 0, 1, 1, 2, 4};
    const Table neigh = {-1, 1, -1, -1, -1, 0, -1, -1, -1, 1, -1, -1, -1, 0, -1};
    ACCEPTED(triangles(art, pt, tri, simp, neigh));

    Table s = simp, n = neigh;
    s[4] = 4;                                                                                // exactly the article's point count
    REFUSED(triangles(art, pt, tri, s, neigh), "fn: triangle 1 of article 0 of page 0 has corner 4, the article has 4 points");
    s = simp, s[0] = -1;
    REFUSED(triangles(art, pt, tri, s, neigh), "fn: triangle 0 of article 0 of page 0 has corner -1, the article has 4 points");
    s = simp, s[7] = 3;                                                                      // an index of the neighbouring article
    REFUSED(triangles(art, pt, tri, s, neigh), "fn: triangle 0 of article 0 of page 1 has corner 3, the article has 3 points");
    s = simp, s[14] = 5;                                                                     // the last corner of the call
    REFUSED(triangles(art, pt, tri, s, neigh), "fn: triangle 1 of article 1 of page 1 has corner 5, the article has 5 points");
    s = simp, s[9] = INT32_MAX;
    REFUSED(triangles(art, pt, tri, s, neigh), "fn: triangle 0 of article 1 of page 1 has corner 2147483647, the article has 5 points");
    n[1] = 2;                                                                                // exactly the article's triangle count
    REFUSED(triangles(art, pt, tri, simp, n), "fn: triangle 0 of article 0 of page 0 has neighbour 2, the article has 2 triangles");
    n = neigh, n[6] = 1;                                                                     // a triangle of the next article
    REFUSED(triangles(art, pt, tri, simp, n), "fn: triangle 0 of article 0 of page 1 has neighbour 1, the article has 1 triangles");
    n = neigh, n[14] = -2;                                                                   // only -1 stands for "none"
    REFUSED(triangles(art, pt, tri, simp, n), "fn: triangle 1 of article 1 of page 1 has neighbour -2, the article has 2 triangles");
    n = neigh, n[3] = INT32_MIN;
    REFUSED(triangles(art, pt, tri, simp, n), "fn: triangle 1 of article 0 of page 0 has neighbour -2147483648, the article has 2 triangles");
    // the corner is looked at before the neighbour of the same entry
    s = simp, s[0] = 9, n = neigh, n[0] = 9;
    REFUSED(triangles(art, pt, tri, s, n), "fn: triangle 0 of article 0 of page 0 has corner 9, the article has 4 points");
    std::printf("alpha shape tables ok: %d cases\n", g_cases);
    return 0;
}
