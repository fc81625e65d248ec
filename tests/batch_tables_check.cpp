// Host check of csrc/batch_tables.h: which offset and member tables the batched evaluation engines accept, and what the refusals say.
// Every table is a heap array of exactly its length, so a read outside it stops the program under the address sanitizer.
// Stand-alone: built and run by tests/test_batch_tables_host.py.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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
constexpr int32_t BIG = INT32_MAX;

#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) {                                                                                    \
            std::fprintf(stderr, "%s:%d: %s (message: \"%s\")\n", __FILE__, __LINE__, #cond, g_msg);      \
            std::exit(1);                                                                                 \
        }                                                                                                 \
    } while (0)

// the verdict, and that a refusal says exactly `want` while an accepted table leaves the error alone
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

bool offsets(const Table& off, bool nonempty = false) {
    return asep::check_offsets("fn", "tab_off", off.data(), (int)off.size() - 1, nonempty);
}

void check_offset_tables() {
    ACCEPTED(offsets({0}));                                                  // n = 0
    ACCEPTED(offsets({0}, true));
    ACCEPTED(offsets({0, 0, 0, 5, 5, 9, 9}));                                // empty pages
    ACCEPTED(offsets({0, 1}, true));                                         // a single item
    ACCEPTED(offsets({0, 1, 2, 3}, true));
    ACCEPTED(offsets({0, BIG}));
    ACCEPTED(offsets({0, 7, BIG, BIG}));
    ACCEPTED(offsets({0, BIG - 1, BIG}, true));

    REFUSED(offsets({-1, 2}), "fn: tab_off must start at 0 (starts at -1)");
    REFUSED(offsets({3, 5}, true), "fn: tab_off must start at 0 (starts at 3)");
    REFUSED(offsets({5}), "fn: tab_off must start at 0 (starts at 5)");      // n = 0 reads off[0] alone
    REFUSED(offsets({INT32_MIN, 0}), "fn: tab_off must start at 0 (starts at -2147483648)");

    REFUSED(offsets({0, -1, 4, 6}), "fn: tab_off 0 (0 -> -1) is decreasing");                  // at the first index,
    REFUSED(offsets({0, 4, 3, 6}), "fn: tab_off 1 (4 -> 3) is decreasing");                    // in the middle
    REFUSED(offsets({0, 4, 6, 5}), "fn: tab_off 2 (6 -> 5) is decreasing");                    // and at the last
    REFUSED(offsets({0, 4, 6, 5}, true), "fn: tab_off 2 (6 -> 5) is empty or decreasing");
    REFUSED(offsets({0, 4, 3, 2}), "fn: tab_off 1 (4 -> 3) is decreasing");                    // the first decrease is the one named
    REFUSED(offsets({0, BIG, INT32_MIN}), "fn: tab_off 1 (2147483647 -> -2147483648) is decreasing");

    ACCEPTED(offsets({0, 2, 2, 3}));                                                            // an empty entry, allowed
    REFUSED(offsets({0, 2, 2, 3}, true), "fn: tab_off 1 (2 -> 2) is empty or decreasing");     // and not
    REFUSED(offsets({0, 0}, true), "fn: tab_off 0 (0 -> 0) is empty or decreasing");
    REFUSED(offsets({0, BIG, BIG}, true), "fn: tab_off 1 (2147483647 -> 2147483647) is empty or decreasing");
}

bool members(const char* group_name, const Table& item_off, const Table& group_off, const Table& member_off, const Table& lines) {
    return asep::check_members("fn", group_name, (int)item_off.size() - 1, item_off.data(), group_off.data(), member_off.data(),
                               lines.empty() ? nullptr : lines.data());
}

void check_member_tables() {
    const char* const R = "region";
    const char* const B = "ground truth block";
    ACCEPTED(members(R, {0}, {0}, {0}, {}));                                                   // no pages
    ACCEPTED(members(R, {0, 0, 0}, {0, 0, 0}, {0}, {}));                                       // empty pages
    ACCEPTED(members(R, {0, 3, 3}, {0, 2, 3}, {0, 0, 0, 0}, {}));                              // empty groups, one on a page without lines
    ACCEPTED(members(B, {0, 1}, {0, 1}, {0, 1}, {0}));                                         // a single item
    ACCEPTED(members(B, {0, 1}, {0, 1}, {0, 3}, {0, 0, 0}));                                   // listed more than once
    // three pages of 3, 0 and 2 lines with 2, 1 and 2 groups: members are indices into their own page
    ACCEPTED(members(R, {0, 3, 3, 5}, {0, 2, 3, 5}, {0, 2, 3, 3, 4, 6}, {2, 0, 1, 1, 0, 1}));
    ACCEPTED(members(R, {0, BIG}, {0, 1}, {0, 2}, {0, BIG - 1}));
    ACCEPTED(members(B, {0, BIG - 2, BIG}, {0, 0, 1}, {0, 2}, {0, 1}));

    REFUSED(members(R, {0, 3, 3, 5}, {0, 2, 3, 5}, {0, 2, 3, 3, 4, 6}, {2, -1, 1, 1, 0, 1}),
            "fn: region 0 of page 0 lists line -1, the page has 3 lines");
    REFUSED(members(R, {0, 3, 3, 5}, {0, 2, 3, 5}, {0, 2, 3, 3, 4, 6}, {2, 0, 3, 1, 0, 1}),     // exactly n; the group's index on its page
            "fn: region 1 of page 0 lists line 3, the page has 3 lines");
    REFUSED(members(B, {0, 3, 3, 5}, {0, 2, 3, 5}, {0, 2, 3, 3, 4, 6}, {2, 0, 1, 1, 0, 2}),     // the last entry of the last group of the last page
            "fn: ground truth block 1 of page 2 lists line 2, the page has 2 lines");
    REFUSED(members(B, {0, 3, 3, 5}, {0, 2, 3, 5}, {0, 2, 3, 4, 4, 6}, {2, 0, 1, 0, 0, 1}),     // a page without lines has no line 0
            "fn: ground truth block 0 of page 1 lists line 0, the page has 0 lines");
    REFUSED(members(R, {0, 1}, {0, 1}, {0, 1}, {1}), "fn: region 0 of page 0 lists line 1, the page has 1 lines");
    REFUSED(members(R, {0, 2, 4}, {0, 1, 2}, {0, 1, 2}, {1, 2}),                                // not an index into the concatenated lines
            "fn: region 0 of page 1 lists line 2, the page has 2 lines");
    REFUSED(members(R, {0, BIG}, {0, 1}, {0, 2}, {0, BIG}), "fn: region 0 of page 0 lists line 2147483647, the page has 2147483647 lines");
    REFUSED(members(R, {0, BIG}, {0, 1}, {0, 1}, {INT32_MIN}), "fn: region 0 of page 0 lists line -2147483648, the page has 2147483647 lines");
}

}  // namespace

int main() {
    check_offset_tables();
    check_member_tables();
    std::printf("batch tables ok: %d cases\n", g_cases);
    return 0;
}
