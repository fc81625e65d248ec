// Host check of csrc/launch_plan.h against brute-force restatements: the cut of a problem list into launches, the 2-D tile / 1-D block / strip
// numbering of a launch's work units, the padding rule of the one-shot kernels and the XCD order of the persistent ones.
// Stand-alone: built and run by tests/test_launch_plan_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "launch_plan.h"

using namespace asep;

namespace {

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

// the tile shapes (columns x rows) the engine's launchers number with
struct Shape { int tw, th; };
const Shape SHAPES[] = {
    {64, 4},     // first layers (conv_c1_kernel / conv_c3_kernel)
    {32, 8},     // CONV_TW x CONV_TH (aru_kernels.h); also the split-product and bf16 conv tiles
    {32, 16},    // the big-tile convs, RB_TW x RB_TH, the bf16 level-0 tile kernels
    {16, 16},    // C1O_T x C1O_T (res8v_kernels.h); also DCV_T
    {32, 4},     // WINO_TW x WINO_TH (aru_kernels.h)
    {32, 8},     // WINO_TW x 2 * WINO_TH: the register-resident Winograd variant for one m-tile
    {58, 64},    // R8_OW x R8_OH * R8_NP (res8_kernels.h)
};

void check_chunks() {
    CHECK(MAXP == 12);
    for (size_t n : {0, 1, 11, 12, 13, 24, 25}) {
        size_t next = 0;
        for (size_t c = 0; c < num_chunks(n); ++c) {
            const size_t b0 = chunk_begin(c), b1 = chunk_end(n, c);
            CHECK(b0 == next && b1 > b0 && b1 - b0 <= (size_t)MAXP && b1 <= n);
            next = b1;
        }
        CHECK(next == n);
        CHECK(num_chunks(n) == (n + 11) / 12);
    }
}

// problems (H, W) of one launch on tiles of shape s: tile_begin is the running sum, every pixel falls into exactly one tile < total
struct Dim { int H, W; };
void check_tiles(const std::vector<Dim>& probs, Shape s) {
    UnitCounter uc;
    std::vector<Units> u;
    int sum = 0;
    for (const Dim& d : probs) {
        u.push_back(uc.next_tiles(d.H, d.W, s.tw, s.th));
        CHECK(u.back().begin == sum);
        int tx = 0, ty = 0;
        while (tx * s.tw < d.W) ++tx;
        while (ty * s.th < d.H) ++ty;
        CHECK(u.back().per_row == tx);
        sum += tx * ty;
        CHECK(uc.total == sum);
    }
    std::vector<int> hits(uc.total, 0);
    for (size_t i = 0; i < probs.size(); ++i)
        for (int y = 0; y < probs[i].H; ++y)
            for (int x = 0; x < probs[i].W; ++x) {
                // the tiles that contain pixel (x, y): searched, not computed
                int found = 0, tile = -1;
                const int rows = (probs[i].H + s.th - 1) / s.th;
                for (int ty = std::max(0, y / s.th - 1); ty < std::min(rows, y / s.th + 2); ++ty)
                    for (int tx = std::max(0, x / s.tw - 1); tx < std::min(u[i].per_row, x / s.tw + 2); ++tx)
                        if (tx * s.tw <= x && x < (tx + 1) * s.tw && ty * s.th <= y && y < (ty + 1) * s.th) { ++found; tile = u[i].begin + ty * u[i].per_row + tx; }
                CHECK(found == 1 && tile >= 0 && tile < uc.total);
                CHECK(i + 1 == probs.size() || tile < u[i + 1].begin);        // inside its own problem's range
                ++hits[tile];
            }
    for (int t = 0; t < uc.total; ++t) CHECK(hits[t] >= 1 && hits[t] <= s.tw * s.th);      // no empty tile
}

void check_tile_numbering() {
    for (const Shape& s : SHAPES) {
        for (int H = 1; H <= 70; ++H)
            for (int W = 1; W <= 70; ++W) check_tiles({{H, W}}, s);
        // lists of 12 and 13 mixed problems (13: as one numbering, the walker never builds it -- the rule itself has no limit)
        std::vector<Dim> mixed;
        unsigned r = 12345;
        for (int i = 0; i < 13; ++i) {
            r = r * 1664525u + 1013904223u;
            mixed.push_back({1 + (int)((r >> 8) % 70), 1 + (int)((r >> 16) % 70)});
        }
        check_tiles(std::vector<Dim>(mixed.begin(), mixed.begin() + 12), s);
        check_tiles(mixed, s);
    }
}

void check_blocks() {
    for (size_t per : {256, 1024, 4096}) {
        UnitCounter uc;
        const size_t items[] = {1, per - 1, per, per + 1, 3 * per, 3 * per + 7, 5};
        int sum = 0;
        for (size_t n : items) {
            const Units u = uc.next_blocks(n, per);
            CHECK(u.begin == sum);
            const int blocks = uc.total - u.begin;
            // the block ranges [b * per, min((b + 1) * per, n)) tile the items; the last one is partial when per does not divide n
            size_t covered = 0;
            for (int b = 0; b < blocks; ++b) {
                const size_t lo = (size_t)b * per, hi = std::min(lo + per, n);
                CHECK(lo == covered && hi > lo);
                covered = hi;
            }
            CHECK(covered == n);
            CHECK((n % per != 0) == (n - (size_t)(blocks - 1) * per < per));
            sum += blocks;
        }
    }
    // convr_kernel's strips: a unit = one row of one 32-column strip
    UnitCounter uc;
    int sum = 0;
    for (Dim d : {Dim{1, 1}, Dim{21, 34}, Dim{41, 68}, Dim{7, 32}, Dim{9, 33}}) {
        const Units u = uc.next_strips(d.H, d.W, 32);
        CHECK(u.begin == sum && u.per_row == (d.W + 31) / 32 && u.per_row * 32 >= d.W && (u.per_row - 1) * 32 < d.W);
        sum += u.per_row * d.H;
        CHECK(uc.total == sum);
    }
}

// the kernels' rule, sched_tile() (csrc/aru_kernels.h:74): block b of a padded grid -> unit (b & 7) * chunk + (b >> 3), or none when that is >= total
int sched_tile(int chunk, int total, int b) {
    if (chunk) {
        const int t = (b & 7) * chunk + (b >> 3);
        return t < total ? t : -1;
    }
    return b;
}

void check_oneshot() {
    for (int total = 1; total < 8 * 64; ++total) {
        const OneshotPlan p = oneshot_plan(total, true);
        CHECK(p.chunk == 0 && p.units == total);             // identity below 512 units
    }
    for (int total : {512, 513, 519, 520, 521, 1000, 4095, 4096, 4097, 100003}) {
        CHECK(oneshot_plan(total, false).chunk == 0 && oneshot_plan(total, false).units == total);
        const OneshotPlan p = oneshot_plan(total, true);
        CHECK(p.chunk > 0 && 8 * p.chunk >= total && 8 * (p.chunk - 1) < total && p.units == 8 * p.chunk);
        std::vector<int> hits(total, 0);
        for (int b = 0; b < p.units; ++b) {
            const int t = sched_tile(p.chunk, total, b);
            CHECK(t >= -1 && t < total);
            if (t >= 0) ++hits[t];
        }
        for (int t = 0; t < total; ++t) CHECK(hits[t] == 1);
    }
}

void check_xcd_order() {
    const std::vector<std::vector<TileDims>> lists = {{{1, 1, 0}}, {{13, 9, 0}}, {{8, 4, 0}}, {{7, 70, 0}, {33, 5, 490}, {1, 3, 655}}};
    for (const std::vector<TileDims>& probs : lists) {
        int total = 0;
        for (const TileDims& q : probs) { CHECK(q.begin == total); total += q.tx * q.ty; }
        const std::vector<int32_t> sched = xcd_order(probs, total);
        CHECK((int)sched.size() == total);
        std::vector<int> hits(total, 0);
        for (int32_t t : sched) { CHECK(t >= 0 && t < total); ++hits[t]; }
        for (int t = 0; t < total; ++t) CHECK(hits[t] == 1);
        // grids that do not add up to the total: no schedule
        CHECK(xcd_order(probs, total + 1).empty());
        CHECK(xcd_order(probs, total - 1).empty() || total == 1);
    }
    // an XCD's consecutive units are neighbours of one super tile: the first 32 units of XCD 0 in a grid of one full group per XCD chunk
    const std::vector<int32_t> s = xcd_order({{8, 32, 0}}, 256);
    for (int k = 0; k < 32; ++k) CHECK(s[8 * k] == (k / 8) * 8 + k % 8);
}

// the one spelling of a page's end-point prefix that both engines use: page 0 has none
void check_page_prefix() {
    CHECK(page_prefix(0) == "");
    CHECK(page_prefix(1) == "p1/");
    CHECK(page_prefix(12) == "p12/");
}

}  // namespace

int main() {
    check_page_prefix();
    check_chunks();
    check_tile_numbering();
    check_blocks();
    check_oneshot();
    check_xcd_order();
    std::printf("launch plan ok: chunks, %d tile shapes on pages up to 70 x 70, block ranges, one-shot map, XCD order\n", (int)(sizeof(SHAPES) / sizeof(SHAPES[0])));
    return 0;
}
