// Host check of csrc/level0_plan.h: the walker region, the f32s frame units and the bf16 border tiles of a page cover every output pixel, and
// the band rule yields items that cover the region's rows.  Stand-alone: built and run by tests/test_level0_plan_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "level0_plan.h"

using namespace asep;

namespace {

constexpr int UNIT_W = 58, UNIT_H = 64;     // the res8v work unit (R8_OW x R8_OH * R8_NP of res8_kernels.h)
int g_H = 0, g_W = 0;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "%s:%d: page %d x %d: %s\n", __FILE__, __LINE__, g_H, g_W, #cond);   \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

int floordiv(int a, int b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }       // Python's //

// adds 1 to the pixels of [x0, x1) x [y0, y1); the rectangle must lie inside the page
void paint(std::vector<unsigned char>& px, int x0, int y0, int x1, int y1) {
    CHECK(0 <= x0 && x0 <= x1 && x1 <= g_W && 0 <= y0 && y0 <= y1 && y1 <= g_H);
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) ++px[(size_t)y * g_W + x];
}

void check_f32s(const WalkRegion& r, std::vector<unsigned char>& px) {
    const int H = g_H, W = g_W;
    const int tx = (W + UNIT_W - 1) / UNIT_W, ty = (H + UNIT_H - 1) / UNIT_H, begin = 7;
    std::vector<int32_t> all, units;
    frame_units(H, W, tx, begin, false, UNIT_W, UNIT_H, &all);                   // a page that does not walk lists all its units, in order
    CHECK((int)all.size() == tx * ty);
    for (int i = 0; i < tx * ty; ++i) CHECK(all[i] == begin + i);
    if (!r.fits) return;
    units.push_back(-1);                                                          // (the list is appended to)
    frame_units(H, W, tx, begin, true, UNIT_W, UNIT_H, &units);
    CHECK(units[0] == -1);
    px.assign((size_t)H * W, 0);
    for (size_t i = 1; i < units.size(); ++i) {
        const int u = units[i] - begin;
        CHECK(u >= 0 && u < tx * ty);
        CHECK(i == 1 || units[i] > units[i - 1]);                                 // unique and ascending
        const int x0 = (u % tx) * UNIT_W, y0 = (u / tx) * UNIT_H, x1 = std::min(x0 + UNIT_W, W), y1 = std::min(y0 + UNIT_H, H);
        CHECK(!(x0 >= R8W_X0 && x1 <= r.xr && y0 >= R8W_Y0 && y1 <= r.y_end));    // not wholly inside the walker's rectangle
        paint(px, x0, y0, x1, y1);
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const bool walker = x >= R8W_X0 && x < r.xr && y >= R8W_Y0 && y < r.y_end;
            CHECK(walker || px[(size_t)y * W + x] == 1);
        }
}

void check_bf16(const WalkRegion& r, std::vector<unsigned char>& px) {
    const int H = g_H, W = g_W;
    const BorderPlan bp = border_plan(H, W);
    CHECK(bp.y_end == r.y_end && bp.xr == r.xr && bp.xr == R8W_X0 + R8W_TW * r.n_strips);
    CHECK(H - r.y_end <= 16 && H - r.y_end >= 4 && W - r.xr <= 32 && W - r.xr >= 4);     // one tile each, and the walker's window margin
    CHECK(r.xr % 2 == 0 && R8W_X0 % 2 == 0 && R8W_Y0 % 2 == 0 && r.y_end % 2 == 0);      // no 2 x 2 pool cell straddles the walker's edge
    CHECK(bp.tiles() == 2 * bp.nbx + 2 * bp.nby);
    px.assign((size_t)H * W, 0);
    paint(px, R8W_X0, R8W_Y0, r.xr, r.y_end);
    for (int t = 0; t < bp.tiles(); ++t) {
        const BorderRect b = bp.rect(t);
        CHECK(b.x0 < b.x1 && b.y0 < b.y1 && b.x1 - b.x0 <= 32 && b.y1 - b.y0 <= 16 && b.x0 % 2 == 0 && b.y0 % 2 == 0);
        paint(px, b.x0, b.y0, b.x1, b.y1);
    }
    for (size_t i = 0; i < px.size(); ++i) CHECK(px[i] == 1);
}

void check_bands(const WalkRegion& r) {
    const long page_rows = (long)r.n_strips * r.rows();
    for (int waves : {4, 8})
        for (int cus : {1, 8, 64, 256, 304})
            for (int pages : {1, 4, 12}) {
                const int band = walk_band(page_rows * pages, cus, waves);
                CHECK(band % 2 == 0 && band >= 32 && band <= 256);
                const int nb = r.bands(band);
                CHECK(r.items(band) == r.n_strips * nb);
                CHECK(nb * band >= r.rows());                 // the items cover the region's rows
                CHECK((nb - 1) * band < r.rows());            // and the last one is not empty
            }
}

void check_page(int H, int W, std::vector<unsigned char>& px) {
    g_H = H; g_W = W;
    const WalkRegion r = walk_region(H, W);
    CHECK(r.fits == (floordiv(W - 36, 24) >= 4 && H - 20 >= 32));
    check_f32s(r, px);
    if (!r.fits) return;
    CHECK(r.n_strips >= 4 && r.rows() >= 32 && r.rows() % 2 == 0);
    check_bf16(r, px);
    check_bands(r);
}

}  // namespace

int main() {
    std::vector<unsigned char> px;
    int pages = 0, walking = 0;
    for (int H = 1; H <= 140; ++H)
        for (int W = 1; W <= 200; ++W) { check_page(H, W, px); ++pages; walking += walk_region(H, W).fits; }
    const int sizes[][2] = {{160, 132}, {140, 131}, {750, 1125}, {1500, 2250}, {3000, 4500}, {4500, 3000}};
    for (const auto& s : sizes) { check_page(s[0], s[1], px); ++pages; walking += walk_region(s[0], s[1]).fits; }
    // the thresholds themselves
    g_H = g_W = 0;
    CHECK(walk_region(52, 132).fits && !walk_region(51, 132).fits && !walk_region(52, 131).fits);
    CHECK(walk_region(160, 132).fits && !walk_region(140, 131).fits);
    // 32-bit offsets: no page of 2^28 pixels or more walks, whatever its shape
    CHECK(walk_region(16384, 16383).fits && !walk_region(16384, 16384).fits);
    CHECK(walk_region(65535, 4096).fits && !walk_region(65536, 4096).fits && !walk_region(4096, 65536).fits);
    CHECK(walk_region(1 << 20, 255).fits && !walk_region(1 << 20, 256).fits);
    CHECK(!walk_region(100000, 100000).fits && !walk_region(2000000, 2000).fits);
    std::printf("level0 plan ok: %d page sizes, %d of them walk\n", pages, walking);
    return 0;
}
