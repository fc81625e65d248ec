// The page geometry of the level-0 strip walkers (res8w_kernel: bf16, res8ws_kernel: f32s), in one place and in plain C++17: no HIP, no device
// types, nothing of the engine, so that a host program can check it (tests/level0_plan_check.cpp).
//
// A walker covers columns [R8W_X0, xr) x rows [R8W_Y0, y_end) of an H x W page: n_strips strips of R8W_TW columns, cut into bands of `band`
// rows; an item = one band of one strip = one wave.  Its 4-pixel window margins lie inside the image.  The frame around that rectangle is
// computed by other kernels:
//   f32s: the vector-ALU block kernels (res8v_*_kernel) over the work units that are not wholly inside the rectangle (frame_units);
//   bf16: res8wb_kernel over 16 x 32 border tiles: a full-width row above and below, a column left and right (BorderPlan).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace asep {

constexpr int R8W_TW = 24;                // output columns of a strip
constexpr int R8W_X0 = 32, R8W_Y0 = 16;   // the walker's region starts here (one border tile column / row in front of it)

struct WalkRegion {
    int n_strips;          // strips at x0 = R8W_X0 + R8W_TW s
    int y_end;             // the walker's rows end here (even, <= H - 4)
    int xr;                // first column behind the strips
    bool fits;             // room for four strips and two 16-row bands, and 32-bit element offsets (< 2^28 pixels); the rest is meaningless without it
    int rows() const { return y_end - R8W_Y0; }
    double pixels() const { return (double)n_strips * R8W_TW * rows(); }
    int bands(int band) const { return (rows() + band - 1) / band; }
    int items(int band) const { return n_strips * bands(band); }       // band-major, the strips of a band side by side
};
inline WalkRegion walk_region(int H, int W) {
    WalkRegion r;
    r.n_strips = (W - 4 - R8W_X0) / R8W_TW;
    r.y_end = R8W_Y0 + 2 * ((H - 4 - R8W_Y0) / 2);
    r.xr = R8W_X0 + R8W_TW * r.n_strips;
    r.fits = r.n_strips >= 4 && H - 4 - R8W_Y0 >= 32 && (size_t)H * W < ((size_t)1 << 28);
    return r;
}

// rows of an item of a walker launch over `strip_rows` rows in all (the sum of n_strips * rows() over its pages): ~6 items per resident wave of
// the chip, so that the hardware's block dispatch balances the tail; within 32 .. 256 and even
inline int walk_band(long strip_rows, int num_cus, int waves_per_cu) {
    const long slots = (long)waves_per_cu * num_cus;
    const int band = (int)std::min<long>(256, std::max<long>(32, strip_rows / (6 * slots)));
    return (band + 1) & ~1;
}

// f32s: appends the res8v work units of a page (unit_w columns x unit_h rows, tiles_x a row, numbered from tile_begin row by row) that the
// walker does not cover: for a page that walks the units not wholly inside the walker's rectangle, for any other page all units
inline void frame_units(int H, int W, int tiles_x, int tile_begin, bool walk, int unit_w, int unit_h, std::vector<int32_t>* units) {
    const WalkRegion r = walk_region(H, W);
    const int tiles_y = (H + unit_h - 1) / unit_h;
    for (int y = 0; y < tiles_y; ++y)
        for (int x = 0; x < tiles_x; ++x) {
            const int ux0 = x * unit_w, ux1 = std::min(ux0 + unit_w, W), uy0 = y * unit_h, uy1 = std::min(uy0 + unit_h, H);
            const bool frame = !walk || ux0 < R8W_X0 || ux1 > r.xr || uy0 < R8W_Y0 || uy1 > r.y_end;
            if (frame) units->push_back(tile_begin + y * tiles_x + x);
        }
}

// bf16: the border tiles of a page that walks, in res8wb_kernel's order (the kernel restates rect() on the device): nbx tiles of the top row,
// nbx of the bottom rows, nby of the left column, nby of the right columns.  A tile is at most 16 rows x 32 columns, so the bottom band must not
// be higher than 16 rows and the right band not wider than 32 columns.
struct BorderRect { int x0, y0, x1, y1; };       // [x0, x1) x [y0, y1)
struct BorderPlan {
    int H, W;
    int nbx;               // tiles of a full-width row: ceil(W / 32)
    int nby;               // tiles of a side column: ceil((y_end - R8W_Y0) / 16)
    int y_end, xr;
    int tiles() const { return 2 * nbx + 2 * nby; }
    BorderRect rect(int t) const {
        int x0, y0, ymax, xmax;
        if (t < nbx) { x0 = 32 * t; y0 = 0; ymax = R8W_Y0; xmax = W; }
        else if (t < 2 * nbx) { x0 = 32 * (t - nbx); y0 = y_end; ymax = H; xmax = W; }
        else if (t < 2 * nbx + nby) { x0 = 0; y0 = R8W_Y0 + 16 * (t - 2 * nbx); ymax = y_end; xmax = R8W_X0; }
        else { x0 = xr; y0 = R8W_Y0 + 16 * (t - 2 * nbx - nby); ymax = y_end; xmax = W; }
        return {x0, y0, std::min(x0 + 32, xmax), std::min(y0 + 16, ymax)};
    }
};
inline BorderPlan border_plan(int H, int W) {
    const WalkRegion r = walk_region(H, W);
    return {H, W, (W + 31) / 32, (r.rows() + 15) / 16, r.y_end, r.xr};
}

}  // namespace asep
