// The arithmetic of the ARU engine's layer launchers, in one place and in plain C++17: no HIP, no device types, nothing of the engine, so that a
// host program can check it (tests/launch_plan_check.cpp).
//
// A launch covers one layer of at most MAXP problems (pages x scales); a longer list is cut into chunks.  The work units of a launch are the
// problems' unit lists one behind the other: problem i's units start at its `begin` (tile_begin / blk_begin / begin of the kernels' *Prob structs).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace asep {

constexpr int MAXP = 12;                  // problems of one launch: the p[] of every *Args struct

// the end points of page b of a grouped backbone forward are "<page_prefix(b)><name>": the ARU engine names them, the relation net looks them up
inline std::string page_prefix(int b) { return b ? "p" + std::to_string(b) + "/" : std::string(); }

// ---- the cut of n problems into launches: chunk c = problems [chunk_begin(c), chunk_end(n, c)) ----
inline size_t num_chunks(size_t n) { return (n + MAXP - 1) / MAXP; }
inline size_t chunk_begin(size_t c) { return c * MAXP; }
inline size_t chunk_end(size_t n, size_t c) { return std::min(n, (c + 1) * (size_t)MAXP); }

// ---- numbering of a launch's work units: next_*() is called for the problems of a launch in order, total = the units so far ----
struct Units { int per_row, begin; };     // 2-D: tiles_x and tile_begin; strips: strips and begin; 1-D: per_row is 0
struct UnitCounter {
    int total = 0;
    // tiles of tw x th pixels over an H x W problem, row by row: tile (x, y) is unit begin + y * per_row + x
    Units next_tiles(int H, int W, int tw, int th) {
        const Units u{(W + tw - 1) / tw, total};
        total += u.per_row * ((H + th - 1) / th);
        return u;
    }
    // blocks of `per_block` items over `items` items (the last block is partial when per_block does not divide items)
    Units next_blocks(size_t items, size_t per_block) {
        const Units u{0, total};
        total += (int)((items + per_block - 1) / per_block);
        return u;
    }
    // convr_kernel: strips of `sw` columns, a unit = one row of one strip
    Units next_strips(int H, int W, int sw) {
        const Units u{(W + sw - 1) / sw, total};
        total += u.per_row * H;
        return u;
    }
};

// ---- one-shot kernels (one block per unit): XCD bands from a few waves of blocks per XCD on.  chunk = ceil(total / 8) and the grid is padded to
//      8 * chunk blocks (block b = unit (b & 7) * chunk + (b >> 3); blocks beyond the last unit leave at once), or chunk = 0: identity order ----
struct OneshotPlan { int chunk, units; };
inline OneshotPlan oneshot_plan(int total, bool use_xcd_sched) {
    if (!use_xcd_sched || total < 8 * 64) return {0, total};
    const int chunk = (total + 7) / 8;
    return {chunk, 8 * chunk};
}

// ---- persistent kernels (resident blocks walk the units with a grid stride): work unit -> tile table for the problems' tile grids (tile numbers
//      begin + y * tx + x, `total` tiles in all): the tiles of every problem in 4 x 8 super-tile order (groups of 4 rows x 8 columns, the groups
//      walked down a column of groups first), the list cut into eight chunks, unit k = the (k / 8)-th tile of chunk k mod 8 (block b runs on XCD
//      b mod 8).  Empty when the grids do not add up to `total`: no schedule ----
struct TileDims { int tx, ty, begin; };
inline std::vector<int32_t> xcd_order(const std::vector<TileDims>& probs, int total) {
    std::vector<int32_t> order;
    order.reserve(total);
    for (const TileDims& q : probs)
        for (int gc = 0; gc * 8 < q.tx; ++gc)
            for (int gr = 0; gr * 4 < q.ty; ++gr)
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 8; ++c) {
                        const int ty = gr * 4 + r, tx = gc * 8 + c;
                        if (ty < q.ty && tx < q.tx) order.push_back(q.begin + ty * q.tx + tx);
                    }
    if ((int)order.size() != total) return {};
    std::vector<int32_t> sched(total);
    int off[9];
    off[0] = 0;
    for (int x = 0; x < 8; ++x) off[x + 1] = off[x] + (total - x + 7) / 8;
    for (int k = 0; k < total; ++k) sched[k] = order[off[k % 8] + k / 8];
    return sched;
}

// ---- page tables of the relation net's batched visual stages (gnn_engine.hip: one launch over the pages of a call, whatever their sizes).
//      The units of a launch (blocks of 256 outputs, or one block per region) are the pages' unit lists one behind the other: page b owns the
//      units begin[b] .. begin[b + 1] - 1, begin[n_pages] is the grid.  A page may own no unit (an empty map, a page without interactions) ----

// TensorFlow's SAME rule along one axis for a 3-tap filter: output size and the padding in front (the smaller half)
inline void same_pad3(int n, int stride, int* out, int* before) {
    *out = (n + stride - 1) / stride;
    *before = std::max((*out - 1) * stride + 3 - n, 0) / 2;
}

// what the 3x3 convolution of a generated feature map (stride 1 or 2) makes of an ih x iw map
struct FmapDims { int ih, iw, oh, ow, pad_t, pad_l; };
inline FmapDims fmap_dims(int ih, int iw, int stride) {
    FmapDims d{ih, iw, 0, 0, 0, 0};
    same_pad3(ih, stride, &d.oh, &d.pad_t);
    same_pad3(iw, stride, &d.ow, &d.pad_l);
    return d;
}

// The maps of one page's layout (feature_map_generators.py:140-194).  Map i is a backbone end point (depth < 0) or generated with two
// convolutions: a 1x1 to depth / 2 channels, then a 3x3 of stride 1 (reads its own end point) or 2 (reads map i - 1) to depth channels.
struct FmapSpec { int depth, stride, Cin; };          // Cin: the channels the 1x1 filter was loaded for
struct FmapShape { int fh, fw, C, bf; };              // bf: bf16 elements (an end point of a bf16 backbone); generated maps are fp32
struct FmapStep {
    bool generated, bad_channels;   // bad_channels: what a generated map reads is not Cin wide / an end point is not want_C[i] wide
    int src;                        // what a generated map reads: -1 = its own end point, else map `src`
    FmapShape in, out;              // what the 1x1 reads (generated maps only), and the map itself
    FmapDims d;                     // the 3x3's geometry
    size_t n1, n2;                  // outputs of the 1x1 and of the 3x3
    // the profiler's figures per launch: flops; algorithmic bytes of this page (the input once, the output once); the filter and bias (once per launch)
    double fl1, io1, w1, fl3, io3, w3;
};
// ends[i]: the end point of map i where one is read (depth < 0 or stride 1); want_C[i]: the channels map i was attached with
inline std::vector<FmapStep> fmap_plan(const FmapSpec* spec, const FmapShape* ends, const int* want_C, int n) {
    std::vector<FmapStep> plan((size_t)n, FmapStep{});
    for (int i = 0; i < n; ++i) {
        FmapStep& k = plan[(size_t)i];
        const FmapSpec& G = spec[i];
        k.src = -1;
        if (G.depth < 0) {
            k.out = ends[i];
            k.bad_channels = k.out.C != want_C[i];
            continue;
        }
        k.generated = true;
        if (G.stride != 1) k.src = i - 1;
        k.in = k.src < 0 ? ends[i] : plan[(size_t)k.src].out;
        k.bad_channels = k.in.C != G.Cin;
        const int half = G.depth / 2;
        k.d = fmap_dims(k.in.fh, k.in.fw, G.stride);
        k.out = FmapShape{k.d.oh, k.d.ow, G.depth, 0};
        k.n1 = (size_t)k.in.fh * k.in.fw * half;
        k.n2 = (size_t)k.d.oh * k.d.ow * G.depth;
        k.fl1 = 2.0 * (double)k.n1 * k.in.C;
        k.io1 = (double)k.in.fh * k.in.fw * k.in.C * (k.in.bf ? 2 : 4) + 4.0 * (double)k.n1;
        k.w1 = 4.0 * ((double)k.in.C * half + half);
        k.fl3 = 2.0 * (double)k.n2 * 9 * half;
        k.io3 = 4.0 * (double)k.n1 + 4.0 * (double)k.n2;
        k.w3 = 4.0 * (9.0 * half * G.depth + G.depth);
    }
    return plan;
}

// begin[0 .. n] for pages of items[b] items in units of per_unit items (the last unit of a page is partial when per_unit does not divide its
// items).  False when the units do not fit one launch (a 31-bit grid): begin is then not to be used.
inline bool page_unit_table(const size_t* items, int n, size_t per_unit, std::vector<int32_t>& begin) {
    begin.assign((size_t)n + 1, 0);
    uint64_t total = 0;
    for (int b = 0; b < n; ++b) {
        total += ((uint64_t)items[b] + per_unit - 1) / per_unit;
        if (total > (uint64_t)INT32_MAX) return false;
        begin[(size_t)b + 1] = (int32_t)total;
    }
    return true;
}

// the page that owns `unit` (0 <= unit < begin[n]): the last b with begin[b] <= unit, which skips the pages without units.  constexpr: the
// kernels call the same function
constexpr int page_of_unit(const int32_t* begin, int n, int unit) {
    int lo = 0, hi = n;                       // begin[lo] <= unit < begin[hi] throughout: a binary search, log2(n) reads per block
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (begin[mid] <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

// one page of the batched TF1 bilinear resize (post_kernels.h prep_resize_tf1_pages_kernel): the uint8 scan [H, W, C] -> float32 [h, w(, C)];
// luma: C = 3 in, one channel out.  sy, sx as the single-page launcher forms them: a double division rounded once to float32
struct ResizePage { const uint8_t* img; float* out; int H, W, h, w; float sy, sx; int C, luma; };
inline ResizePage resize_page(const uint8_t* img, int H, int W, int C, bool luma, int h, int w, float* out) {
    return ResizePage{img, out, H, W, h, w, (float)((double)H / (double)h), (float)((double)W / (double)w), C, luma ? 1 : 0};
}

// one page of the batched per-image moments (aru_kernels.h moments_pages_kernel): n values at x; `parts` blocks leave their partial sums in
// sums [parts][2]; stats receives {mean, 1 / max(sd, 1e-4)}.  moments_parts: the block count the single-page launcher uses for n values
struct MomentsPage { const float* x; size_t n; double* sums; float* stats; int parts; };
inline int moments_parts(size_t n) { return (int)std::min<size_t>(((n + 3) / 4 + 255) / 256, 256 * 8); }

// offsets of n buffers of items[b] elements in one arena, each aligned to `align` elements; returns the arena's size in elements
inline size_t arena_offsets(const size_t* items, int n, size_t align, std::vector<size_t>& off) {
    off.assign((size_t)n, 0);
    size_t total = 0;
    for (int b = 0; b < n; ++b) {
        off[(size_t)b] = total;
        total += (items[b] + align - 1) / align * align;
    }
    return total;
}

}  // namespace asep
