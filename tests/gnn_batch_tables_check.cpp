// Host check of the page-table builders csrc/launch_plan.h gained for the relation net's batched visual stages (same_pad3, fmap_dims,
// page_unit_table, page_of_unit, arena_offsets) against brute-force restatements.  Plain C++17, no HIP: tests/test_gnn_batch_host.py builds it
// with the host compiler under the address and undefined-behaviour sanitizers.  Called as `check stride channels h0 w0 h1 w1 ...` it also prints
// the tables of those map sizes for the numpy restatement of the test.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "launch_plan.h"

using namespace asep;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// TensorFlow's SAME rule restated by enumeration instead of its closed form: the output has as many cells as there are positions 0, stride,
// 2 stride, ... below n; the windows of those cells together span `span` = last position + 3 inputs; what of it exceeds n is padding, placed so
// that the part in front is as large as it can be without exceeding the part behind: found by trying every split
static void brute_same(int n, int stride, int* out, int* before) {
    int o = 0;
    for (int pos = 0; pos < n; pos += stride) ++o;
    *out = o;
    *before = 0;
    if (o == 0) return;
    const int span = (o - 1) * stride + 3;
    int pad = 0;
    while (n + pad < span) ++pad;
    for (int front = 0; front <= pad; ++front)
        if (front <= pad - front) *before = front;
}

int main(int argc, char** argv) {
    // ---- same_pad3 / fmap_dims over every small size, strides 1 and 2 (0: a zero-area map, 1: a single pixel) ----
    for (int stride = 1; stride <= 2; ++stride)
        for (int n = 0; n <= 130; ++n) {
            int o, b, o2, b2;
            same_pad3(n, stride, &o, &b);
            brute_same(n, stride, &o2, &b2);
            CHECK(o == o2 && (o == 0 || b == b2));        // (an empty map has no window: its padding is never read)
            // every real tap of every output cell is read inside the map or skipped: the first and last window positions
            if (o > 0) CHECK(-b <= 0 && (o - 1) * stride - b < std::max(n, 1) + 2);
            const FmapDims d = fmap_dims(n, n + 3, stride);
            int ow, bl;
            brute_same(n + 3, stride, &ow, &bl);
            CHECK(d.ih == n && d.iw == n + 3 && d.oh == o && d.pad_t == b && d.ow == ow && d.pad_l == bl);
        }
    {   // the chains of the GPU test: 71 x 53 page, up_1 map 36 x 27, then two strided maps; and down to one cell and to nothing
        FmapDims d = fmap_dims(36, 27, 2);
        CHECK(d.oh == 18 && d.ow == 14 && d.pad_t == 0 && d.pad_l == 1);
        d = fmap_dims(18, 14, 2);
        CHECK(d.oh == 9 && d.ow == 7 && d.pad_t == 0 && d.pad_l == 0);
        d = fmap_dims(1, 1, 2);
        CHECK(d.oh == 1 && d.ow == 1 && d.pad_t == 1 && d.pad_l == 1);
        d = fmap_dims(0, 5, 2);
        CHECK(d.oh == 0 && d.ow == 3);
    }
    // ---- page_unit_table / page_of_unit: heap arrays of their exact length ----
    const std::vector<std::vector<size_t>> item_sets = {
        {64 * 96 * 3, 96 * 64 * 3, 71 * 53 * 3, 128 * 80 * 3}, {0, 0, 5, 0}, {1}, {0}, {256, 257, 255, 0, 512}, {2, 3, 30, 17}, {0, 0, 0}};
    for (const auto& items : item_sets)
        for (size_t per : {(size_t)256, (size_t)1}) {
            const int n = (int)items.size();
            std::unique_ptr<size_t[]> it(new size_t[n]);
            for (int b = 0; b < n; ++b) it[b] = items[b];
            std::vector<int32_t> begin;
            CHECK(page_unit_table(it.get(), n, per, begin));
            CHECK((int)begin.size() == n + 1 && begin[0] == 0);
            std::unique_ptr<int32_t[]> bg(new int32_t[n + 1]);
            for (int b = 0; b <= n; ++b) bg[b] = begin[b];
            int unit = 0;
            for (int b = 0; b < n; ++b) {
                const int units = (int)((items[b] + per - 1) / per);
                CHECK(begin[b + 1] - begin[b] == units);
                for (int k = 0; k < units; ++k, ++unit) {
                    const int pg = page_of_unit(bg.get(), n, unit);
                    CHECK(pg == b);
                    // the items this unit covers lie inside the page
                    CHECK((size_t)(unit - bg[pg]) * per < items[b]);
                }
            }
            CHECK(unit == begin[n]);
        }
    {   // more units than a 31-bit grid: refused
        const size_t big[2] = {(size_t)1 << 40, (size_t)1 << 40};
        std::vector<int32_t> begin;
        CHECK(!page_unit_table(big, 2, 256, begin));
        const size_t edge[1] = {(size_t)INT32_MAX * 256};
        CHECK(page_unit_table(edge, 1, 256, begin) && begin[1] == INT32_MAX);
    }
    // ---- arena_offsets: aligned, disjoint, in order ----
    for (const auto& items : item_sets) {
        std::vector<size_t> off;
        const size_t total = arena_offsets(items.data(), (int)items.size(), 64, off);
        size_t end = 0;
        for (size_t b = 0; b < items.size(); ++b) {
            CHECK(off[b] % 64 == 0 && off[b] >= end);
            end = off[b] + items[b];
        }
        CHECK(total >= end && total % 64 == 0);
    }
    // ---- the tables of the sizes on the command line, for the numpy restatement ----
    if (argc > 2) {
        const int stride = std::atoi(argv[1]), co = std::atoi(argv[2]);
        const int n = (argc - 3) / 2;
        std::vector<size_t> items(n);
        for (int b = 0; b < n; ++b) {
            const FmapDims d = fmap_dims(std::atoi(argv[3 + 2 * b]), std::atoi(argv[4 + 2 * b]), stride);
            items[b] = (size_t)d.oh * d.ow * co;
            std::printf("dims %d %d %d %d %d %d\n", d.ih, d.iw, d.oh, d.ow, d.pad_t, d.pad_l);
        }
        std::vector<int32_t> begin;
        CHECK(page_unit_table(items.data(), n, 256, begin));
        std::printf("begin");
        for (int32_t v : begin) std::printf(" %d", v);
        std::printf("\npage_of");
        for (int u = 0; u < begin[n]; ++u) std::printf(" %d", page_of_unit(begin.data(), n, u));
        std::printf("\n");
    }
    if (failures) return 1;
    std::printf("gnn batch tables ok\n");
    return 0;
}
