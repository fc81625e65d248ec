// Host check of the page-table builders csrc/launch_plan.h gained for the relation net's batched visual stages (same_pad3, fmap_dims,
// fmap_plan, page_unit_table, page_of_unit, arena_offsets) against brute-force restatements.  Plain C++17, no HIP: tests/test_gnn_batch_host.py builds it
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
    // ---- fmap_plan: one page's maps for the layout [end point, depth 8 stride 1, depth 6 stride 2, depth 2 stride 2] over end points of four
    //      sizes, fp32 and bf16, against fmap_dims and the products; heap arrays of their exact length ----
    {
        const int n = 4, C = 5;                                      // the end points' channels
        const FmapSpec layout[n] = {{-1, 1, 0}, {8, 1, C}, {6, 2, 8}, {2, 2, 6}};
        const int want_src[n] = {-1, -1, 1, 2};
        const int sizes[4][2] = {{1, 1}, {1, 5}, {5, 4}, {36, 27}};
        for (const auto& hw : sizes)
            for (int bf = 0; bf <= 1; ++bf)
                for (int wrong = -1; wrong < n; ++wrong) {           // -1: every filter fits; else map `wrong` was loaded for (or attached with) one channel more
                    std::unique_ptr<FmapSpec[]> spec(new FmapSpec[n]);
                    std::unique_ptr<FmapShape[]> ends(new FmapShape[n]);
                    std::unique_ptr<int[]> want_C(new int[n]);
                    for (int i = 0; i < n; ++i) {
                        spec[i] = layout[i];
                        ends[i] = i < 2 ? FmapShape{hw[0], hw[1], C, bf} : FmapShape{-7, -7, -7, -7};   // (maps 2 and 3 read no end point)
                        want_C[i] = layout[i].depth < 0 ? C : layout[i].depth;
                    }
                    if (wrong == 0) ++want_C[0];
                    else if (wrong > 0) ++spec[wrong].Cin;
                    const std::vector<FmapStep> plan = fmap_plan(spec.get(), ends.get(), want_C.get(), n);
                    CHECK((int)plan.size() == n);
                    CHECK(!plan[0].generated && plan[0].out.fh == hw[0] && plan[0].out.fw == hw[1] && plan[0].out.C == C && plan[0].out.bf == bf);
                    for (int i = 0; i < n; ++i) CHECK(plan[i].bad_channels == (i == wrong));
                    FmapShape in{hw[0], hw[1], C, bf};                // what map 1 reads; then each map's output
                    for (int i = 1; i < n; ++i) {
                        const FmapStep& k = plan[i];
                        const int depth = layout[i].depth, half = depth / 2;
                        const FmapDims d = fmap_dims(in.fh, in.fw, layout[i].stride);
                        CHECK(k.generated && k.src == want_src[i]);
                        CHECK(k.in.fh == in.fh && k.in.fw == in.fw && k.in.C == in.C && k.in.bf == in.bf);
                        CHECK(k.d.ih == d.ih && k.d.iw == d.iw && k.d.oh == d.oh && k.d.ow == d.ow && k.d.pad_t == d.pad_t && k.d.pad_l == d.pad_l);
                        CHECK(k.n1 == (size_t)in.fh * in.fw * half && k.n2 == (size_t)d.oh * d.ow * depth);
                        CHECK(k.out.fh == d.oh && k.out.fw == d.ow && k.out.C == depth && k.out.bf == 0);
                        CHECK(k.fl1 == 2.0 * k.n1 * in.C && k.fl3 == 2.0 * k.n2 * 9 * half);
                        CHECK(k.io1 == (double)in.fh * in.fw * in.C * (in.bf ? 2 : 4) + 4.0 * k.n1 && k.io3 == 4.0 * k.n1 + 4.0 * k.n2);
                        CHECK(k.w1 == 4.0 * (in.C * half + half) && k.w3 == 4.0 * (9 * half * depth + depth));
                        in = k.out;
                    }
                }
        {   // the 36 x 27 end point's chain, spelled out: 36 x 27 x 8, 18 x 14 x 6, 9 x 7 x 2
            const FmapShape ends[n] = {{36, 27, C, 1}, {36, 27, C, 1}, {}, {}};
            const int want_C[n] = {C, 8, 6, 2};
            const std::vector<FmapStep> plan = fmap_plan(layout, ends, want_C, n);
            CHECK(plan[1].out.fh == 36 && plan[1].out.fw == 27 && plan[1].d.pad_t == 1 && plan[1].d.pad_l == 1 && plan[1].n1 == 36 * 27 * 4 && plan[1].n2 == 36 * 27 * 8);
            CHECK(plan[2].out.fh == 18 && plan[2].out.fw == 14 && plan[2].d.pad_t == 0 && plan[2].d.pad_l == 1 && plan[2].n1 == 36 * 27 * 3 && plan[2].n2 == 18 * 14 * 6);
            CHECK(plan[3].out.fh == 9 && plan[3].out.fw == 7 && plan[3].n1 == 18 * 14 * 1 && plan[3].n2 == 9 * 7 * 2);
            CHECK(plan[1].in.bf == 1 && plan[2].in.bf == 0 && plan[3].in.bf == 0);      // only the end point is bf16
        }
        {   // the default layout (every depth -1): no generated entry, every map its end point
            const FmapSpec all_ends[3] = {{-1, 1, 0}, {-1, 1, 0}, {-1, 1, 0}};
            const FmapShape ends[3] = {{5, 4, 16, 0}, {3, 2, 32, 0}, {1, 1, 64, 0}};
            const int want_C[3] = {16, 32, 64};
            const std::vector<FmapStep> plan = fmap_plan(all_ends, ends, want_C, 3);
            for (int i = 0; i < 3; ++i)
                CHECK(!plan[i].generated && !plan[i].bad_channels && plan[i].src == -1 && plan[i].n1 == 0 && plan[i].n2 == 0 && plan[i].out.fh == ends[i].fh &&
                      plan[i].out.fw == ends[i].fw && plan[i].out.C == ends[i].C);
            CHECK(fmap_plan(all_ends, ends, want_C, 0).empty());
        }
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
