// Host check of pack_first_rgb (csrc/aru_pack.h; no GPU, no HIP): the [3,3,3,cout] first filter of a colour net as conv_c3_kernel reads it
// (TensorFlow's order, rounded to bfloat16 for the bf16 engine; every other shape refused).  Packs generated filters into heap vectors of their exact length (the sanitizers this is built with see a slot computed past the
// end) and prints "P <case> <count> <hex bits of every packed float>" per accepted case and "R <case> <code> <error text>" per refused one;
// tests/test_rgb_host.py builds the same filters with numpy and compares.  Filter element i = (i + 1) * 1.001f, bias element i = i.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "aru_pack.h"

namespace asep {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace asep
using namespace asep;

static HostTensor filled(std::vector<int> dims, float scale) {
    HostTensor t;
    t.dims = dims;
    t.data.resize(t.count());
    for (size_t i = 0; i < t.data.size(); ++i) t.data[i] = (float)(i + 1) * scale;
    return t;
}

static void run(const char* name, std::vector<int> dims, int nbias, bool bf16) {
    const HostTensor w = filled(dims, 1.001f), b = filled({nbias}, 1.0f);
    const Layer L{w, b};
    g_err[0] = 0;
    try {
        const std::vector<float> pk = pack_first_rgb("t/conv1", L, bf16);
        printf("P %s %zu", name, pk.size());
        for (float v : pk) {
            uint32_t u;
            memcpy(&u, &v, 4);
            printf(" %08x", u);
        }
        printf("\n");
    } catch (const PackRefusal& r) {
        printf("R %s %d %s\n", name, r.code, g_err);
    }
}

int main() {
    run("c8", {3, 3, 3, 8}, 8, false);
    run("c16", {3, 3, 3, 16}, 16, false);
    run("c8_bf16", {3, 3, 3, 8}, 8, true);
    run("c16_bf16", {3, 3, 3, 16}, 16, true);
    run("gray", {3, 3, 1, 8}, 8, false);                     // the 1-channel filter is not this function's
    run("four_channels", {3, 3, 4, 8}, 8, false);
    run("cout12", {3, 3, 3, 12}, 12, false);
    run("k4", {4, 4, 3, 8}, 8, false);
    run("rank3", {3, 3, 24}, 8, false);
    run("bias", {3, 3, 3, 8}, 7, false);
    printf("aru pack rgb ok\n");
    return 0;
}
