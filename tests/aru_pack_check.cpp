// Host check of csrc/aru_pack.h (no GPU, no HIP): packs generated filters of every shape that takes another branch of a packer and
//  1. prints, for every packed vector, "D name count fnv1a64" and, for every layer, "I name key=value ..." with the shape-derived integers;
//     tests/test_aru_pack_host.py compares the lines with tests/golden/aru_pack_digests.json, recorded from the packers before they moved;
//  2. asserts that every element of every three-part buffer sums back to its fp32 coefficient bit for bit;
//  3. asserts for the fp32 orders that every coefficient lands as often as the layout says and every other slot is zero.
// Every buffer is a heap vector of its exact length, so the sanitizers this is built with see a slot computed past the end.
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

static int g_checks = 0;
#define CHECK(cond, ...)                                                            \
    do {                                                                            \
        ++g_checks;                                                                 \
        if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } \
    } while (0)

// ---- generator + digest: 64-bit FNV-1a; an LCG (Knuth's MMIX constants) seeded with the tensor name's hash, the high 32 bits as a
// signed integer scaled by 2^-31: floats in [-1, 1) with full 24-bit mantissas
static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
static HostTensor gen(const std::string& name, std::vector<int> dims) {
    HostTensor t;
    t.dims = dims;
    t.data.resize(t.count());
    uint64_t s = fnv1a(name.data(), name.size());
    for (float& v : t.data) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        v = (float)(int32_t)(s >> 32) * (1.0f / 2147483648.0f);
    }
    return t;
}
template <class T>
static void emit(const std::string& name, const std::vector<T>& v) {
    printf("D %s %zu %016llx\n", name.c_str(), v.size(), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static void add_layer(WeightBlob& b, const std::string& scope, std::vector<int> dims, int nbias, const char* bias = "biases") {
    b[scope + "/weights"] = gen(scope + "/weights", dims);
    b[scope + "/" + bias] = gen(scope + "/" + bias, {nbias});
}

// ---- assertion 2: buf = blocks of [3 parts][blk]; the float sums h + m + l (in that order) of all slots are the coefficients of `coef`, each
// `mult` times, and zeros
static void check_exact3(const std::string& name, const std::vector<bf16_t>& buf, size_t blk, const std::vector<float>& coef, int mult) {
    CHECK(buf.size() % (3 * blk) == 0, "%s: %zu elements are no multiple of 3 x %zu", name.c_str(), buf.size(), blk);
    std::map<uint32_t, long> want, got;
    for (float c : coef) {
        CHECK(c != 0.f, "%s: the generator gave a zero coefficient", name.c_str());
        want[bits(c)] += mult;
    }
    for (size_t b0 = 0; b0 < buf.size(); b0 += 3 * blk)
        for (size_t i = 0; i < blk; ++i) {
            const float s = bfval(buf[b0 + i]) + bfval(buf[b0 + blk + i]) + bfval(buf[b0 + 2 * blk + i]);
            if (s != 0.f) ++got[bits(s)];
        }
    CHECK(got == want, "%s: the three parts do not sum to the fp32 coefficients (%zu distinct sums, %zu distinct coefficients)", name.c_str(),
          got.size(), want.size());
}

// ---- assertion 3: `pk` holds each of the values 1 .. n exactly `mult` times and zeros elsewhere
static void check_lands(const std::string& name, const std::vector<float>& pk, size_t n, int mult) {
    std::vector<int> seen(n + 1, 0);
    for (float v : pk) {
        CHECK(v >= 0.f && v <= (float)n && v == (float)(size_t)v, "%s: slot holds %g", name.c_str(), (double)v);
        ++seen[(size_t)v];
    }
    for (size_t i = 1; i <= n; ++i) CHECK(seen[i] == mult, "%s: coefficient %zu lands %d times, the layout says %d", name.c_str(), i, seen[i], mult);
    CHECK(seen[0] == (long)pk.size() - (long)n * mult, "%s: %d zero slots", name.c_str(), seen[0]);
}
static HostTensor counted(std::vector<int> dims) {
    HostTensor t;
    t.dims = dims;
    t.data.resize(t.count());
    for (size_t i = 0; i < t.data.size(); ++i) t.data[i] = (float)(i + 1);
    return t;
}

static void conv_case(const std::string& name, int k, int cin, int cout, bool deconv, bool use_c12 = true) {
    WeightBlob b;
    const std::string scope = "t/" + name;
    const char* bias = deconv ? "bias" : "biases";
    const std::vector<int> dims = deconv ? std::vector<int>{k, k, cout, cin} : std::vector<int>{k, k, cin, cout};
    add_layer(b, scope, dims, cout, bias);
    ConvPack c;
    try {
        c = pack_conv_layer(scope, find_layer(b, scope, bias), deconv, use_c12, true, true);
    } catch (const PackRefusal& r) {
        printf("I %s rc=%d\n", name.c_str(), r.code);
        return;
    }
    const ConvPlan& p = c.plan;
    printf("I %s rc=0 kh=%d kw=%d cin=%d cout=%d c8=%d c12=%d deconv=%d groups=%d mtiles=%d nchunks=%d bmode=%d bchunks=%d smode=%d\n", name.c_str(), p.kh,
           p.kw, p.cin, p.cout, (int)p.c8, (int)p.c12, (int)p.deconv, p.groups, p.mtiles, p.nchunks, p.bmode, p.bchunks, p.smode);
    emit(name + "/w", c.w); emit(name + "/b", b[scope + "/" + bias].data); emit(name + "/wino", c.wino); emit(name + "/wv", c.wv);
    emit(name + "/wb", c.wb); emit(name + "/wb8", c.wb8); emit(name + "/ws", c.ws); emit(name + "/ws16", c.ws16);
    // every coefficient once in each three-part order ([chunk][part][mtile][lane][8])
    const std::vector<float>& coef = b[scope + "/weights"].data;
    if (!c.ws.empty()) check_exact3(name + "/ws", c.ws, (size_t)p.mtiles * 512, coef, 1);
    if (!c.ws16.empty()) check_exact3(name + "/ws16", c.ws16, (size_t)p.mtiles * 512, coef, 1);
    // the fp32 A fragments (C16 / C8 / C12 chunks) and the scalar d_wv layouts: every coefficient once
    const HostTensor cw = counted(dims);
    const FilterView W(cw, deconv);
    check_lands(name + "/w", pack_mfma_a(W, p), cw.count(), 1);
    if (p.wv_deconv8() || p.wv_c1out()) check_lands(name + "/wv", pack_wv(W), cw.count(), 1);
}

static WeightBlob net_blob() {
    WeightBlob b;
    const std::string a = "aru_net/attMapG/attPart/", f = "aru_net/featMapG/";
    add_layer(b, a + "conv1", {4, 4, 1, 12}, 12);
    add_layer(b, a + "conv2", {4, 4, 12, 16}, 16);
    add_layer(b, a + "conv3", {4, 4, 16, 32}, 32);
    add_layer(b, a + "conv4", {4, 4, 32, 1}, 1);
    for (int l = 0; l < 3; ++l) {
        const int c = 8 << l;
        const std::string s = f + "unet_down_" + std::to_string(l);
        add_layer(b, s + "/conv1", {3, 3, l ? c / 2 : 1, c}, c);
        for (int r = 0; r < 3; ++r) add_layer(b, convR(s, r), {3, 3, c, c}, c);
        if (l == 2) continue;
        const std::string u = f + "unet_up_" + std::to_string(l);
        add_layer(b, u + "/deconv", {3, 3, c, 2 * c}, c, "bias");
        add_layer(b, u + "/conv1", {3, 3, 2 * c, c}, c);
        for (int r = 0; r < 3; ++r) add_layer(b, convR(u, r), {3, 3, c, c}, c);
    }
    add_layer(b, "aru_net/logit/class", {4, 4, 8, 2}, 2);
    return b;
}

// the coefficients of the three convR filters of a block, in one list
static std::vector<float> tail_coef(const WeightBlob& b, const std::string& scope) {
    std::vector<float> c;
    for (int r = 0; r < 3; ++r) append(c, b.at(convR(scope, r) + "/weights").data);
    return c;
}

static void level0_case(const std::string& name, const WeightBlob& b) {
    const Res8Pack p = pack_res8(b, true, false);
    printf("I %s/res8 rc=0\n", name.c_str());
    emit(name + "/r8_down_wr", p.down_wr); emit(name + "/r8_down_br", p.down_br); emit(name + "/r8v_down_wr", p.v_down_wr);
    emit(name + "/r8_up_w1", p.up_w1); emit(name + "/r8_up_wr", p.up_wr); emit(name + "/r8_up_br", p.up_br); emit(name + "/r8_up_b1", p.up_b1);
    emit(name + "/r8v_up_w1", p.v_up_w1); emit(name + "/r8v_up_wr", p.v_up_wr);
    const Res8wsPack s = pack_res8ws(b, true);
    printf("I %s/res8ws rc=0\n", name.c_str());
    emit(name + "/r8ws_down_w", s.down_w); emit(name + "/r8ws_up_w", s.up_w); emit(name + "/r8ws_up_w1", s.up_w1);
    // pixel-pair rows: every coefficient once per pixel parity = twice ([..][part][64][8])
    if (!s.down_w.empty()) {
        check_exact3(name + "/r8ws_down_w", s.down_w, 512, tail_coef(b, "aru_net/featMapG/unet_down_0"), 2);
        check_exact3(name + "/r8ws_up_w", s.up_w, 512, tail_coef(b, "aru_net/featMapG/unet_up_0"), 2);
        check_exact3(name + "/r8ws_up_w1", s.up_w1, 512, b.at("aru_net/featMapG/unet_up_0/conv1/weights").data, 2);
    }
    const Res8bPack q = pack_res8b(b, true);
    printf("I %s/res8b rc=0\n", name.c_str());
    emit(name + "/r8b_down_w", q.down_w); emit(name + "/r8b_down_b", q.down_b); emit(name + "/r8f_down_w1", q.f_down_w1);
    emit(name + "/r8b_down_w1r", q.down_w1r); emit(name + "/r8b_up_w", q.up_w); emit(name + "/r8b_up_b", q.up_b);
    emit(name + "/r8b_up_w1", q.up_w1); emit(name + "/r8b_up_b1", q.up_b1); emit(name + "/r8f_up_w1", q.f_up_w1);
}

static void resb_case(const std::string& name, const WeightBlob& b, int level, int C) {
    const ResbPack p = pack_resb(b, "aru_net/featMapG/unet_down_" + std::to_string(level), C);
    printf("I %s rc=0 set=%d C=%d\n", name.c_str(), (int)p.ok, p.ok ? C : 0);
    emit(name + "/w", p.w);
    emit(name + "/b", p.b);
}

// the first layers, both attention-head fragments (the bf16 one is the bf16 engine's) and the logit filters of compute_dtype `dtype`
static void load_case(const WeightBlob& b, int dtype) {
    const std::string name = "load" + std::to_string(dtype);
    const Layer det = find_direct(b, "aru_net/featMapG/unet_down_0/conv1"), att = find_direct(b, "aru_net/attMapG/attPart/conv1");
    printf("I %s det_k=%d det_cout=%d att_k=%d att_cout=%d\n", name.c_str(), det.w.dims[0], det.w.dims[3], att.w.dims[0], att.w.dims[3]);
    emit(name + "/det_first_w", det.w.data); emit(name + "/det_first_b", det.b.data);
    emit(name + "/att_first_w", att.w.data); emit(name + "/att_first_b", att.b.data);
    emit(name + "/att_head", pack_att_head(FilterView(att.w)));
    emit(name + "/att_headb", dtype == 1 ? pack_att_headb(FilterView(att.w)) : std::vector<bf16_t>());
    const Layer logit = find_layer(b, "aru_net/logit/class");
    emit(name + "/logit_w", logit.w.data); emit(name + "/logit_b", logit.b.data); emit(name + "/logit_wd", pack_logit_diff(logit));
}

int main() {
    conv_case("c3_8_16", 3, 8, 16, false);                   // C8; bf16 mode 0
    conv_case("c4_12_16", 4, 12, 16, false);                 // three dense C12 chunks; split mode 1 with Cin 12; bf16 Cin 12 -> mode 1
    conv_case("c4_12_16_noc12", 4, 12, 16, false, false);    // the padded 16-group
    conv_case("c3_16_16", 3, 16, 16, false);                 // Winograd; bf16 mode 1; split mode 1
    conv_case("c3_32_32", 3, 32, 32, false);                 // bf16 mode 2; split mode 2; d_ws16 with 2 stages
    conv_case("c3_64_32", 3, 64, 32, false);                 // groups > 2
    conv_case("c4_16_32", 4, 16, 32, false);                 // split mode 1 with 4x4; bf16 mode 1
    conv_case("c4_32_1", 4, 32, 1, false);                   // scalar d_wv; mtiles = 1 with 15 padded rows; split refused; bf16 mode 2
    conv_case("d3_16_8", 3, 16, 8, true);                    // scalar d_wv; six-fragment mode 1; d_wb8; split deconv refused
    conv_case("d3_32_16", 3, 32, 16, true);                  // bf16 mode 2; split deconv with G = 1
    conv_case("d3_64_32", 3, 64, 32, true);                  // ... and G = 2
    // one shape per "left unset" rule, and the refused Cin
    conv_case("c3_24_16", 3, 24, 16, false);
    conv_case("c5_16_16", 5, 16, 16, false);
    conv_case("c3_16_12", 3, 16, 12, false);
    conv_case("c4_8_16", 4, 8, 16, false);
    conv_case("d4_32_16", 4, 32, 16, true);
    conv_case("c3_6_16", 3, 6, 16, false);
    const WeightBlob net = net_blob();
    level0_case("net", net);
    WeightBlob alt = net;                                    // a tail filter of another shape: the fused blocks are left unset
    alt["aru_net/featMapG/unet_up_0/convR_1/weights"] = gen("alt/convR_1/weights", {3, 3, 8, 16});
    level0_case("alt", alt);
    resb_case("resb8", net, 0, 8);
    resb_case("resb16", net, 1, 16);
    resb_case("resb32", net, 2, 32);
    resb_case("resb_other", net, 1, 8);
    for (int d = 0; d < 3; ++d) load_case(net, d);

    // assertion 3 for the level-0 fp32 orders, W[3][3][16][8] = 1 .. 1152, both sources of 8 channels together
    const HostTensor cw = counted({3, 3, 16, 8});
    const FilterView W(cw);
    std::vector<float> pair, direct;
    for (int src = 0; src < 2; ++src) {
        append(pair, pack_pair8(W, 8 * src));
        append(direct, pack_scalar8(W, 8 * src, false));
    }
    check_lands("pair8", pair, cw.count(), 2);               // pixel-pair rows: once per pixel parity
    check_lands("scalar8 direct", direct, cw.count(), 1);    // the scalar direct form: once, no padding
    // the Winograd x-only form of a filter that is 1 at kx = 1 only: G's middle column (0, .5, -.5, 0) at j = 0 .. 3
    HostTensor one;
    one.dims = {3, 3, 8, 8};
    one.data.assign(one.count(), 0.f);
    for (int ky = 0; ky < 3; ++ky)
        for (int i = 0; i < 64; ++i) one.data[((size_t)ky * 3 + 1) * 64 + i] = 1.f;
    const std::vector<float> wv = pack_scalar8(FilterView(one), 0, true);
    CHECK(wv.size() == 768, "scalar8 Winograd: %zu floats", wv.size());
    for (size_t i = 0; i < wv.size(); ++i) CHECK(wv[i] == (float)WINO_G[(i / 32) % 4][1], "scalar8 Winograd: slot %zu holds %g", i, (double)wv[i]);

    // the refusals of the layer lookup
    WeightBlob nob = net;
    nob.erase("aru_net/featMapG/unet_down_0/convR_2/biases");
    for (int which = 0; which < 3; ++which) {
        int code = 0;
        g_err[0] = 0;
        try {
            if (which == 0) pack_res8(nob, true, false);
            else if (which == 1) pack_res8b(nob, true);
            else pack_resb(nob, "aru_net/featMapG/unet_down_0", 8);
        } catch (const PackRefusal& r) { code = r.code; }
        CHECK(code == ASEP_ERR_WEIGHTS && std::string(g_err) == "weights: missing tensor aru_net/featMapG/unet_down_0/convR_2/{weights,biases}",
              "missing bias, packer %d: code %d, '%s'", which, code, g_err);
    }
    CHECK(!pack_res8ws(nob, true).down_w.empty(), "the walkers' filters need no bias");
    printf("aru pack ok: %d checks\n", g_checks);
    return 0;
}
