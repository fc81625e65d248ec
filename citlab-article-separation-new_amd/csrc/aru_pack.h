// ARU-Net weight packing: every fragment order that a kernel header of this directory reads its filters in, as pure host functions
// from the blob's filters to std::vector<float> / std::vector<bf16_t>.  Plain C++17 without HIP: tests/aru_pack_check.cpp compares
// every order with recorded digests on the CPU under the sanitizers.  aru_engine.hip decides which vector goes into which member.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/asep_hip.h"
#include "host_tensor.h"

namespace asep {

void set_error(const char* fmt, ...);

typedef unsigned short bf16_t;                 // as in bf16_kernels.h
typedef std::map<std::string, HostTensor> WeightBlob;
struct PackRefusal { int code; };              // thrown with the error text set: ASEP_ERR_WEIGHTS / ASEP_ERR_UNSUPPORTED

// ---- bfloat16 -----------------------------------------------------------------------------------
inline bf16_t f2bf(float f) {                  // round-to-nearest-even like v_cvt_pk_bf16_f32 (weights have no NaN)
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
inline float bfval(bf16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// fp32 -> its three bfloat16 parts h, m, l (round to nearest at every cut: v = h + m + l exactly)
inline std::array<bf16_t, 3> split3(float v) {
    const bf16_t h = f2bf(v);
    const float r = v - bfval(h);
    const bf16_t m = f2bf(r);
    return {h, m, f2bf(r - bfval(m))};
}

// ---- filter view --------------------------------------------------------------------------------
// conv   W[kh][kw][cin][cout]  (layers.py:219);  deconv W[kh][kw][cout][cin] (layers.py:352, ARU_v1.py:257); zero outside the filter
struct FilterView {
    const float* d;
    int kh, kw, cin, cout;
    bool deconv;
    explicit FilterView(const HostTensor& w, bool deconv_ = false)
        : d(w.data.data()), kh(w.dims[0]), kw(w.dims[1]), cin(w.dims[deconv_ ? 3 : 2]), cout(w.dims[deconv_ ? 2 : 3]), deconv(deconv_) {}
    // a conv filter read as [kh][kw][cin][cout] whatever its dims say (the fused fp32 level-0 blocks: their call condition implies the shape)
    FilterView(const HostTensor& w, int kh_, int kw_, int cin_, int cout_) : d(w.data.data()), kh(kh_), kw(kw_), cin(cin_), cout(cout_), deconv(false) {}
    int taps() const { return kh * kw; }
    float operator()(int tap, int ci, int co) const {
        if (tap < 0 || tap >= taps() || ci >= cin || co >= cout) return 0.f;
        return deconv ? d[((size_t)tap * cout + co) * cin + ci] : d[((size_t)tap * cin + ci) * cout + co];
    }
    float at(int ky, int kx, int ci, int co) const { return (ky < 0 || ky >= kh || kx < 0 || kx >= kw) ? 0.f : (*this)(ky * kw + kx, ci, co); }
    // pixel-pair rows: row = (pixel parity e, cout), the filter column of window pixel p is kx = p - e
    float pair(int ky, int row, int p, int ci) const { return at(ky, p - (row >> 3), ci, row & 7); }
};

inline bool has_shape(const HostTensor& w, int kh, int kw, int cin, int cout) {
    return w.dims.size() == 4 && w.dims[0] == kh && w.dims[1] == kw && w.dims[2] == cin && w.dims[3] == cout;
}

// ---- layer lookup -------------------------------------------------------------------------------
struct Layer { const HostTensor& w; const HostTensor& b; };
inline Layer find_layer(const WeightBlob& blob, const std::string& scope, const char* bias_name = "biases") {
    auto wi = blob.find(scope + "/weights");
    auto bi = blob.find(scope + "/" + bias_name);
    if (wi == blob.end() || bi == blob.end()) {
        set_error("weights: missing tensor %s/{weights,%s}", scope.c_str(), bias_name);
        throw PackRefusal{ASEP_ERR_WEIGHTS};
    }
    return {wi->second, bi->second};
}
inline std::string convR(const std::string& scope, int r) { return scope + "/convR_" + std::to_string(r); }
inline void append(std::vector<float>& dst, const std::vector<float>& v) { dst.insert(dst.end(), v.begin(), v.end()); }

// ---- fragment writers ---------------------------------------------------------------------------
// A fragments of v_mfma_f32_16x16x4_f32, one block [mtile][lane][4]: element (mt, lane, r) = f(mt, row = lane & 15, kk = lane >> 4, r)
template <class F>
void put_frag4(float* dst, int mtiles, F f) {
    for (int mt = 0; mt < mtiles; ++mt)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) dst[((size_t)mt * 64 + lane) * 4 + r] = f(mt, lane & 15, lane >> 4, r);
}
// A fragments of v_mfma_f32_16x16x32_bf16, `parts` blocks [mtile][lane][8] (k = 8 kk + j): one block of rounded values, or the three
// blocks h, m, l of split3
template <class F>
void put_frag8(bf16_t* dst, int parts, int mtiles, F f) {
    const size_t blk = (size_t)mtiles * 64 * 8;
    for (int mt = 0; mt < mtiles; ++mt)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const float v = f(mt, lane & 15, lane >> 4, j);
                const size_t i = ((size_t)mt * 64 + lane) * 8 + j;
                if (parts == 1) { dst[i] = f2bf(v); continue; }
                const std::array<bf16_t, 3> p = split3(v);
                for (int s = 0; s < 3; ++s) dst[s * blk + i] = p[s];
            }
}

// ---- shape decisions of one conv / deconv layer ---------------------------------------------------
struct ConvPlan {
    int kh = 0, kw = 0, cin = 0, cout = 0;
    bool c8 = false;       // Cin == 8: two taps per 16-slot chunk
    bool c12 = false;      // Cin == 12, 4x4 taps (attention conv2): dense rows of 48 floats = 3 chunks, no channel padding
    bool deconv = false;
    int groups = 0, mtiles = 0, nchunks = 0;
    // native bf16 path (bf16_kernels.h): A fragments of v_mfma_f32_16x16x32_bf16, 8 bf16 per lane
    int bmode = -1;        // convb / deconvb MODE (0: Cin 8, 1: Cin 16, 2: Cin % 32 == 0); -1: not packed
    int bchunks = 0;       // 0: no bf16 fragments (not served by convb / deconvb: refused at run time if it is needed)
    // fp32 with split products (split_kernels.h)
    int smode = -1;        // 1: Cin 12 / 16 (chunk = two taps), 2: Cin % 32 == 0 (chunk = tap x 32 channels); -1: not packed
    int taps() const { return kh * kw; }
    bool k3() const { return kh == 3 && kw == 3; }
    bool wino() const { return !deconv && k3() && cin % 16 == 0 && cout % 16 == 0; }
    bool wv_deconv8() const { return deconv && k3() && cin == 16 && cout == 8; }
    bool wv_c1out() const { return !deconv && kh == 4 && kw == 4 && cin == 32 && cout == 1; }
    bool wb8() const { return deconv && bmode == 1 && cout == 8; }
    bool ws16() const { return !deconv && smode > 0 && k3() && cin % 16 == 0 && cin >= 32; }
};

inline int conv_bmode(int cin) { return cin == 8 ? 0 : (cin == 16 ? 1 : (cin % 32 == 0 ? 2 : -1)); }
inline int frag_chunks(int mode, int kh, int kw, int cin) { return mode == 0 ? kh : (mode == 1 ? (kh * kw + 1) / 2 : (cin / 32) * kh * kw); }

// use_c12: 12-channel inputs as three dense chunks (off: padded to a 16-channel group); bf16 / split: the engine's compute_dtype 1 / 2
inline ConvPlan conv_plan(const std::string& scope, const Layer& L, bool deconv, bool use_c12, bool bf16, bool split) {
    const HostTensor& w = L.w;
    if (w.dims.size() != 4) {
        set_error("weights: %s/weights must have rank 4", scope.c_str());
        throw PackRefusal{ASEP_ERR_WEIGHTS};
    }
    ConvPlan p;
    p.kh = w.dims[0];
    p.kw = w.dims[1];
    p.deconv = deconv;
    p.cin = deconv ? w.dims[3] : w.dims[2];
    p.cout = deconv ? w.dims[2] : w.dims[3];
    if ((int)L.b.count() != p.cout) {
        set_error("weights: %s bias has %zu elements, expected %d", scope.c_str(), L.b.count(), p.cout);
        throw PackRefusal{ASEP_ERR_WEIGHTS};
    }
    if (p.cin % 4 != 0) {
        set_error("weights: %s has Cin=%d; the MFMA path needs Cin %% 4 == 0", scope.c_str(), p.cin);
        throw PackRefusal{ASEP_ERR_UNSUPPORTED};
    }
    p.c8 = !deconv && p.cin == 8;
    p.c12 = !deconv && p.cin == 12 && p.kh == 4 && p.kw == 4 && p.cout <= 16 && use_c12;
    p.mtiles = (p.cout + 15) / 16;
    p.groups = (p.c8 || p.c12) ? 1 : (p.cin + 15) / 16;
    p.nchunks = p.c8 ? (p.taps() + 1) / 2 : (p.c12 ? p.kh * (p.kw * 12 / 16) : p.groups * p.taps());
    if (bf16 && !deconv) {
        // the 12-channel output of the attention head is stored as a 16-channel plane (4 zero channels): Cin 12 -> mode 1
        p.bmode = conv_bmode(p.cin == 12 ? 16 : p.cin);
        if (p.bmode > 0 || (p.bmode == 0 && p.kh == 3)) p.bchunks = frag_chunks(p.bmode, p.kh, p.kw, p.cin);
    }
    if (bf16 && deconv && p.k3()) {
        p.bmode = p.cin == 16 ? 1 : (p.cin % 32 == 0 ? 2 : -1);
        p.bchunks = p.bmode == 1 ? 6 : (p.bmode == 2 ? p.cin / 32 * 9 : 0);
    }
    if (split && !deconv && (p.k3() || (p.kh == 4 && p.kw == 4)) && p.cout % 16 == 0) {
        p.smode = (p.cin == 16 || p.cin == 12) ? 1 : (p.cin % 32 == 0 ? 2 : -1);
        if (p.smode == 2 && p.kh != 3) p.smode = -1;         // 4x4 filters are instantiated for the 12- / 16-channel form only: such a layer keeps the fp32 MFMA kernel
    }
    if (split && deconv && p.k3() && p.cin % 32 == 0 && p.cout % 16 == 0) p.smode = 2;      // (level 0, 16 -> 8: deconv8v_kernel)
    return p;
}

// ---- fp32 orders of a conv / deconv layer -------------------------------------------------------
// A operand of v_mfma_f32_16x16x4_f32, [chunk][mtile][lane][4], slot = 4 kk + r.  C8: chunk = two taps x 8 channels;
// C12: the 48 floats of a filter row (4 taps x 12 channels) as three dense chunks; else chunk = (group of 16 channels, tap)
inline std::vector<float> pack_mfma_a(const FilterView& W, const ConvPlan& p) {
    std::vector<float> pk((size_t)p.nchunks * p.mtiles * 64 * 4);
    for (int ch = 0; ch < p.nchunks; ++ch)
        put_frag4(&pk[(size_t)ch * p.mtiles * 256], p.mtiles, [&](int mt, int row, int kk, int r) {
            int tap, ci;
            if (p.c8) {
                tap = 2 * ch + (kk >> 1);
                ci = 4 * (kk & 1) + r;
            } else if (p.c12) {
                const int cpr = p.kw * 12 / 16, ky = ch / cpr, flat = (ch % cpr) * 16 + 4 * kk + r;   // float of the row's run
                tap = ky * p.kw + flat / 12;
                ci = flat % 12;
            } else {
                tap = ch % p.taps();
                ci = 16 * (ch / p.taps()) + 4 * kk + r;
            }
            return W(tap, ci, mt * 16 + row);
        });
    return pk;
}

// Winograd F(2,3): G of U = G g G^T (2-D, double accumulation) and of its x-only form U_j = sum_kx G[j][kx] g[ky][kx]
constexpr double WINO_G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};

// Winograd F(2x2,3x3) transformed weights U = G g G^T, packed [g][pos = 4 a + b][mtile][lane][4]
inline std::vector<float> pack_wino(const FilterView& W, const ConvPlan& p) {
    std::vector<float> wk((size_t)p.groups * 16 * p.mtiles * 64 * 4);
    for (int g = 0; g < p.groups; ++g)
        for (int pos = 0; pos < 16; ++pos)
            put_frag4(&wk[((size_t)g * 16 + pos) * p.mtiles * 256], p.mtiles, [&](int mt, int row, int kk, int r) {
                double u = 0;
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) u += WINO_G[pos >> 2][i] * (double)W(i * 3 + j, 16 * g + 4 * kk + r, mt * 16 + row) * WINO_G[pos & 3][j];
                return (float)u;
            });
    return wk;
}

// scalar-operand filters of the vector-ALU kernels: deconv 16 -> 8 [tap][ci][co] (deconv8v_kernel), 4x4 conv 32 -> 1 [tap][ci] (conv_c1out_kernel)
inline std::vector<float> pack_wv(const FilterView& W) {
    std::vector<float> wv((size_t)W.taps() * W.cin * W.cout);
    for (int tap = 0; tap < W.taps(); ++tap)
        for (int ci = 0; ci < W.cin; ++ci)
            for (int co = 0; co < W.cout; ++co) wv[((size_t)tap * W.cin + ci) * W.cout + co] = W(tap, ci, co);
    return wv;
}

// ---- bf16 orders of a conv / deconv layer (parts = 1) and their three-part forms (parts = 3) -----
// k-slot (kk, j) of chunk ch -> filter tap and input channel; a tap outside the filter is a zero slot
//   mode 0: chunk = ky, k = 8 kx + ci (kx = 3: zero);  mode 1: chunk c, k = 16 (tap - 2c) + ci;  mode 2: chunk = G taps + tap, k = ci - 32 G
struct KSlot { int tap, ci; };
inline KSlot kslot(int mode, int ch, int kk, int j, int kw, int taps) {
    if (mode == 0) return {kk < kw ? ch * kw + kk : -1, j};
    if (mode == 1) return {2 * ch + (kk >> 1), (kk & 1) * 8 + j};
    return {ch % taps, 32 * (ch / taps) + kk * 8 + j};
}

// A fragments of a conv for convb_kernel / resb_tail_kernel and of a 3x3 deconv with Cin % 32 == 0 for deconvb_kernel (mode 2: [G][tap]),
// [chunk][mtile][lane][8]; with parts = 3 the filter of convs_kernel / deconvs_kernel as three bf16 parts, [chunk][part h, m, l][mtile][lane][8]
inline std::vector<bf16_t> pack_frags(const FilterView& W, int mode, int mtiles, int parts) {
    const int chunks = frag_chunks(mode, W.kh, W.kw, W.cin);
    const size_t blk = (size_t)parts * mtiles * 64 * 8;
    std::vector<bf16_t> pk(chunks * blk);
    for (int ch = 0; ch < chunks; ++ch)
        put_frag8(&pk[ch * blk], parts, mtiles, [&](int mt, int row, int kk, int j) {
            const KSlot s = kslot(mode, ch, kk, j, W.kw, W.taps());
            return W(s.tap, s.ci, mt * 16 + row);
        });
    return pk;
}

// 3x3, Cin % 16 == 0, Cin >= 32: stages of 16 channels, chunk = two taps (convs16_kernel): [stage][chunk 5][part][mtile][lane][8]
inline std::vector<bf16_t> pack_split16(const FilterView& W, int mtiles) {
    const int stages = W.cin / 16;
    const size_t blk = (size_t)3 * mtiles * 64 * 8;
    std::vector<bf16_t> pk(stages * 5 * blk);
    for (int g = 0; g < stages; ++g)
        for (int t = 0; t < 5; ++t)
            put_frag8(&pk[(g * 5 + t) * blk], 3, mtiles, [&](int mt, int row, int kk, int j) {
                const KSlot s = kslot(1, t, kk, j, W.kw, W.taps());
                return W(s.tap, 16 * g + s.ci, mt * 16 + row);
            });
    return pk;
}

// 3x3 deconv, Cin 16: the tap that output class (py, px) takes from input pixel (dy, dx) of its 2 x 2 window, -1: none (k = 16 dx + ci)
inline int deconv_tap(int dy, int py, int px, int dx) {
    const int ky = py ? 1 : (dy ? 2 : 0), kx = px ? (dx ? -1 : 1) : (dx ? 2 : 0);
    return kx < 0 ? -1 : ky * 3 + kx;
}
// deconvb_kernel MODE 1, [frag 0..5][mtile][lane][8]: fragment f: dy = f >= 4; class (py, px) = dy ? (0, f & 1) : (f >> 1, f & 1)
inline std::vector<bf16_t> pack_deconv6(const FilterView& W, int mtiles) {
    const size_t blk = (size_t)mtiles * 64 * 8;
    std::vector<bf16_t> pk(6 * blk);
    for (int f = 0; f < 6; ++f)
        put_frag8(&pk[f * blk], 1, mtiles, [&](int mt, int row, int kk, int j) {
            const int dy = f >= 4;
            return W(deconv_tap(dy, dy ? 0 : (f >> 1), f & 1, kk >> 1), (kk & 1) * 8 + j, mt * 16 + row);
        });
    return pk;
}
// deconvb8_kernel (16 -> 8, level 0), [3][lane][8]: fragment q = (dy = 0, py = 0), (dy = 0, py = 1), (dy = 1, py = 0); row m = 8 px + co
inline std::vector<bf16_t> pack_deconv8(const FilterView& W) {
    std::vector<bf16_t> pk(3 * 512);
    for (int q = 0; q < 3; ++q)
        put_frag8(&pk[q * 512], 1, 1, [&](int, int row, int kk, int j) { return W(deconv_tap(q == 2, q == 1, row >> 3, kk >> 1), (kk & 1) * 8 + j, row & 7); });
    return pk;
}

// every order of one layer
struct ConvPack {
    ConvPlan plan;
    std::vector<float> w, wino, wv;            // empty: not packed for this shape
    std::vector<bf16_t> wb, wb8, ws, ws16;
};
inline ConvPack pack_conv_layer(const std::string& scope, const Layer& L, bool deconv, bool use_c12, bool bf16, bool split) {
    ConvPack c;
    const ConvPlan& p = c.plan = conv_plan(scope, L, deconv, use_c12, bf16, split);
    const FilterView W(L.w, deconv);
    c.w = pack_mfma_a(W, p);
    if (p.wino()) c.wino = pack_wino(W, p);
    if (p.wv_deconv8() || p.wv_c1out()) c.wv = pack_wv(W);
    if (p.bchunks) c.wb = (deconv && p.bmode == 1) ? pack_deconv6(W, p.mtiles) : pack_frags(W, p.bmode, p.mtiles, 1);
    if (p.wb8()) c.wb8 = pack_deconv8(W);
    if (p.smode > 0) c.ws = pack_frags(W, p.smode, p.mtiles, 3);
    if (p.ws16()) c.ws16 = pack_split16(W, p.mtiles);
    return c;
}

// the three convR filters of a residual block for resb_tail_kernel<C> / res32_tail_kernel: [3][chunk][mtile][64][8] + biases [3][C]
struct ResbPack { bool ok = false; std::vector<bf16_t> w; std::vector<float> b; };      // !ok: not this shape, layer by layer
inline ResbPack pack_resb(const WeightBlob& blob, const std::string& scope, int C) {
    ResbPack o;
    for (int r = 0; r < 3; ++r) {
        const Layer L = find_layer(blob, convR(scope, r));
        if (!has_shape(L.w, 3, 3, C, C)) return ResbPack();
        const std::vector<bf16_t> f = pack_frags(FilterView(L.w), conv_bmode(C), C == 32 ? 2 : 1, 1);
        o.w.insert(o.w.end(), f.begin(), f.end());
        append(o.b, L.b.data);
    }
    o.ok = true;
    return o;
}

// ---- level 0: 3x3 filters W[3][3][cin][8] on pixel-pair rows ---------------------------------------
// fp32 pixel-pair A fragments of the 8 input channels from ci0 on: [ky][h][lane][4], slot s = 4 kk + r: window pixel 2h + (s>>3), ci = s&7
inline std::vector<float> pack_pair8(const FilterView& W, int ci0) {
    std::vector<float> pk(3 * 2 * 256);
    for (int ky = 0; ky < 3; ++ky)
        for (int h = 0; h < 2; ++h)
            put_frag4(&pk[(ky * 2 + h) * 256], 1, [&](int, int row, int kk, int r) { return W.pair(ky, row, 2 * h + ((4 * kk + r) >> 3), ci0 + ((4 * kk + r) & 7)); });
    return pk;
}

// bf16 pixel-pair A fragment of filter row ky, `parts` x [lane][8], k = 8 kk + j.  Narrow (res8b / res8f / res8ws kernels, 8 input channels from
// ci0 on): window pixel kk, ci = ci0 + j.  Wide (half hf of the 4-pixel window, 16 input channels): window pixel 2 hf + (kk >> 1), ci = 8 (kk & 1) + j
inline void put_pair(bf16_t* dst, int parts, const FilterView& W, int ky, int ci0, int hf = -1) {
    put_frag8(dst, parts, 1, [&](int, int row, int kk, int j) {
        return hf < 0 ? W.pair(ky, row, kk, ci0 + j) : W.pair(ky, row, 2 * hf + (kk >> 1), 8 * (kk & 1) + j);
    });
}
// [ky][source of 8 channels][part][lane][8]: the filter rows of res8b_kernel (cin 8), the two planes of res8f_kernel's conv1 (cin 16), and with
// parts = 3 the walkers' three-part forms (res8ws_kernels.h)
inline void append_pairs(std::vector<bf16_t>& dst, const FilterView& W, int parts) {
    const int srcs = W.cin / 8;
    const size_t at = dst.size(), blk = (size_t)parts * 512;
    dst.resize(at + 3 * srcs * blk);
    for (int ky = 0; ky < 3; ++ky)
        for (int s = 0; s < srcs; ++s) put_pair(&dst[at + (ky * srcs + s) * blk], parts, W, ky, 8 * s);
}
// conv1 of unet_up_0 for res8b_kernel: [ky][half][lane][8], wide form
inline std::vector<bf16_t> pack_pair_wide(const FilterView& W) {
    std::vector<bf16_t> pk(3 * 2 * 512);
    for (int ky = 0; ky < 3; ++ky)
        for (int hf = 0; hf < 2; ++hf) put_pair(&pk[(ky * 2 + hf) * 512], 1, W, ky, 0, hf);
    return pk;
}

// scalar layout of the 8 input channels from ci0 on (res8v_kernels.h).  Direct: [g = (ky*2 + hf)*3 + kx][c][co], input channel ci0 + hf*4 + c.
// Winograd F(2,3) along x (wino: the kernels' R8V_WINO): [(ky*2 + hf)*4 + j][c][co], U_j = sum_kx G[j][kx] g[ky][kx] (double accumulation)
inline std::vector<float> pack_scalar8(const FilterView& W, int ci0, bool wino) {
    const int nx = wino ? 4 : 3;
    std::vector<float> pk((size_t)6 * nx * 32);
    for (int rh = 0; rh < 6; ++rh)
        for (int x = 0; x < nx; ++x)
            for (int c = 0; c < 4; ++c)
                for (int co = 0; co < 8; ++co) {
                    const int ci = ci0 + (rh & 1) * 4 + c;
                    double u = W.at(rh >> 1, x, ci, co);
                    if (wino) {
                        u = 0;
                        for (int kx = 0; kx < 3; ++kx) u += WINO_G[x][kx] * (double)W.at(rh >> 1, kx, ci, co);
                    }
                    pk[((rh * nx + x) * 4 + c) * 8 + co] = (float)u;
                }
    return pk;
}

// the fused fp32 level-0 blocks (res8_kernels.h pixel-pair fragments, res8v_kernels.h scalar layout)
struct Res8Pack {
    std::vector<float> down_wr, down_br, v_down_wr;            // [3][6][64][4], [3][8], [3][filter]
    std::vector<float> up_w1, up_wr, up_br, up_b1, v_up_w1, v_up_wr;   // up_w1: skip channels 0..7, then deconv channels 8..15
};
inline Res8Pack pack_res8(const WeightBlob& blob, bool up, bool wino) {
    Res8Pack o;
    const std::string d = "aru_net/featMapG/unet_down_0", u = "aru_net/featMapG/unet_up_0";
    for (int r = 0; r < 3; ++r) {
        const Layer L = find_layer(blob, convR(d, r));
        const FilterView W(L.w, 3, 3, 8, 8);
        append(o.down_wr, pack_pair8(W, 0));
        append(o.v_down_wr, pack_scalar8(W, 0, wino));
        append(o.down_br, L.b.data);
    }
    if (!up) return o;
    const Layer L1 = find_layer(blob, u + "/conv1");
    for (int src = 0; src < 2; ++src) {
        append(o.up_w1, pack_pair8(FilterView(L1.w, 3, 3, 16, 8), 8 * src));
        append(o.v_up_w1, pack_scalar8(FilterView(L1.w, 3, 3, 16, 8), 8 * src, wino));
    }
    o.up_b1 = L1.b.data;
    for (int r = 0; r < 3; ++r) {
        const Layer L = find_layer(blob, convR(u, r));
        const FilterView W(L.w, 3, 3, 8, 8);
        append(o.up_wr, pack_pair8(W, 0));
        append(o.v_up_wr, pack_scalar8(W, 0, wino));
        append(o.up_br, L.b.data);
    }
    return o;
}

// the split-product walkers' filters (f32s engine): both level-0 tails [3 convs][3 ky][3 parts][64][8] and the UP block's conv1
// [3 ky][2 sources][3 parts][64][8]; all empty (the walkers off) for other shapes
struct Res8wsPack { std::vector<bf16_t> down_w, up_w, up_w1; };
inline Res8wsPack pack_res8ws(const WeightBlob& blob, bool up) {
    auto tail = [&](const std::string& scope, std::vector<bf16_t>& pk) {
        for (int r = 0; r < 3; ++r) {
            auto wi = blob.find(convR(scope, r) + "/weights");
            if (wi == blob.end() || !has_shape(wi->second, 3, 3, 8, 8)) return false;
            append_pairs(pk, FilterView(wi->second), 3);
        }
        return true;
    };
    Res8wsPack o;
    if (!tail("aru_net/featMapG/unet_down_0", o.down_w)) return Res8wsPack();
    if (up) {
        auto w1 = blob.find("aru_net/featMapG/unet_up_0/conv1/weights");
        if (!tail("aru_net/featMapG/unet_up_0", o.up_w) || w1 == blob.end() || !has_shape(w1->second, 3, 3, 16, 8)) return Res8wsPack();
        append_pairs(o.up_w1, FilterView(w1->second), 3);
    }
    return o;
}

// whole level-0 blocks of the bf16 path (res8b_kernel, res8f_kernel): pixel-pair fragments; a block whose filters have another shape stays
// empty (generic kernels)
struct Res8bPack {
    std::vector<bf16_t> down_w, up_w;          // [3 convs][3 ky][64][8]
    std::vector<float> down_b, up_b, up_b1;    // [3][8], [3][8], [8]
    std::vector<bf16_t> f_down_w1;             // conv1 of unet_down_0 (1 -> 8) as ONE pair fragment [64][8]
    std::vector<float> down_w1r;               // the same filter [9][8] as fp32 values rounded to bfloat16
    std::vector<bf16_t> up_w1, f_up_w1;        // conv1 of unet_up_0: [3 ky][2 halves][64][8] (res8b), [3 ky][2 sources][64][8] (res8f)
};
inline Res8bPack pack_res8b(const WeightBlob& blob, bool up) {
    auto tail = [&](const std::string& scope, std::vector<bf16_t>& pk, std::vector<float>& br) {
        for (int r = 0; r < 3; ++r) {
            const Layer L = find_layer(blob, convR(scope, r));
            if (!has_shape(L.w, 3, 3, 8, 8)) { pk.clear(); br.clear(); return false; }
            append_pairs(pk, FilterView(L.w), 1);
            append(br, L.b.data);
        }
        return true;
    };
    Res8bPack o;
    const std::string d = "aru_net/featMapG/unet_down_0", u = "aru_net/featMapG/unet_up_0";
    if (!tail(d, o.down_w, o.down_b)) return o;
    auto w1 = blob.find(d + "/conv1/weights");
    if (w1 != blob.end() && has_shape(w1->second, 3, 3, 1, 8)) {
        // row m = (parity e, cout); k = 8 kk + jj: window row 2 kk + (jj >> 2) (kk < 2), column jj & 3
        const FilterView W(w1->second);
        o.f_down_w1.resize(512);
        put_frag8(o.f_down_w1.data(), 1, 1, [&](int, int row, int kk, int jj) { return W.pair(kk < 2 ? 2 * kk + (jj >> 2) : -1, row, jj & 3, 0); });
        o.down_w1r.resize(w1->second.data.size());
        for (size_t i = 0; i < o.down_w1r.size(); ++i) o.down_w1r[i] = bfval(f2bf(w1->second.data[i]));
    }
    if (!up) return o;
    const Layer L1 = find_layer(blob, u + "/conv1");
    if (!has_shape(L1.w, 3, 3, 16, 8) || !tail(u, o.up_w, o.up_b)) return o;
    o.up_w1 = pack_pair_wide(FilterView(L1.w));
    o.up_b1 = L1.b.data;
    append_pairs(o.f_up_w1, FilterView(L1.w), 1);
    return o;
}

// ---- first layers and the logits ------------------------------------------------------------------
// Cin == 1 first layers, uploaded as stored: [k*k][cout]
inline Layer find_direct(const WeightBlob& blob, const std::string& scope) {
    const Layer L = find_layer(blob, scope);
    if (L.w.dims.size() != 4 || L.w.dims[2] != 1 || L.w.dims[0] != L.w.dims[1]) {
        set_error("weights: %s must be [k,k,1,cout]", scope.c_str());
        throw PackRefusal{ASEP_ERR_UNSUPPORTED};
    }
    return L;
}
// Cin == 3 first layer of a colour net (conv_c3_kernel).  No re-layout: the kernel reads TensorFlow's own [ky][kx][ci][cout] order, which runs
// in step with the pixel-interleaved page.  This function checks the shape ([3,3,3,cout], cout 8 or 16: the instantiated kernels) and the bias
// length and, for the bf16 engine, rounds every coefficient to bfloat16 (its first layer multiplies bfloat16 filter and image values in fp32;
// conv_c1_kernel does that rounding while it fills its LDS filter, here it is done once at load).
inline std::vector<float> pack_first_rgb(const std::string& scope, const Layer& L, bool bf16) {
    if (L.w.dims.size() != 4 || L.w.dims[0] != 3 || L.w.dims[1] != 3 || L.w.dims[2] != 3 || (L.w.dims[3] != 8 && L.w.dims[3] != 16)) {
        set_error("weights: %s must be [3,3,3,8] or [3,3,3,16] for 3-channel input", scope.c_str());
        throw PackRefusal{ASEP_ERR_UNSUPPORTED};
    }
    const FilterView W(L.w);
    if ((int)L.b.count() != W.cout) {
        set_error("weights: %s bias has %zu elements, expected %d", scope.c_str(), L.b.count(), W.cout);
        throw PackRefusal{ASEP_ERR_WEIGHTS};
    }
    std::vector<float> pk(L.w.data);
    if (bf16)
        for (float& v : pk) v = bfval(f2bf(v));
    return pk;
}
// attPart/conv1 [4][4][1][12] as ONE fp32 A fragment for att_head_kernel: row = cout (12 of 16), kk = ky, r = kx
inline std::vector<float> pack_att_head(const FilterView& W) {
    std::vector<float> pk(256);
    put_frag4(pk.data(), 1, [&](int, int row, int kk, int r) { return W.at(kk, r, 0, row); });
    return pk;
}
// the same as ONE bf16 fragment [64][8] (att_headb_kernel): k = 8 kk + 4 r + c <-> tap (2 kk + r, c) for kk < 2, zero rows / slots elsewhere
inline std::vector<bf16_t> pack_att_headb(const FilterView& W) {
    std::vector<bf16_t> pk(512);
    put_frag8(pk.data(), 1, 1, [&](int, int row, int kk, int i) { return W.at(kk < 2 ? 2 * kk + (i >> 2) : -1, i & 3, 0, row); });
    return pk;
}
// two classes: [16][feat_root] class-1 minus class-0 filter + the bias difference (combine_kernel behind a soft-max)
inline std::vector<float> pack_logit_diff(const Layer& L) {
    const std::vector<float>& w = L.w.data;    // [4][4][feat_root][2]
    std::vector<float> wd(w.size() / 2 + 1);
    for (size_t i = 0; i + 1 < wd.size(); ++i) wd[i] = w[2 * i + 1] - w[2 * i];
    wd.back() = L.b.data[1] - L.b.data[0];
    return wd;
}


// ---- RU_v2 (asep_aru_cfg.input_pyramid) -------------------------------------------------------------
// The graph's variables live under ru_net/..., and conv1 of every block that reads the pooled page I_l has `channels` more input rows, LAST in
// the concat (RU_v2.py:101,144): down blocks l >= 1 [3,3,f_{l-1} + channels,f_l], with inp4up up blocks [3,3,2 f_l + channels,f_l].  Returns the
// blob that the packers above read -- the same tensors under aru_net/..., those filters cut to their main rows (the layer the conv kernels run)
// -- and leaves the image rows [9][channels][f_l] (pyr_tap_kernel's order) in taps[<aru_net scope of the conv1>].  max_cout: the widest conv1 the
// tap kernel serves (PYR_MAX_COUT of pyr_kernels.h, where the bound is derived); a wider one is refused here, before anything is launched.
inline WeightBlob split_pyramid_blob(const WeightBlob& in, const asep_aru_cfg& cfg, std::map<std::string, std::vector<float>>& taps, int max_cout) {
    WeightBlob out;
    for (const auto& kv : in) out[kv.first.compare(0, 7, "ru_net/") == 0 ? "aru_" + kv.first.substr(3) : kv.first] = kv.second;
    const int n = cfg.scale_space_num, ch = cfg.channels;
    auto cut = [&](const std::string& scope, int cmain, int f) {
        if (f % 4 != 0 || f > max_cout) {
            set_error("weights: %s has %d output channels: the input-pyramid tap serves multiples of 4 up to %d", scope.c_str(), f, max_cout);
            throw PackRefusal{ASEP_ERR_UNSUPPORTED};
        }
        auto wi = out.find(scope + "/weights");
        if (wi == out.end() || !has_shape(wi->second, 3, 3, cmain + ch, f)) {
            set_error("weights: ru%s/weights must be [3,3,%d,%d] (%d channels + the %d of the pooled page, RU_v2.py:101,144)", scope.c_str() + 3,
                      cmain + ch, f, cmain, ch);
            throw PackRefusal{ASEP_ERR_WEIGHTS};
        }
        const std::vector<float> w = wi->second.data;
        HostTensor& mainw = wi->second;
        mainw.dims[2] = cmain;
        mainw.data.resize((size_t)9 * cmain * f);
        std::vector<float>& tap = taps[scope];
        tap.resize((size_t)9 * ch * f);
        for (int t = 0; t < 9; ++t) {
            const float* row = &w[(size_t)t * (cmain + ch) * f];
            std::copy(row, row + (size_t)cmain * f, &mainw.data[(size_t)t * cmain * f]);
            std::copy(row + (size_t)cmain * f, row + (size_t)(cmain + ch) * f, &tap[(size_t)t * ch * f]);
        }
    };
    for (int l = 1; l < n; ++l) cut("aru_net/featMapG/unet_down_" + std::to_string(l) + "/conv1", cfg.feat_root << (l - 1), cfg.feat_root << l);
    if (cfg.inp4up)
        for (int l = 0; l + 1 < n; ++l) cut("aru_net/featMapG/unet_up_" + std::to_string(l) + "/conv1", 2 * (cfg.feat_root << l), cfg.feat_root << l);
    return out;
}

}  // namespace asep
