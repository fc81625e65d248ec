// Input-pyramid kernels of the RU_v2 graph (RU_v2.py:92-101,142-144; asep_aru_cfg.input_pyramid / .inp4up; fp32 engines f32 and f32s).
//
// RU_v2 concatenates the average-pooled page I_l behind the input of conv1 of its blocks.  A convolution is linear over concatenated input
// channels: conv1(concat[a, I_l]) = conv1_main(a) + tap(I_l), tap = the 3x3 SAME convolution of the CH-channel pooled page (CH = 1 gray, 3
// colour) with the LAST CH input rows of conv1/weights, no bias.  conv1_main is the layer the engine's conv kernels already run, unchanged;
// pyr_tap_kernel adds the tap to its result t in place.
//
//   pyr_tap_kernel<CH>:  t[h,w,cout] += tap(I[h,w,CH]); cout a run-time multiple of 4 (<= PYR_MAX_COUT: the filter lies in LDS).  One block = 64 x 4
//     pixels.  The block puts its standardised 66 x 6 window (zero outside the page = SAME padding; {mean, 1/std} applied while loading like
//     the first-layer kernels do) and the 9 CH cout filter values into LDS; a thread then takes (pixel, channel quad) items, consecutive
//     threads consecutive quads of a pixel and then the next pixel of the row, so every load and store of t is a 16-byte access and a wave's
//     accesses are one contiguous range of a row.  Sums: 9 CH fp32 FMAs per channel from zero in the fixed order (ky, kx, ci), then ONE add
//     to t: the result of a pixel does not depend on the tile, the launch or the other pages of a call.
//     Bound: the kernel reads and writes cout floats per pixel (8 cout bytes; the page's CH floats are negligible) against 18 CH cout flops.
//   avgpool2_cn_kernel<C>: the pyramid of a colour page -- layers.avg_pool2d 2x2 / stride 2 / SAME (ceil mode, divisor = valid pixels) over C
//     interleaved channels, the association of avgpool2_c1_kernel: ((v00 + v01) + v10) + v11 over the values that exist.  Gray pages use
//     avgpool2_c1_kernel itself.
//
// Both are templates launched only from the last functions of aru_engine.hip, so that they are emitted behind every other kernel of the
// code object (see the note there).
#pragma once
#include "aru_kernels.h"

namespace asep {

constexpr int PYR_TW = 64, PYR_TH = 4;                         // output pixels of a block
constexpr int pyr_win_floats(int ch) { return (PYR_TH + 2) * (PYR_TW + 2) * ch; }      // 396 ch: a multiple of 4 (the filter behind it is 16-byte aligned)
constexpr size_t pyr_tap_lds(int ch, int cout) { return ((size_t)pyr_win_floats(ch) + (size_t)9 * ch * cout) * sizeof(float); }
// The widest tapped conv1.  A block's dynamic LDS is pyr_tap_lds(ch, cout) = (396 ch + 9 ch cout) * 4 bytes, and launch_pyr_tap asks for it
// without hipFuncAttributeMaxDynamicSharedMemorySize, so a launch may count on 64 KiB and no more.  At cout = 256 that is 10 800 bytes gray and
// 32 400 bytes colour: half the limit, and four blocks a CU.  The LDS alone would hold up to cout 560 in colour ((16384 - 1188) / 27, down to a
// multiple of 4) and 1776 gray; 1024 channels in colour (feat_root 32, six levels) ask for 115 344 bytes and cannot launch.  The bound stays
// at 256, the widest level that the engine's other layers are compared at (feat_root 16 with five levels, feat_root 8 with six): it is what
// asep_aru_load refuses beyond (split_pyramid_blob, with the layer and this limit in the message), and the assertion below ties it to the LDS.
constexpr int PYR_MAX_COUT = 256;
constexpr size_t PYR_LDS_LIMIT = 64 * 1024;                    // dynamic LDS of a launch without the opt-in attribute
static_assert(pyr_tap_lds(3, PYR_MAX_COUT) <= PYR_LDS_LIMIT && pyr_tap_lds(1, PYR_MAX_COUT) <= PYR_LDS_LIMIT, "the tap's window and filter must fit the LDS of a plain launch");

struct TapProb {
    const float* img;      // pooled page of the block's level [H,W,CH], values as fed (not standardised)
    float* t;              // conv1's result [H,W,cout], updated in place
    const float* stats;    // {mean, 1/std} of the page or nullptr
    int H, W;
    int tiles_x;           // 64-pixel-wide, 4-row blocks per row
    int tile_begin;
};
struct TapArgs {
    TapProb p[MAXP];
    int nprob;
    const float* w;        // [3*3][CH][cout]: the image rows of conv1/weights
    int cout;
};

template <int CH>
__global__ __launch_bounds__(256) void pyr_tap_kernel(const TapArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pyr_lds[];
    constexpr int WR = (PYR_TW + 2) * CH;                     // floats of a window row
    float* __restrict__ win = pyr_lds;                         // [PYR_TH + 2][WR]
    float* __restrict__ sw = pyr_lds + pyr_win_floats(CH);     // [9][CH][cout]
    const int pi = prob_of_tile(a, (int)blockIdx.x);
    const TapProb& P = a.p[pi];
    const int tile = blockIdx.x - P.tile_begin;
    const int ty = tile / P.tiles_x, tx = tile - ty * P.tiles_x;
    const int x0 = tx * PYR_TW, y0 = ty * PYR_TH;
    const int H = P.H, W = P.W, cout = a.cout;
    float mean = 0.f, inv = 1.f;
    if (P.stats) { mean = P.stats[0]; inv = P.stats[1]; }
    const float* __restrict__ img = P.img;
    const long rowf = (long)W * CH;                            // floats of a page row
    for (int i = threadIdx.x; i < (PYR_TH + 2) * WR; i += 256) {
        const int r = i / WR, c = i - r * WR;
        const int gy = y0 + r - 1;
        const long gc = (long)(x0 - 1) * CH + c;               // float index inside the page row
        float v = 0.f;
        if (gy >= 0 && gy < H && gc >= 0 && gc < rowf) v = (img[(size_t)gy * rowf + gc] - mean) * inv;
        win[i] = v;
    }
    for (int i = threadIdx.x; i < 9 * CH * cout; i += 256) sw[i] = a.w[i];
    __syncthreads();
    const int nq = cout >> 2;
    float* __restrict__ t = P.t;
    for (int j = threadIdx.x; j < 256 * nq; j += 256) {
        const int p = j / nq, q = j - p * nq;
        const int px = p & (PYR_TW - 1), py = p / PYR_TW;
        const int x = x0 + px, y = y0 + py;
        if (x >= W || y >= H) continue;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int ci = 0; ci < CH; ++ci) {
                    const float v = win[(py + ky) * WR + (px + kx) * CH + ci];
                    const f32x4 w4 = *reinterpret_cast<const f32x4*>(sw + ((ky * 3 + kx) * CH + ci) * cout + q * 4);
                    acc.x = fmaf(v, w4.x, acc.x); acc.y = fmaf(v, w4.y, acc.y); acc.z = fmaf(v, w4.z, acc.z); acc.w = fmaf(v, w4.w, acc.w);
                }
        float* o = t + ((size_t)y * W + x) * cout + q * 4;
        const f32x4 old = *reinterpret_cast<const f32x4*>(o);
        *reinterpret_cast<f32x4*>(o) = f32x4{old.x + acc.x, old.y + acc.y, old.z + acc.z, old.w + acc.w};
    }
}

// the pyramid of a page of C interleaved channels: PoolArgs as for avgpool2_c1_kernel, an item = one output pixel
template <int C>
__global__ __launch_bounds__(256) void avgpool2_cn_kernel(const PoolArgs a) {
    const int pi = prob_of_blk(a, (int)blockIdx.x);
    const PoolProb& P = a.p[pi];
    const int H = P.H, W = P.W, Wo = P.Wo;
    const size_t total = (size_t)P.Ho * Wo;
    const size_t base = (size_t)(blockIdx.x - P.blk_begin) * POOL_ITEMS;
    for (int k = 0; k < POOL_ITEMS / 256; ++k) {
        const size_t i = base + k * 256 + threadIdx.x;
        if (i >= total) break;
        const int x = (int)(i % Wo), y = (int)(i / Wo);
        const bool xin = 2 * x + 1 < W, yin = 2 * y + 1 < H;
        const float* __restrict__ r0 = P.in + ((size_t)(2 * y) * W + 2 * x) * C;
        const float* __restrict__ r1 = r0 + (size_t)W * C;     // read only when yin
        const float n = (float)((xin ? 2 : 1) * (yin ? 2 : 1));
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float s = r0[c];
            if (xin) s += r0[C + c];
            if (yin) { s += r1[c]; if (xin) s += r1[C + c]; }
            P.out[i * C + c] = s / n;
        }
    }
}

}  // namespace asep
