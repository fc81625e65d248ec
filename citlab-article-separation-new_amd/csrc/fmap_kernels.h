// Generated feature maps of the relation net's visual branch (feature_map_generators.py:72-197 with insert_1x1_conv, as
// graph_relation.py:100-104 calls it): a map that is not a backbone end point is
//     1x1 conv + bias + ReLU to d/2 channels  ->  3x3 SAME conv + bias + ReLU to d channels, stride 1 (from_layer named) or 2 (from_layer '')
// over an NHWC map [fh, fw, C]: a backbone end point (fp32, or bf16 from a bf16 backbone) or the previous generated map (fp32).
//
// Two launches per map, one thread per output value (pixel-major, channel fastest): neighbouring lanes read neighbouring filter
// columns (coalesced) and the same input value (one broadcast load).  No tile and no vector width enters the index arithmetic, so
// every channel count is the same path -- d/2 = 1, 3 (d = 2, 6) included -- and there are no tails.  Operands and accumulation are fp32,
// the order of one output's sum is fixed: the bias, then the taps row-major (ky, kx), within a tap the input channels ascending.
// DESIGN.md section 4.3 says why this plain form was built first and what the fused form would be.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "launch_plan.h"

namespace asep {

struct FmapConvArgs {
    const void* in;           // [ih, iw, Ci] NHWC: fp32, or bf16 (2 bytes per value) for the <true> instantiation of the 1x1 kernel
    const float* W;           // [k, k, Ci, Co] as the reference stores it (layers.py:220)
    const float* b;           // [Co]
    float* out;               // [oh, ow, Co] fp32
    int ih, iw, Ci, Co;
    int oh, ow;
    int stride;               // 3x3 only: 1 or 2
    int pad_t, pad_l;         // 3x3 only: TensorFlow's SAME -- total = max((o - 1) * stride + 3 - i, 0), the smaller half in front
};

// out[p][m] = relu(b[m] + sum_c in[p][c] W[c][m])
template <bool BF>
__device__ __forceinline__ void fmap_conv1x1_body(const FmapConvArgs& a, const unsigned blk) {
    const size_t total = (size_t)a.ih * a.iw * a.Co;
    const size_t i = (size_t)blk * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t p = i / a.Co;
    const int m = (int)(i - p * a.Co);
    float acc = a.b[m];
    const float* w = a.W + m;
    if constexpr (BF) {
        const unsigned short* x = reinterpret_cast<const unsigned short*>(a.in) + p * a.Ci;
        for (int c = 0; c < a.Ci; ++c) acc = fmaf(__uint_as_float((unsigned)x[c] << 16), w[(size_t)c * a.Co], acc);
    } else {
        const float* x = reinterpret_cast<const float*>(a.in) + p * a.Ci;
        for (int c = 0; c < a.Ci; ++c) acc = fmaf(x[c], w[(size_t)c * a.Co], acc);
    }
    a.out[i] = fmaxf(acc, 0.f);
}

template <bool BF>
__global__ void __launch_bounds__(256) fmap_conv1x1_kernel(const FmapConvArgs a) { fmap_conv1x1_body<BF>(a, blockIdx.x); }

// out[oy][ox][m] = relu(b[m] + sum_{ky,kx,c} in[oy s - pad_t + ky][ox s - pad_l + kx][c] W[ky][kx][c][m]), taps outside the map are zeros
__device__ __forceinline__ void fmap_conv3x3_body(const FmapConvArgs& a, const unsigned blk) {
    const size_t total = (size_t)a.oh * a.ow * a.Co;
    const size_t i = (size_t)blk * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t p = i / a.Co;
    const int m = (int)(i - p * a.Co);
    const int oy = (int)(p / a.ow), ox = (int)(p - (size_t)oy * a.ow);
    const float* in = reinterpret_cast<const float*>(a.in);
    float acc = a.b[m];
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * a.stride - a.pad_t + ky;
        if (iy < 0 || iy >= a.ih) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * a.stride - a.pad_l + kx;
            if (ix < 0 || ix >= a.iw) continue;
            const float* x = in + ((size_t)iy * a.iw + ix) * a.Ci;
            const float* w = a.W + (size_t)(ky * 3 + kx) * a.Ci * a.Co + m;
            for (int c = 0; c < a.Ci; ++c) acc = fmaf(x[c], w[(size_t)c * a.Co], acc);
        }
    }
    a.out[i] = fmaxf(acc, 0.f);
}
__global__ void __launch_bounds__(256) fmap_conv3x3_kernel(const FmapConvArgs a) { fmap_conv3x3_body(a, blockIdx.x); }

// ---- the same two convolutions over the pages of a batch call in ONE launch each, the pages' maps of any sizes: a page table in device memory
//      (launch_plan.h: page b owns the blocks begin[b] .. begin[b + 1] - 1 of 256 outputs each).  A block looks its page up and runs the body
//      above on that page's map with its own block number: the same sum, in the same order, per output value ----
struct FmapPage {
    const void* in;           // this page's input map
    float* out;               // and its output
    int ih, iw, oh, ow;
    int pad_t, pad_l;         // 3x3 only
};
struct FmapPagesArgs {
    const FmapPage* pages;    // [n_pages], device memory
    const int32_t* begin;     // [n_pages + 1], device memory
    int n_pages;
    const float* W;
    const float* b;
    int Ci, Co, stride;
};
__device__ __forceinline__ FmapConvArgs fmap_page_args(const FmapPagesArgs& t, const int pg) {
    const FmapPage q = t.pages[pg];
    FmapConvArgs a;
    a.in = q.in; a.W = t.W; a.b = t.b; a.out = q.out;
    a.ih = q.ih; a.iw = q.iw; a.Ci = t.Ci; a.Co = t.Co; a.oh = q.oh; a.ow = q.ow;
    a.stride = t.stride; a.pad_t = q.pad_t; a.pad_l = q.pad_l;
    return a;
}
template <bool BF>
__global__ void __launch_bounds__(256) fmap_conv1x1_pages_kernel(const FmapPagesArgs t) {
    const int pg = page_of_unit(t.begin, t.n_pages, (int)blockIdx.x);
    fmap_conv1x1_body<BF>(fmap_page_args(t, pg), blockIdx.x - (unsigned)t.begin[pg]);
}
__global__ void __launch_bounds__(256) fmap_conv3x3_pages_kernel(const FmapPagesArgs t) {
    const int pg = page_of_unit(t.begin, t.n_pages, (int)blockIdx.x);
    fmap_conv3x3_body(fmap_page_args(t, pg), blockIdx.x - (unsigned)t.begin[pg]);
}

}  // namespace asep
