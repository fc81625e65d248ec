// Kernels of the segmentation net evaluation (include/asep_hip.h, "segmentation net evaluation" block): what the reference's
// article_separation/plot_net_output.py computes between `sess.run` and `cv2.imwrite`, on the probabilities where the net left them.
//
// seg_eval_kernel<C, THR>: ONE launch over the pages of a call, whatever their sizes.  The work units are blocks of SEG_UNIT pixels, the
// pages' unit lists one behind the other (SegProb::blk_begin), at most MAXP pages per launch.  A thread takes SEG_PIX = 4 consecutive pixels
// per step: 4 C floats, which start on a 16-byte boundary for every C when the page does, so the probabilities arrive in C 16-byte loads
// (a page is one flat list of H * W pixels here: a row that ends inside a thread's four pixels is nothing special).  The ground truth planes and
// the mask planes go through 4-byte words where the plane's address allows, else through bytes.
//
// Per pixel (plot_net_output.py:196-241): `unsure` counts the values with 0 < p < 1 BEFORE the threshold; THR turns the values into p > 0.6
// (float32 compare, as numpy compares a float32 array with a Python float); the arg max takes the FIRST maximum (numpy's tie rule: a NaN wins
// over every number, the first NaN over later ones); per class cl, `equal` counts the pixels where the one-hot arg max equals gt_cl / 255, i.e.
// (gt == 255 and arg max == cl) or (gt == 0 and arg max != cl) -- any other ground truth byte never matches; tp and the count of gt == 255
// give the host tp / fp / fn.  Masks: uint8(p * 255) by truncation (the engine's out_u8 rule), of the thresholded run 0 / 255.
//
// Counters: per thread 32-bit counts (at most 16 pixels), summed over the wave with shuffles and over the block's four waves in LDS, then one
// 64-bit atomic add per block and non-zero counter.  Integer sums: the result does not depend on the order of the blocks.
//
// Stream bound: 4 C bytes of probabilities + C bytes of ground truth in, up to C bytes of masks out per pixel; no reuse, no arithmetic to speak of.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "launch_plan.h"   // MAXP

namespace asep {

constexpr int SEG_MAXC = 8;                                   // classes served: seg_eval_kernel<1..8, .>
constexpr int SEG_BLOCK = 256;
constexpr int SEG_PIX = 4;                                    // consecutive pixels of a thread per step
constexpr int SEG_STEPS = 4;
constexpr int SEG_UNIT = SEG_BLOCK * SEG_PIX * SEG_STEPS;     // pixels of one block
// a page's counters in device memory: [0] unsure, [8 + c] class_count, [16 + c] equal, [24 + c] tp, [32 + c] pixels with gt_c == 255
constexpr int SEG_DEV_SLOTS = 40;
constexpr int SEG_D_UNSURE = 0, SEG_D_CLASS = 8, SEG_D_EQUAL = 16, SEG_D_TP = 24, SEG_D_GT = 32;

typedef float seg_f32x4 __attribute__((ext_vector_type(4)));

struct SegProb {
    const float* prob;                 // [npix, C]
    const uint8_t* gt[SEG_MAXC];       // C planes [npix], or all null
    uint8_t* masks;                    // planar [C][npix], or null
    unsigned long long* cnt;           // SEG_DEV_SLOTS counters, zeroed by the call
    long long npix;
    int blk_begin;                     // the page's first block of the launch
    int vec;                           // prob is 16-byte aligned
};
struct SegArgs {
    SegProb p[MAXP];
    int nprob;
};

__device__ __forceinline__ bool seg_word_aligned(const void* p) { return ((uintptr_t)p & 3) == 0; }

template <int C, bool THR>
__global__ __launch_bounds__(SEG_BLOCK) void seg_eval_kernel(const SegArgs a) {
    constexpr int NV = 1 + 4 * C;      // unsure, class_count[C], equal[C], tp[C], gt255[C]
    __shared__ uint32_t red[SEG_BLOCK / 64][NV];
    const int blk = (int)blockIdx.x;
    int pi = 0;
    for (int i = 1; i < MAXP; ++i)
        if (i < a.nprob && blk >= a.p[i].blk_begin) pi = i;
    const SegProb& P = a.p[pi];
    const long long npix = P.npix;
    const long long base = (long long)(blk - P.blk_begin) * SEG_UNIT;
    const bool has_gt = P.gt[0] != nullptr;
    uint32_t acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0;

#pragma unroll 1
    for (int s = 0; s < SEG_STEPS; ++s) {
        const long long p0 = base + ((long long)s * SEG_BLOCK + (int)threadIdx.x) * SEG_PIX;
        if (p0 >= npix) break;
        const int n = (npix - p0 < SEG_PIX) ? (int)(npix - p0) : SEG_PIX;
        const bool full = n == SEG_PIX;
        float v[SEG_PIX * C];
        if (full && P.vec) {
            const seg_f32x4* q = reinterpret_cast<const seg_f32x4*>(P.prob + p0 * C);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const seg_f32x4 t = q[k];
                v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SEG_PIX; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) v[j * C + c] = j < n ? P.prob[(p0 + j) * C + c] : 0.0f;
        }
        uint32_t g[C];                 // the four pixels' ground truth bytes of plane c, pixel j in byte j
        if (has_gt) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint8_t* q = P.gt[c] + p0;
                if (full && seg_word_aligned(q)) {
                    g[c] = *reinterpret_cast<const uint32_t*>(q);
                } else {
                    g[c] = 0;
#pragma unroll
                    for (int j = 0; j < SEG_PIX; ++j)
                        if (j < n) g[c] |= (uint32_t)q[j] << (8 * j);
                }
            }
        }
        uint32_t m[C];                 // the four pixels' mask bytes of plane c
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = 0;
#pragma unroll
        for (int j = 0; j < SEG_PIX; ++j) {
            if (j >= n) break;
            int am = 0;
            float best = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float x = v[j * C + c];
                acc[0] += (x > 0.0f && x < 1.0f) ? 1u : 0u;
                if (THR) x = x > 0.6f ? 1.0f : 0.0f;
                m[c] |= (THR ? (x != 0.0f ? 255u : 0u) : (uint32_t)(uint8_t)(x * 255.0f)) << (8 * j);
                if (c == 0) {
                    best = x;
                } else if (x > best || (x != x && best == best)) {
                    best = x, am = c;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool is = am == c;
                acc[1 + c] += is ? 1u : 0u;
                if (has_gt) {
                    const uint32_t b = (g[c] >> (8 * j)) & 255u;
                    acc[1 + C + c] += ((b == 255u && is) || (b == 0u && !is)) ? 1u : 0u;
                    acc[1 + 2 * C + c] += (b == 255u && is) ? 1u : 0u;
                    acc[1 + 3 * C + c] += (b == 255u) ? 1u : 0u;
                }
            }
        }
        if (P.masks) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                uint8_t* q = P.masks + (long long)c * npix + p0;
                if (full && seg_word_aligned(q)) {
                    *reinterpret_cast<uint32_t*>(q) = m[c];
                } else {
#pragma unroll
                    for (int j = 0; j < SEG_PIX; ++j)
                        if (j < n) q[j] = (uint8_t)(m[c] >> (8 * j));
                }
            }
        }
    }

    // wave sums, then the block's four waves in LDS, then one atomic add per counter
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        uint32_t x = acc[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) red[wave][i] = x;
    }
    __syncthreads();
    const int t = (int)threadIdx.x;
    if (t < NV) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < SEG_BLOCK / 64; ++w) sum += red[w][t];
        if (sum) {
            const int grp = t == 0 ? 0 : 1 + (t - 1) / C, c = t == 0 ? 0 : (t - 1) % C;   // grp 1..4 = class_count, equal, tp, gt255
            atomicAdd(P.cnt + (t == 0 ? SEG_D_UNSURE : 8 * grp + c), (unsigned long long)sum);
        }
    }
}

// apply_mask of plot_net_output.py:57-70 with its alpha 0.5: out = mask == 255 ? (scan + colour) / 2 rounded down : scan, per byte of the
// three channels.  (image * 0.5 + 0.5 * colour is exact in double; the assignment into the uint32 / uint8 image truncates.)  Four pixels =
// three words per thread where the three addresses allow; out may be scan.
struct SegBlendArgs {
    const uint8_t* scan;   // [npix, 3]
    const uint8_t* mask;   // [npix]
    uint8_t* out;          // [npix, 3]
    long long npix;
    uint32_t col[3];
};

__global__ __launch_bounds__(SEG_BLOCK) void seg_blend_kernel(const SegBlendArgs a) {
    const long long p0 = ((long long)blockIdx.x * SEG_BLOCK + (int)threadIdx.x) * SEG_PIX;
    if (p0 >= a.npix) return;
    const int n = (a.npix - p0 < SEG_PIX) ? (int)(a.npix - p0) : SEG_PIX;
    const uint8_t* s = a.scan + 3 * p0;
    const uint8_t* mk = a.mask + p0;
    uint8_t* o = a.out + 3 * p0;
    if (n == SEG_PIX && seg_word_aligned(s) && seg_word_aligned(mk) && seg_word_aligned(o)) {
        const uint32_t mw = *reinterpret_cast<const uint32_t*>(mk);
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const uint32_t*>(s)[k];
        uint32_t r[3] = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < 12; ++i) {                     // byte i of the twelve: pixel i / 3, channel i % 3
            const uint32_t b = (w[i / 4] >> (8 * (i % 4))) & 255u;
            const bool on = ((mw >> (8 * (i / 3))) & 255u) == 255u;
            r[i / 4] |= (on ? (b + a.col[i % 3]) >> 1 : b) << (8 * (i % 4));
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(o)[k] = r[k];
    } else {
        for (int j = 0; j < n; ++j) {
            const bool on = mk[j] == 255;
            for (int c = 0; c < 3; ++c) {
                const uint32_t b = s[3 * j + c];
                o[3 * j + c] = (uint8_t)(on ? (b + a.col[c]) >> 1 : b);
            }
        }
    }
}

}  // namespace asep
