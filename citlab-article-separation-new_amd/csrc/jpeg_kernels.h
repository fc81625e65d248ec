// Device half of the JPEG decode (include/asep_hip.h, "JPEG pixels" block): quantised coefficients -> pixels, integer throughout, equal
// to libjpeg-turbo's defaults bit for bit (tests/jpeg_ref.py is the same arithmetic in numpy):
//   jpeg_idct_kernel    dequantise + the accurate integer inverse DCT (jidctint.c: 13-bit constants, 2 extra bits after the column pass,
//                       descaled with rounding, + 128, clamped) of every block of every component; one thread per block, the block in
//                       registers, eight 16-byte loads in, eight 8-byte stores out.  A one-component page is written straight into the
//                       cropped output, a colour page into padded component planes.
//   jpeg_colour_kernel  "fancy" chroma upsampling (jdsample.c: h2v1 3:1 triangle with alternating rounding, h2v2 3:1 rows then columns
//                       with the + 8 / + 7 biases; replication when the downsampled width is <= 2) over the REAL downsampled size, then
//                       YCbCr -> RGB in 16-bit fixed point (jdcolor.c), written interleaved and cropped; four pixels per thread.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace asep {

constexpr int JPEG_IDCT_BLOCK = 64;      // threads (= 8x8 blocks) per workgroup of jpeg_idct_kernel
constexpr int JPEG_COLOUR_BLOCK = 256;   // threads per workgroup of jpeg_colour_kernel
constexpr int JPEG_COLOUR_PIX = 4;       // pixels of one row per thread

struct JpegIdctComp {
    const int16_t* coef;                 // [blocks_h][blocks_w][64]
    uint8_t* out;                        // plane (or the cropped gray page)
    long long stride;                    // bytes between rows of out
    int blocks_w;
    int crop_w, crop_h;                  // pixels of out that exist
    int first;                           // number of this component's first block in the launch
    int qt;                              // its table
};

struct JpegIdctArgs {
    JpegIdctComp c[3];
    int ncomp;
    int total;                           // blocks of all components
    uint16_t qt[4][64];                  // natural order
};

struct JpegColourArgs {
    const uint8_t* y;
    const uint8_t* cb;
    const uint8_t* cr;
    uint8_t* out;                        // [H][W][3] or, for order gray, [H][W]
    int y_stride, c_stride;
    int W, H;
    int dw, dh;                          // real downsampled size: ceil(W / hs), ceil(H / vs)
    int hs, vs;
    int order;                           // ASEP_JPEG_ORDER_*
    int groups_w;                        // threads per row: ceil(W / JPEG_COLOUR_PIX)
};

// one 1-D pass of jidctint.c over v[0..7]; SHIFT = 11 after the column pass, 18 after the row pass
template <int SHIFT>
__device__ __forceinline__ void jpeg_idct_1d(int (&v)[8]) {
    constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
    constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
    constexpr int RND = 1 << (SHIFT - 1);
    int z2 = v[2], z3 = v[6];
    int z1 = (z2 + z3) * F_0_541;
    int tmp2 = z1 - z3 * F_1_847;
    int tmp3 = z1 + z2 * F_0_765;
    int tmp0 = (v[0] + v[4]) * (1 << 13);
    int tmp1 = (v[0] - v[4]) * (1 << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7], tmp1 = v[5], tmp2 = v[3], tmp3 = v[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175;
    tmp0 *= F_0_298, tmp1 *= F_2_053, tmp2 *= F_3_072, tmp3 *= F_1_501;
    z1 *= -F_0_899, z2 *= -F_2_562;
    z3 = z3 * -F_1_961 + z5, z4 = z4 * -F_0_390 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    v[0] = (tmp10 + tmp3 + RND) >> SHIFT;
    v[7] = (tmp10 - tmp3 + RND) >> SHIFT;
    v[1] = (tmp11 + tmp2 + RND) >> SHIFT;
    v[6] = (tmp11 - tmp2 + RND) >> SHIFT;
    v[2] = (tmp12 + tmp1 + RND) >> SHIFT;
    v[5] = (tmp12 - tmp1 + RND) >> SHIFT;
    v[3] = (tmp13 + tmp0 + RND) >> SHIFT;
    v[4] = (tmp13 - tmp0 + RND) >> SHIFT;
}

__device__ __forceinline__ int jpeg_clamp255(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

__global__ __launch_bounds__(JPEG_IDCT_BLOCK) void jpeg_idct_kernel(const JpegIdctArgs a) {
    const int g = (int)(blockIdx.x * JPEG_IDCT_BLOCK + threadIdx.x);
    if (g >= a.total) return;
    const int ci = (a.ncomp > 2 && g >= a.c[2].first) ? 2 : ((a.ncomp > 1 && g >= a.c[1].first) ? 1 : 0);
    const JpegIdctComp& c = a.c[ci];
    const int b = g - c.first;
    const int by = b / c.blocks_w, bx = b - by * c.blocks_w;
    const uint16_t* q = a.qt[c.qt];
    const uint4* src = reinterpret_cast<const uint4*>(c.coef + (size_t)b * 64);      // a block is 128 bytes, 16-byte aligned
    int m[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 w = src[r];
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[r][2 * k] = (int)(int16_t)(u[k] & 0xffffu) * (int)q[r * 8 + 2 * k];
            m[r][2 * k + 1] = (int)(int16_t)(u[k] >> 16) * (int)q[r * 8 + 2 * k + 1];
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {                              // pass 1: columns
        int v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = m[r][col];
        jpeg_idct_1d<11>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) m[r][col] = v[r];
    }
    const int x0 = bx * 8, y0 = by * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                                    // pass 2: rows
        jpeg_idct_1d<18>(m[r]);
        const int y = y0 + r;
        if (y >= c.crop_h) continue;
        uint8_t px[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) px[k] = (uint8_t)jpeg_clamp255(m[r][k] + 128);
        uint8_t* dst = c.out + (size_t)y * (size_t)c.stride + x0;
        if (x0 + 8 <= c.crop_w && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
            uint2 w;
            w.x = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
            w.y = (uint32_t)px[4] | ((uint32_t)px[5] << 8) | ((uint32_t)px[6] << 16) | ((uint32_t)px[7] << 24);
            *reinterpret_cast<uint2*>(dst) = w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (x0 + k < c.crop_w) dst[k] = px[k];
        }
    }
}

// the upsampled chroma sample of output pixel (x, y)
__device__ __forceinline__ int jpeg_chroma_at(const uint8_t* p, int stride, int x, int y, const JpegColourArgs& a) {
    if (a.hs == 1) return p[(size_t)y * stride + x];
    const int cx = x >> 1;
    if (a.vs == 1) {
        const uint8_t* row = p + (size_t)y * stride;
        if (a.dw <= 2) return row[cx];
        const int here = row[cx];
        if (x & 1) return (3 * here + row[min(cx + 1, a.dw - 1)] + 2) >> 2;
        return (3 * here + row[max(cx - 1, 0)] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* near = p + (size_t)cy * stride;
    if (a.dw <= 2) return near[cx];
    const uint8_t* far = p + (size_t)((y & 1) ? min(cy + 1, a.dh - 1) : max(cy - 1, 0)) * stride;
    const int here = 3 * near[cx] + far[cx];
    if (x & 1) {
        const int n = min(cx + 1, a.dw - 1);
        return (3 * here + 3 * near[n] + far[n] + 7) >> 4;
    }
    const int n = max(cx - 1, 0);
    return (3 * here + 3 * near[n] + far[n] + 8) >> 4;
}

__global__ __launch_bounds__(JPEG_COLOUR_BLOCK) void jpeg_colour_kernel(const JpegColourArgs a) {
    const long long g = (long long)blockIdx.x * JPEG_COLOUR_BLOCK + threadIdx.x;
    if (g >= (long long)a.groups_w * a.H) return;
    const int y = (int)(g / a.groups_w);
    const int x0 = (int)(g - (long long)y * a.groups_w) * JPEG_COLOUR_PIX;
    const int n = min(JPEG_COLOUR_PIX, a.W - x0);
    const int nch = a.order == ASEP_JPEG_ORDER_GRAY ? 1 : 3;
    uint8_t v[JPEG_COLOUR_PIX * 3];
#pragma unroll
    for (int k = 0; k < JPEG_COLOUR_PIX; ++k) {
        if (k >= n) {
            v[3 * k] = v[3 * k + 1] = v[3 * k + 2] = 0;
            continue;
        }
        const int x = x0 + k;
        const int Y = a.y[(size_t)y * a.y_stride + x];
        const int cb = jpeg_chroma_at(a.cb, a.c_stride, x, y, a) - 128;
        const int cr = jpeg_chroma_at(a.cr, a.c_stride, x, y, a) - 128;
        const int r = jpeg_clamp255(Y + ((91881 * cr + 32768) >> 16));
        const int gg = jpeg_clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
        const int b = jpeg_clamp255(Y + ((116130 * cb + 32768) >> 16));
        if (a.order == ASEP_JPEG_ORDER_GRAY) {
            v[k] = (uint8_t)((b * 3735 + gg * 19235 + r * 9798 + 16384) >> 15);     // the BGR2GRAY weights of load_image_gray
        } else if (a.order == ASEP_JPEG_ORDER_BGR) {
            v[3 * k] = (uint8_t)b, v[3 * k + 1] = (uint8_t)gg, v[3 * k + 2] = (uint8_t)r;
        } else {
            v[3 * k] = (uint8_t)r, v[3 * k + 1] = (uint8_t)gg, v[3 * k + 2] = (uint8_t)b;
        }
    }
    uint8_t* dst = a.out + ((size_t)y * a.W + x0) * nch;
    if (n == JPEG_COLOUR_PIX && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < nch)
                d32[k] = (uint32_t)v[4 * k] | ((uint32_t)v[4 * k + 1] << 8) | ((uint32_t)v[4 * k + 2] << 16) | ((uint32_t)v[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < n * nch; ++k) dst[k] = v[k];
    }
}

}  // namespace asep
