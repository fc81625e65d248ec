// res8ws_kernel: the level-0 residual blocks of the f32s engine (compute_dtype 2, ReLU graph) as column-strip walkers on SPLIT PRODUCTS.
//
// The strip geometry, the pixel-pair MFMA mapping, the stage schedule and the ring addressing are those of res8w_kernel (res8w_kernels.h):
// one wave walks down a strip of 24 output columns, two rows per iteration, and iteration k runs conv1 on rows 2 k + 1, 2 k + 2 of its
// item, stage 1 three rows behind it, stage 2 three behind stage 1, stage 3 three behind stage 2, out of rolling LDS rings that no other
// wave reads: no barrier, no vertical halo recomputed, a horizontal one of 1.17 x.  What changes is the arithmetic (split_kernels.h):
//   * every fp32 operand is the exact sum of three bfloat16 parts; a product group is six v_mfma_f32_16x16x32_bf16 in the order of the
//     other split kernels (smallest terms first: wl xh, wh xl, wm xm, wm xh, wh xm, wh xh), accumulated in fp32;
//   * the filters are split once on the host; the fragments of all three parts of every filter the wave uses are loaded once per item
//     into the accumulator half of the register file (UP: 45 fragments = 180 AGPRs, DOWN: 27), the MFMAs take them from there;
//   * every intermediate stage is stored as its three part planes, split ONCE in the producing epilogue (after the ReLU, on fp32);
//   * UP: the raw conv1 result t stays fp32 (a ring of 16 rows x 24 pixels x 32 bytes) and is added in the stage-3 epilogue, then the ReLU;
//     DOWN: no t ring.  The stage-3 epilogue computes t again for its two rows out of the image ring, with the instruction sequence of the
//     conv1 stage (72 FMAs a pixel against about 1800 split products in the tail), so the sum t + conv is bit for bit what a t ring gave;
//   * UP conv1 (16 -> 8 over [skip, deconv]) reads its fp32 input rows straight from global memory one iteration ahead (the lane's window
//     pixel, two rows per iteration and source), splits them once and carries the two lower rows to the next iteration in registers;
//   * DOWN conv1 (1 -> 8) stays on fp32 FMAs in res8v_down_kernel's order (bias, taps ky-major): t is bit-identical to res8v's; the image
//     rows pass through a sixteen-row fp32 ring (the depth: at NI in the kernel), standardised like res8v;
//   * the DOWN block's 2 x 2 max pool runs on the fp32 stage-3 results (rows inside the lane, the pixel pair across lane ^ 32).
// LDS per wave (bytes): stage rings of 4 rows x 3 parts x 30 / 28 / 26 pixels x 16 = 5760 + 5376 + 4992, a 16-byte dump, UP: + raw t 12288
// = 28432 (27.8 KB); DOWN: + the image ring 16 x 32 x 4 = 2048 = 18192 (17.8 KB).  Registers (compiler's resource report): UP 234 VGPRs + 196
// AGPRs (filters), one wave per SIMD = four per CU; DOWN 98 VGPRs + 128 AGPRs, no scratch, two waves per SIMD = eight per CU, which the LDS now
// holds as well (8 x 17.8 KB of 160 KB; with the t ring it was 28.9 KB a wave and five waves per CU).
//
// The walker covers columns [32, 32 + 24 n) x rows [16, y_end) of a page like res8w_kernel.  The frame around it is computed by the
// vector-ALU kernels (res8v_*_kernel) over the work units that touch it, launched BEFORE the walker: the walker then overwrites the part
// of those units that lies in its region, so every pixel has one writer at the end and the seam needs no special case.
#pragma once
#include "res8w_kernels.h"
#include "split_kernels.h"

namespace asep {

struct Res8WSProb {
    const float* skip;     // UP: [H,W,8]
    const float* dec;      // UP: [H,W,8] deconv output
    const float* img;      // DOWN: [H,W] image (pyramid level)
    const float* stats;    // DOWN: {mean, 1/std} or nullptr
    float* out;            // [H,W,8]
    float* pool;           // DOWN: maxpool2(out) [ceil(H/2), ceil(W/2), 8] or nullptr
    int H, W;
    int n_strips;          // strips at x0 = 32 + 24 s
    int band;              // output rows of an item (even)
    int y_end;             // the walker's rows end here (even, <= H - 4)
    int tile_begin;        // first item of this problem in the launch (band-major, the strips of a band side by side)
};
struct Res8WSArgs {
    Res8WSProb p[MAXP];
    int nprob;
    const float* b1;       // conv1 bias [8]
    const u32x4* w1s;      // UP: conv1 split pair fragments [ky 3][source 2][part 3][64 lanes] x 16 bytes
    const float* w1f;      // DOWN: conv1 fp32 [9 taps][8]
    const u32x4* ws;       // tail: [3 convs][ky 3][part 3][64 lanes] x 16 bytes
    const float* bias;     // tail biases [3][8]
    XcdMap xm;
};

// one split product group of the pair-window mapping for tiles A and B, interleaved: c += w * x over the six largest part products
__device__ __forceinline__ void r8ws_mm6(const u32x4 (&w)[3], const u32x4 (&xa)[3], const u32x4 (&xb)[3], f32x4& ca, f32x4& cb) {
    ca = mfma_bf16_k32(w[2], xa[0], ca); cb = mfma_bf16_k32(w[2], xb[0], cb);
    ca = mfma_bf16_k32(w[0], xa[2], ca); cb = mfma_bf16_k32(w[0], xb[2], cb);
    ca = mfma_bf16_k32(w[1], xa[1], ca); cb = mfma_bf16_k32(w[1], xb[1], cb);
    ca = mfma_bf16_k32(w[1], xa[0], ca); cb = mfma_bf16_k32(w[1], xb[0], cb);
    ca = mfma_bf16_k32(w[0], xa[1], ca); cb = mfma_bf16_k32(w[0], xb[1], cb);
    ca = mfma_bf16_k32(w[0], xa[0], ca); cb = mfma_bf16_k32(w[0], xb[0], cb);
}
// four packed words {v.x, v.y}, {v.z, v.w} -> their three parts
__device__ __forceinline__ void r8ws_split4(f32x4 v, u32x2& h, u32x2& m, u32x2& l) {
    unsigned h0, m0, l0, h1, m1, l1;
    split3_pair(v.x, v.y, h0, m0, l0);
    split3_pair(v.z, v.w, h1, m1, l1);
    h = u32x2{h0, h1}; m = u32x2{m0, m1}; l = u32x2{l0, l1};
}

// waves (one-wave blocks) of an instance that a CU holds, for the launcher's band plan: UP one per SIMD by registers, DOWN two per SIMD by
// registers and LDS
constexpr int R8WS_UP_WAVES_PER_CU = 4, R8WS_DOWN_WAVES_PER_CU = 8;

template <bool UP>
__global__ __launch_bounds__(64, 1) void res8ws_kernel(const Res8WSArgs a) {
    constexpr int TW = R8W_TW;
    constexpr int W0 = TW + 6, W1 = TW + 4, W2 = TW + 2;                      // 30, 28, 26 pixels
    constexpr int NR = 4, NT = 16;                                             // stage ring rows, raw t rows (UP)
    // DOWN: rows of the image ring.  Iteration k's stage 3 finishes item rows 2 k - 8, 2 k - 7 (row r = image row Ya - 4 + r) and recomputes
    // their t from the 3 x 3 windows around them, item rows 2 k - 9 .. 2 k - 6; conv1 of the same iteration stores pair k + 1, item rows
    // 2 k + 2, 2 k + 3.  So rows 2 k - 9 .. 2 k + 3 are live, whole pairs 2 k - 10 .. 2 k + 3: 14 rows.  16 = the next power of two, so
    // that a row's place is its number under a mask like the stage rings' (256 bytes more; eight waves fit per CU either way).
    constexpr int NI = 16;
    constexpr int PL0 = W0 * 16, PL1 = W1 * 16, PL2 = W2 * 16;                 // bytes of one part plane of a ring row
    // the region behind the stage rings: UP raw t, DOWN the image ring of NI rows x 32 fp32
    constexpr int R0_OFF = 0, R1_OFF = R0_OFF + NR * 3 * PL0, R2_OFF = R1_OFF + NR * 3 * PL1, TC_OFF = R2_OFF + NR * 3 * PL2, IM_OFF = TC_OFF,
                  TRASH = TC_OFF + (UP ? NT * TW * 32 : NI * 32 * 4), LDSB = TRASH + 16;
    // (a fragment read of lanes j >= the tile's pairs takes units up to 33 of its row, 8 pixels past an r2 row: into the next plane, row or
    //  region, never past the region behind the stage rings)
    static_assert(TRASH - TC_OFF >= (34 - W2) * 16, "the fragment reads of the last r2 plane stay inside the array");
    static_assert(UP ? LDSB <= 30 * 1024 : LDSB <= 20 * 1024, "UP: four waves per CU with room to spare; DOWN: eight");
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDSB];

    const int lane = threadIdx.x;
    const int j = lane & 15, kk = lane >> 4, e = kk >> 1, ch = (kk & 1) * 4;   // D layout: pixel parity e, channels ch .. ch + 3
    const int isB = kk & 1;
    const int c = 2 * j + e;                                                  // the lane's pixel column in a tile
    const int item = sched_tile(a.xm);
    if (item < 0) return;
    const int pi = prob_of_tile(a, item);
    const Res8WSProb& P = a.p[pi];
    const int li = item - P.tile_begin;
    const int bi = li / P.n_strips, si = li - bi * P.n_strips;
    const int x0 = R8W_X0 + TW * si;
    const int Ya = R8W_Y0 + bi * P.band;
    const int nb = min(P.band, P.y_end - Ya);                                 // output rows of this item (even)
    const int W = P.W;

    // ---- filters: the three parts of every fragment in AGPRs for the whole item (see convr_kernel: a value the compiler defines lives in a
    //      VGPR first and is copied back in front of every use once the file is full) ----
    constexpr int NF1 = UP ? 18 : 0, NFW = 27;
    u32x4 wf[NFW], w1[UP ? NF1 : 1];
    {
        const u32x4* wl = a.ws + lane;
#pragma unroll
        for (int i = 0; i < NFW; ++i) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(wf[i]) : "v"(wl + i * 64) : "memory");
        if constexpr (UP) {
            const u32x4* w1l = a.w1s + lane;
#pragma unroll
            for (int i = 0; i < NF1; ++i) asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(w1[i]) : "v"(w1l + i * 64) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < NFW; ++i) asm volatile("" : "+a"(wf[i]));
        if constexpr (UP) {
#pragma unroll
            for (int i = 0; i < NF1; ++i) asm volatile("" : "+a"(w1[i]));
        }
    }
    auto wpart = [&](int s, int ky, u32x4 (&o)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p) o[p] = wf[(s * 3 + ky) * 3 + p];
    };
    const f32x4 bias1 = *reinterpret_cast<const f32x4*>(a.b1 + ch);
    f32x4 biasw[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) biasw[t] = *reinterpret_cast<const f32x4*>(a.bias + 8 * t + ch);

    // ---- inputs ----
    // UP: lane (j, kk) reads window pixel kk of pair j = column x0 - 4 + 2 j + kk (clamped: lanes of the unused pairs 15 read the last column)
    const int gxw = min(x0 - 4 + 2 * j + kk, W - 1);
    const float* __restrict__ skp = P.skip;
    const float* __restrict__ dcp = P.dec;
    auto in_row = [&](const float* __restrict__ src, int gy, f32x4& lo, f32x4& hi) {
        const float* q = src + ((size_t)gy * (size_t)W + (size_t)gxw) * 8;
        lo = *reinterpret_cast<const f32x4*>(q);
        hi = *reinterpret_cast<const f32x4*>(q + 4);
    };
    // DOWN: a pair of image rows = 64 fp32 = one per lane (row lane >> 5, column x0 - 4 + (lane & 31)); the ring holds item rows mod NI
    float mean = 0.f, inv = 1.f;
    if constexpr (!UP) {
        if (P.stats) { mean = P.stats[0]; inv = P.stats[1]; }
    }
    const float* __restrict__ imp = P.img;
    const size_t ioff0 = (size_t)(Ya - 4 + (lane >> 5)) * (size_t)W + (size_t)(x0 - 4 + (lane & 31));
    auto iload = [&](int p) { return imp[ioff0 + (size_t)p * 2 * (size_t)W]; };
    float* const iring = reinterpret_cast<float*>(lds + IM_OFF);
    auto istore = [&](float v, int p) { iring[((2 * p) & (NI - 1)) * 32 + lane] = (v - mean) * inv; };   // pair p -> ring rows 2 p, 2 p + 1 (mod NI)
    float w1v[UP ? 1 : 36];
    if constexpr (!UP) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int o = 0; o < 4; ++o) w1v[t * 4 + o] = a.w1f[t * 8 + ch + o];
    }
    // conv1 of the lane's four channels at ring column cb (+ kx) of item rows r0, r0 + 1 (window rows r0 - 1 .. r0 + 2), in
    // res8v_down_kernel's order (bias, taps ky-major).  The conv1 stage and the stage-3 epilogue both call it: the same instruction sequence
    // on the same ring values, so the t that stage 3 adds is bit for bit the t whose ReLU went into the stage rings.
    auto conv1_down = [&](int r0, int cb, f32x4& ra, f32x4& rb) {
        if constexpr (!UP)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float va = iring[((r0 - 1 + ky) & (NI - 1)) * 32 + cb + kx], vb = iring[((r0 + ky) & (NI - 1)) * 32 + cb + kx];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    ra[o] = fmaf(va, w1v[(ky * 3 + kx) * 4 + o], ra[o]);
                    rb[o] = fmaf(vb, w1v[(ky * 3 + kx) * 4 + o], rb[o]);
                }
            }
    };

    const int p_last = nb / 2 + 3;                                            // input pairs 0 .. p_last: rows Ya - 4 .. Ya + nb + 3
    u32x4 cin[2][2][3] = {};                                                  // UP: split rows 0, 1 of conv1's window [row][source][part]
    f32x4 nxt[2][2][2];                                                       // UP: fp32 rows of the next pair [row][source][half]
    float inx = 0.f;                                                          // DOWN: the next pair's image values
    if constexpr (UP) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            f32x4 lo, hi;
            in_row(skp, Ya - 4 + r, lo, hi);
            split3_x8(lo, hi, cin[r][0][0], cin[r][0][1], cin[r][0][2]);
            in_row(dcp, Ya - 4 + r, lo, hi);
            split3_x8(lo, hi, cin[r][1][0], cin[r][1][1], cin[r][1][2]);
            in_row(skp, Ya - 2 + r, nxt[r][0][0], nxt[r][0][1]);
            in_row(dcp, Ya - 2 + r, nxt[r][1][0], nxt[r][1][1]);
        }
    } else {
        istore(iload(0), 0);
        inx = iload(1);
    }

    const int lcol = r8w_swz(2 * j + kk) * 16;               // the lane's window pixel in a ring row
    auto whole = [&](u32x2 pa, u32x2 pb) {                   // lanes kk = 0 / 2 end with the whole pixel of tile A, kk = 1 / 3 with that of tile B
        const auto s0 = __builtin_amdgcn_permlane16_swap(pa.x, pb.x, false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(pa.y, pb.y, false, false);
        return u32x4{s0[0], s1[0], s0[1], s1[1]};
    };
    const int cs = r8w_swz(c) * 16;
    const bool v0 = j < W0 / 2, v1 = j < W1 / 2, v2 = j < W2 / 2;
    const bool tvalid = c >= 3 && c < 3 + TW;
    const int tcol = (tvalid ? c - 3 : 0) * 32 + ch * 4;     // UP: conv1's lane writes its half of raw t at pixel c - 3
    const int trd = min(c, TW - 1) * 32 + ch * 4;            // UP: stage 3 reads it at its output pixel c
    const int tcb = min(c, TW - 1) + 3;                      // DOWN: stage 3 recomputes it at conv1's pixel c + 3 (ring columns tcb .. tcb + 2 <= 28)
    const bool ost = j < TW / 2;
    float* __restrict__ const outp = P.out;
    float* __restrict__ const poolp = P.pool;
    const size_t Wp = (size_t)((W + 1) >> 1);

    // the epilogue of stages 0 .. 2: ReLU, the three parts, whole pixels, three 16-byte stores per lane into ring rows rtop, rtop + 1
    auto store_parts = [&](f32x4 ra, f32x4 rb, int roff, int pl, bool valid, int rowa, int rowb) {
        u32x2 ha, ma, la, hb, mb, lb;
        r8ws_split4(relu4i(ra), ha, ma, la);
        r8ws_split4(relu4i(rb), hb, mb, lb);
        const u32x4 ph = whole(ha, hb), pm = whole(ma, mb), pl_ = whole(la, lb);
        const int rr = isB ? rowb : rowa;
        const int base = valid ? roff + rr * 3 * pl + cs : TRASH;
        const int step = valid ? pl : 0;
        *reinterpret_cast<u32x4*>(lds + base) = ph;
        *reinterpret_cast<u32x4*>(lds + base + step) = pm;
        *reinterpret_cast<u32x4*>(lds + base + 2 * step) = pl_;
    };
    auto ring_read = [&](int roff, int pl, int rr, u32x4 (&o)[3]) {
#pragma unroll
        for (int p = 0; p < 3; ++p) o[p] = *reinterpret_cast<const u32x4*>(lds + roff + (rr * 3 + p) * pl + lcol);
    };

    const int K = nb / 2 + 6;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const int i4 = (2 * k) & (NR - 1), i16 = (2 * k) & (NT - 1);
        const bool do_c1 = k < nb / 2 + 3, do_s1 = k >= 2 && k < nb / 2 + 4, do_s2 = k >= 4 && k < nb / 2 + 5, do_s3 = k >= 6;

        // ---- stage 3: output rows Ya - 12 + 2 k, + 1 = conv of r2 rows i4 - 9 .. i4 - 6, + raw t (DOWN: recomputed), ReLU; DOWN: the 2 x 2 pool ----
        if (do_s3) {
            u32x4 q[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) ring_read(R2_OFF, PL2, (i4 + r - 9) & (NR - 1), q[r]);
            f32x4 t0 = bias1, t1 = bias1;
            if constexpr (UP) {
                t0 = *reinterpret_cast<const f32x4*>(lds + TC_OFF + ((i16 - 8) & (NT - 1)) * TW * 32 + trd);
                t1 = *reinterpret_cast<const f32x4*>(lds + TC_OFF + ((i16 - 7) & (NT - 1)) * TW * 32 + trd);
            } else {
                conv1_down(2 * k - 8, tcb, t0, t1);          // item rows 2 k - 8, 2 k - 7, conv1's pixel c + 3
            }
            f32x4 va = biasw[2], vb = biasw[2];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                u32x4 w[3];
                wpart(2, ky, w);
                r8ws_mm6(w, q[ky], q[ky + 1], va, vb);
            }
            va = relu4i(va + t0);
            vb = relu4i(vb + t1);
            const int oy = Ya - 12 + 2 * k;
            if (ost) {
                float* o = outp + ((size_t)oy * (size_t)W + (size_t)(x0 + c)) * 8 + ch;
                *reinterpret_cast<f32x4*>(o) = va;
                *reinterpret_cast<f32x4*>(o + (size_t)W * 8) = vb;
            }
            if constexpr (!UP) {
                if (poolp) {
                    // (non-negative values: the float maximum; the pixel pair of a pool window sits in lanes l, l ^ 32)
                    const f32x4 mv = f32x4{fmaxf(va.x, vb.x), fmaxf(va.y, vb.y), fmaxf(va.z, vb.z), fmaxf(va.w, vb.w)};
                    float pm[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned u = __float_as_uint(mv[i]);
                        const auto s = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                        pm[i] = fmaxf(__uint_as_float(s[0]), __uint_as_float(s[1]));
                    }
                    if (ost && e == 0) {
                        float* po = poolp + ((size_t)(oy >> 1) * Wp + (size_t)((x0 >> 1) + j)) * 8 + ch;
                        *reinterpret_cast<f32x4*>(po) = f32x4{pm[0], pm[1], pm[2], pm[3]};
                    }
                }
            }
        }
        // ---- stage 2: r1 rows i4 - 6 .. i4 - 3 -> r2 rows i4 - 5, i4 - 4 ----
        if (do_s2) {
            u32x4 q[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) ring_read(R1_OFF, PL1, (i4 + r - 6) & (NR - 1), q[r]);
            f32x4 ra = biasw[1], rb = biasw[1];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                u32x4 w[3];
                wpart(1, ky, w);
                r8ws_mm6(w, q[ky], q[ky + 1], ra, rb);
            }
            store_parts(ra, rb, R2_OFF, PL2, v2, (i4 - 5) & (NR - 1), (i4 - 4) & (NR - 1));
        }
        // ---- stage 1: r0 rows i4 - 3 .. i4 -> r1 rows i4 - 2, i4 - 1 ----
        if (do_s1) {
            u32x4 q[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r) ring_read(R0_OFF, PL0, (i4 + r - 3) & (NR - 1), q[r]);
            f32x4 ra = biasw[0], rb = biasw[0];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                u32x4 w[3];
                wpart(0, ky, w);
                r8ws_mm6(w, q[ky], q[ky + 1], ra, rb);
            }
            store_parts(ra, rb, R1_OFF, PL1, v1, (i4 - 2) & (NR - 1), (i4 - 1) & (NR - 1));
        }
        // ---- conv1: item rows 2 k + 1, 2 k + 2 (image rows Ya - 3 + 2 k, + 1) -> relu(t) parts into r0 rows i4 + 1, i4 + 2, UP: raw t into tc ----
        if (do_c1) {
            f32x4 ra = bias1, rb = bias1;
            if constexpr (UP) {
                // window rows 0, 1 are carried; rows 2, 3 = pair k + 1, requested one iteration ago; pair k + 2 is requested now
                u32x4 x2[2][2][3];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int s = 0; s < 2; ++s) split3_x8(nxt[r][s][0], nxt[r][s][1], x2[r][s][0], x2[r][s][1], x2[r][s][2]);
                if (k + 2 <= p_last) {
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        in_row(skp, Ya + 2 * k + r, nxt[r][0][0], nxt[r][0][1]);
                        in_row(dcp, Ya + 2 * k + r, nxt[r][1][0], nxt[r][1][1]);
                    }
                }
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        u32x4 w[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p) w[p] = w1[(ky * 2 + s) * 3 + p];
                        u32x4 xa[3], xb[3];
#pragma unroll
                        for (int p = 0; p < 3; ++p) {
                            xa[p] = ky == 0 ? cin[0][s][p] : (ky == 1 ? cin[1][s][p] : x2[0][s][p]);
                            xb[p] = ky == 0 ? cin[1][s][p] : (ky == 1 ? x2[0][s][p] : x2[1][s][p]);
                        }
                        r8ws_mm6(w, xa, xb, ra, rb);
                    }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int p = 0; p < 3; ++p) cin[r][s][p] = x2[r][s][p];
            } else {
                // pair k + 1 -> the ring (its rows 2 k + 2, 2 k + 3 replace those of pair k - 7, which stage 3 left behind two iterations ago), pair k + 2 is requested; then the taps of the
                // lane's pixel c (ring column c + kx) in res8v_down_kernel's order
                istore(inx, k + 1);
                if (k + 2 <= p_last) inx = iload(k + 2);
                conv1_down(2 * k + 1, min(c, 29), ra, rb);
            }
            if constexpr (UP) {
                if (tvalid) {
                    *reinterpret_cast<f32x4*>(lds + TC_OFF + ((i16 + 1) & (NT - 1)) * TW * 32 + tcol) = ra;
                    *reinterpret_cast<f32x4*>(lds + TC_OFF + ((i16 + 2) & (NT - 1)) * TW * 32 + tcol) = rb;
                }
            }
            store_parts(ra, rb, R0_OFF, PL0, v0, (i4 + 1) & (NR - 1), (i4 + 2) & (NR - 1));
        }
    }
}

}  // namespace asep
