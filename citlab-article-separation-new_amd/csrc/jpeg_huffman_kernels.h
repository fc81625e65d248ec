// Entropy decode of a baseline JPEG scan on the device (include/asep_hip.h, "JPEG entropy decode" block), by self-synchronising
// subsequences (Klein & Wiseman; Weissenberger & Schmidt).  The scan comes unstuffed from asep_jpeg_scan_prepare; every segment (restart
// interval) is cut into subsequences of `subseq_bits` bits, one thread each.  The state between two symbols is (bit position, block within
// the MCU, zigzag index), packed into one 64-bit word so that it is stored and loaded whole.
//   jpeg_huff_sync_kernel<true>    speculate: decode every subsequence from a guessed state
//   jpeg_huff_sync_kernel<false>   rounds of entry[s] = exit[s - 1]; a thread whose entry changed decodes again.  Barriers inside the
//                                  workgroup between rounds, nothing waits for another workgroup: what a neighbour workgroup stored is seen
//                                  in this launch or the next, and a launch in which no thread decoded is the fixed point.
//   jpeg_huff_scan_kernel<K, P>    segmented sums in three launches (chunk totals, carries, final): K = PLACE the exclusive sum of
//                                  completed blocks per segment, K = DC the inclusive sum of DC differences per component and segment
//   jpeg_huff_write_kernel         decode once more from the correct entries and write the coefficients; real errors -> status
//   jpeg_huff_energy_kernel        the energy bound of host_jpeg.c (MAX_BLOCK_ENERGY) per block
// The four to six Huffman tables and the de-zigzag table live in LDS (8.6 KiB).  The scan is read as 32-bit words, every read clamped to
// the buffer; every loop over symbols advances at least one bit and ends at the subsequence's end, which lies inside the segment.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/asep_hip.h"

namespace asep {

constexpr int JPEG_HUFF_BLOCK = 256;         // threads (= subsequences) per workgroup of the decode kernels
constexpr int JPEG_SCAN_BLOCK = 256;         // threads per workgroup of the sum kernels
constexpr int JPEG_SCAN_ITEMS = 4;           // consecutive elements per thread
constexpr int JPEG_SCAN_CHUNK = JPEG_SCAN_BLOCK * JPEG_SCAN_ITEMS;
constexpr int JPEG_MAX_BLOCK_ENERGY = 4000000;   // host_jpeg.c, MAX_BLOCK_ENERGY
constexpr int JPEG_CARRY_LIMIT = 1 << 30;    // carries are clamped here: above any block count, and a DC sum that far out was reported where it left its range

struct JpegHuffSeg {
    uint32_t bit_begin, bit_end;             // in the unstuffed scan
    uint32_t first_block, n_blocks;          // in scan order: first_mcu * blocks per MCU, n_mcus * blocks per MCU
    uint32_t sub_first;                      // index of its first subsequence
};

struct JpegHuffArgs {
    const uint32_t* scan;                    // big-endian bit order inside each byte string: words are byte-swapped on load
    uint32_t n_words;
    const asep_jpeg_scan_tables* tables;     // device copy
    const JpegHuffSeg* segs;
    int n_segs;
    int n_subs;
    int subseq_bits;
    int ncomp, hs, vs, bpm;                  // bpm: blocks per MCU
    int mcus_w;
    int blocks_w[3];
    long long plane_off[3];                  // of a component's plane in coef, in int16
    long long comp_blocks[3];                // blocks of a component
    int restart_interval;
    unsigned long long* entry;               // [n_subs] the state a subsequence was last decoded from
    unsigned long long* exit_;               // [n_subs] the state it ended in
    uint32_t* sub_seg;                       // [n_subs] its segment
    int32_t* count;                          // [n_subs] blocks it completed
    int32_t* first_block;                    // [n_subs] scan-order index of its first block (after PLACE)
    int32_t* changed;                        // one word: a thread decoded in this launch
    int16_t* coef;
    int32_t* status;
};

struct JpegHuffLds {
    asep_jpeg_huff tab[6];                   // dc[3], ac[3]
    uint8_t natural[64];
};

__device__ __forceinline__ unsigned long long jpeg_huff_pack(uint32_t pos, int blk, int idx) {
    return ((unsigned long long)pos << 16) | ((unsigned long long)blk << 8) | (unsigned long long)idx;
}

// zig-zag position -> natural position, ITU-T T.81 figure A.6, eight entries per word
__device__ __forceinline__ void jpeg_huff_load_lds(JpegHuffLds& l, const asep_jpeg_scan_tables* t) {
    constexpr unsigned char NAT[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    const uint32_t* src = reinterpret_cast<const uint32_t*>(t);      // dc[3], ac[3] are the first 6 * 1432 bytes
    uint32_t* dst = reinterpret_cast<uint32_t*>(l.tab);
    constexpr int WORDS = (int)(6 * sizeof(asep_jpeg_huff) / 4);
    for (int i = (int)threadIdx.x; i < WORDS; i += (int)blockDim.x) dst[i] = src[i];
    if (threadIdx.x < 64) l.natural[threadIdx.x] = NAT[threadIdx.x];
    __syncthreads();
}

struct JpegBitReader {
    const uint32_t* scan;
    uint32_t n_words;
    uint32_t wi;                             // index of w0
    uint32_t w0, w1;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return i < n_words ? __builtin_bswap32(scan[i]) : 0u; }
    __device__ __forceinline__ void start(uint32_t pos) {
        wi = pos >> 5;
        w0 = word(wi), w1 = word(wi + 1);
    }
    // the 32 bits from bit `pos` on (zeros past the buffer)
    __device__ __forceinline__ uint32_t peek(uint32_t pos) {
        const uint32_t i = pos >> 5;
        if (i != wi) {
            w0 = i == wi + 1 ? w1 : word(i);
            w1 = word(i + 1);
            wi = i;
        }
        const uint32_t sh = pos & 31;
        return sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;
    }
};

// the address of scan-order block g (< total blocks): MCU by MCU, in an MCU the luma blocks row by row, then Cb, then Cr
__device__ __forceinline__ int16_t* jpeg_huff_block_ptr(const JpegHuffArgs& a, uint32_t g) {
    const uint32_t mcu = g / (uint32_t)a.bpm, b = g - mcu * (uint32_t)a.bpm;
    const uint32_t my = mcu / (uint32_t)a.mcus_w, mx = mcu - my * (uint32_t)a.mcus_w;
    const int luma = a.bpm == 1 ? 1 : a.bpm - 2;
    if ((int)b < luma) {
        const uint32_t v = b / (uint32_t)a.hs, u = b - v * (uint32_t)a.hs;
        return a.coef + a.plane_off[0] + ((long long)(my * a.vs + v) * a.blocks_w[0] + (mx * a.hs + u)) * 64;
    }
    const int c = (int)b - luma + 1;
    return a.coef + a.plane_off[c] + ((long long)my * a.blocks_w[c] + mx) * 64;
}

// Decodes from `state` until the position reaches sub_end.  WRITE = false: the speculative rule -- an invalid code or index skips one bit, a
// symbol that would cross the segment's end stops the thread where it stands; nothing is reported.  WRITE = true: coefficients go to the
// blocks g, g + 1, ... below block_limit, any of those is an error (returned), and so is a segment that ends with blocks missing or bytes
// left over.  Returns 0 or ASEP_JPEG_STATUS_DAMAGED.
template <bool WRITE>
__device__ __forceinline__ int jpeg_huff_decode(const JpegHuffLds& l, const JpegHuffArgs& a, unsigned long long& state, uint32_t sub_end,
                                                uint32_t seg_end, int& completed, uint32_t g, uint32_t block_limit) {
    uint32_t pos = (uint32_t)(state >> 16);
    int blk = (int)((state >> 8) & 255), idx = (int)(state & 255);
    const int luma = a.bpm == 1 ? 1 : a.bpm - 2;
    JpegBitReader r{a.scan, a.n_words, 0, 0, 0};
    r.start(pos);
    int16_t* dst = nullptr;
    if (WRITE && g < block_limit) dst = jpeg_huff_block_ptr(a, g);
    completed = 0;
    int err = 0;
    while (pos < sub_end) {                                          // every pass advances pos by >= 1 or leaves the loop
        if (WRITE && g >= block_limit) break;                        // the segment's blocks are complete
        const int comp = blk < luma ? 0 : blk - luma + 1;
        const asep_jpeg_huff& t = l.tab[(idx == 0 ? 0 : 3) + comp];
        const uint32_t v = r.peek(pos);
        int len = 0, sym = 0;
        const uint32_t e = t.look[v >> (32 - ASEP_JPEG_LOOK_BITS)];
        if (e) {
            len = (int)(e >> 8), sym = (int)(e & 255);
        } else {
            for (int k = ASEP_JPEG_LOOK_BITS + 1; k <= 16; ++k) {
                const int code = (int)(v >> (32 - k));
                if (code <= t.maxcode[k]) {
                    const int i = code + t.valoff[k];
                    if (i >= 0 && i < t.nsym) len = k, sym = t.sym[i];
                    break;
                }
            }
        }
        bool valid = len != 0, done = false;
        int s = 0, at = 0, next_idx = idx;
        if (valid) {
            if (idx == 0) {
                s = sym;
                valid = s <= 11;
                next_idx = 1;
            } else {
                const int run = sym >> 4;
                s = sym & 15;
                if (s == 0) {
                    if (run == 0) done = true;                       // end of block
                    else if (run == 15) next_idx = idx + 16, valid = next_idx <= 64;
                    else valid = false;                              // end-of-band runs belong to progressive scans
                } else {
                    at = idx + run;
                    valid = at <= 63 && s <= 10;
                    next_idx = at + 1;
                }
            }
        }
        if (!valid) {
            if (WRITE) { err = ASEP_JPEG_STATUS_DAMAGED; break; }
            pos += 1;
            continue;
        }
        const uint32_t total = (uint32_t)(len + s);                  // <= 16 + 11, inside the 32 bits of v
        if (total > seg_end - pos) {                                 // the segment does not hold the symbol (pos < sub_end <= seg_end)
            if (WRITE) err = ASEP_JPEG_STATUS_DAMAGED;
            break;
        }
        if (WRITE && s) {
            const int bits = (int)((v << len) >> (32 - s));
            dst[l.natural[at]] = (int16_t)(bits < (1 << (s - 1)) ? bits - (1 << s) + 1 : bits);      // T.81 F.2.2.1
        }
        pos += total;
        idx = next_idx;
        if (done || idx >= 64) {
            idx = 0;
            blk = blk + 1 == a.bpm ? 0 : blk + 1;
            ++completed;
            if (WRITE) {
                ++g;
                if (g < block_limit) dst = jpeg_huff_block_ptr(a, g);
            }
        }
    }
    state = jpeg_huff_pack(pos, blk, idx);
    if (WRITE && !err) {
        if (g >= block_limit) {
            if (seg_end - pos >= 8) err = ASEP_JPEG_STATUS_DAMAGED;  // whole bytes behind the last block
        } else if (sub_end == seg_end) {
            err = ASEP_JPEG_STATUS_DAMAGED;                          // the segment ends with blocks missing
        }
    }
    return err;
}

// the segment of subsequence s: the last one whose sub_first is <= s
__device__ __forceinline__ uint32_t jpeg_huff_find_seg(const JpegHuffArgs& a, uint32_t s) {
    uint32_t lo = 0, hi = (uint32_t)a.n_segs;                        // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.segs[mid].sub_first <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <bool SPECULATE>
__global__ __launch_bounds__(JPEG_HUFF_BLOCK) void jpeg_huff_sync_kernel(const JpegHuffArgs a, const int rounds) {
    __shared__ JpegHuffLds l;
    jpeg_huff_load_lds(l, a.tables);
    const uint32_t s = blockIdx.x * JPEG_HUFF_BLOCK + threadIdx.x;
    const bool active = s < (uint32_t)a.n_subs;
    uint32_t sub_begin = 0, sub_end = 0, seg_end = 0;
    bool head = true;
    if (active) {
        const uint32_t si = SPECULATE ? jpeg_huff_find_seg(a, s) : a.sub_seg[s];
        const JpegHuffSeg seg = a.segs[si];
        sub_begin = seg.bit_begin + (s - seg.sub_first) * (uint32_t)a.subseq_bits;   // < bit_end: the host counted the subsequences
        seg_end = seg.bit_end;
        sub_end = min(sub_begin + (uint32_t)a.subseq_bits, seg_end);
        head = s == seg.sub_first;
        if (SPECULATE) a.sub_seg[s] = si;
    }
    if (SPECULATE) {
        if (!active) return;
        // a segment's first subsequence starts a block; the others guess the commonest state, an AC position of the MCU's first block
        unsigned long long st = jpeg_huff_pack(sub_begin, 0, head ? 0 : 1);
        a.entry[s] = st;
        int completed;
        jpeg_huff_decode<false>(l, a, st, sub_end, seg_end, completed, 0, 0);
        a.count[s] = completed;
        __hip_atomic_store(&a.exit_[s], st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    unsigned long long cur = active ? a.entry[s] : 0;
    bool any = false;
    for (int r = 0; r < rounds; ++r) {
        if (active && !head) {
            const unsigned long long e = __hip_atomic_load(&a.exit_[s - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (e != cur) {
                cur = e;
                unsigned long long st = e;
                int completed;
                jpeg_huff_decode<false>(l, a, st, sub_end, seg_end, completed, 0, 0);
                a.count[s] = completed;
                __hip_atomic_store(&a.exit_[s], st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                any = true;
            }
        }
        __syncthreads();
    }
    if (any) a.entry[s] = cur;
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(a.changed, 1);
}

__global__ __launch_bounds__(JPEG_HUFF_BLOCK) void jpeg_huff_write_kernel(const JpegHuffArgs a) {
    __shared__ JpegHuffLds l;
    jpeg_huff_load_lds(l, a.tables);
    const uint32_t s = blockIdx.x * JPEG_HUFF_BLOCK + threadIdx.x;
    if (s >= (uint32_t)a.n_subs) return;
    const JpegHuffSeg seg = a.segs[a.sub_seg[s]];
    const uint32_t sub_begin = seg.bit_begin + (s - seg.sub_first) * (uint32_t)a.subseq_bits;
    const uint32_t sub_end = min(sub_begin + (uint32_t)a.subseq_bits, seg.bit_end);
    unsigned long long st = s == seg.sub_first ? jpeg_huff_pack(sub_begin, 0, 0) : a.exit_[s - 1];
    const uint32_t limit = seg.first_block + seg.n_blocks;           // <= the frame's blocks: checked on the host
    const int32_t fb = a.first_block[s];
    const uint32_t g = fb < 0 ? limit : min((uint32_t)fb, limit);
    int completed;
    const int err = jpeg_huff_decode<true>(l, a, st, sub_end, seg.bit_end, completed, g, limit);
    if (err) atomicOr(a.status, err);
}

// ---- segmented sums ------------------------------------------------------------------------------------------------------------------
enum { JPEG_SCAN_PLACE = 0, JPEG_SCAN_DC = 1 };

struct JpegScanArgs {
    JpegHuffArgs h;
    int chunks;                              // per component (gridDim.x)
    int32_t* chunk_sum;                      // [components][chunks] sum from the chunk's last head (or its start) to its end
    int32_t* chunk_head;                     // [components][chunks] the chunk holds a head
    int32_t* chunk_carry;                    // [components][chunks] what elements in front of its first head add
};

// element j of component c (PLACE: subsequence j): its value and whether it starts a segment
template <int KIND>
__device__ __forceinline__ void jpeg_scan_load(const JpegHuffArgs& a, int c, long long j, int& value, bool& head, int16_t*& where) {
    if (KIND == JPEG_SCAN_PLACE) {
        value = a.count[j];
        head = a.segs[a.sub_seg[j]].sub_first == (uint32_t)j;
        where = nullptr;
    } else {
        const int luma = a.bpm == 1 ? 1 : a.bpm - 2;
        const int per = c == 0 ? luma : 1;                           // blocks of c in an MCU
        const long long mcu = j / per;
        const int b = (int)(j - mcu * per) + (c == 0 ? 0 : luma + c - 1);
        where = jpeg_huff_block_ptr(a, (uint32_t)(mcu * a.bpm + b));
        value = where[0];
        head = a.restart_interval > 0 ? j % ((long long)a.restart_interval * per) == 0 : j == 0;
    }
}

template <int KIND>
__device__ __forceinline__ long long jpeg_scan_count(const JpegHuffArgs& a, int c) {
    return KIND == JPEG_SCAN_PLACE ? (long long)a.n_subs : a.comp_blocks[c];
}

// PASS 0: the chunk's total and head flag.  PASS 2: the sums themselves, with the chunk's carry.
template <int KIND, int PASS>
__global__ __launch_bounds__(JPEG_SCAN_BLOCK) void jpeg_huff_scan_kernel(const JpegScanArgs a) {
    __shared__ int lv[JPEG_SCAN_BLOCK];
    __shared__ int lf[JPEG_SCAN_BLOCK];
    const int c = (int)blockIdx.y, t = (int)threadIdx.x;
    const long long n = jpeg_scan_count<KIND>(a.h, c);
    const long long j0 = ((long long)blockIdx.x * JPEG_SCAN_BLOCK + t) * JPEG_SCAN_ITEMS;
    int v[JPEG_SCAN_ITEMS], own[JPEG_SCAN_ITEMS];
    bool f[JPEG_SCAN_ITEMS];
    int16_t* where[JPEG_SCAN_ITEMS];
#pragma unroll
    for (int i = 0; i < JPEG_SCAN_ITEMS; ++i) {
        v[i] = 0, f[i] = false, where[i] = nullptr;
        if (j0 + i < n) jpeg_scan_load<KIND>(a.h, c, j0 + i, v[i], f[i], where[i]);
        own[i] = v[i];
        if (i > 0) {
            if (!f[i]) v[i] += v[i - 1];
            f[i] = f[i] || f[i - 1];
        }
    }
    // inclusive scan of the threads' totals under (F1, V1) + (F2, V2) = (F1 | F2, F2 ? V2 : V1 + V2)
    int tv = v[JPEG_SCAN_ITEMS - 1], tf = f[JPEG_SCAN_ITEMS - 1] ? 1 : 0;
    lv[t] = tv, lf[t] = tf;
    __syncthreads();
    for (int d = 1; d < JPEG_SCAN_BLOCK; d <<= 1) {
        int pv = 0, pf = 0;
        if (t >= d) pv = lv[t - d], pf = lf[t - d];
        __syncthreads();
        if (t >= d) {
            if (!tf) tv += pv;
            tf |= pf;
            lv[t] = tv, lf[t] = tf;
        }
        __syncthreads();
    }
    const size_t ci = (size_t)c * a.chunks + blockIdx.x;
    if (PASS == 0) {
        if (t == JPEG_SCAN_BLOCK - 1) a.chunk_sum[ci] = tv, a.chunk_head[ci] = tf;
        return;
    }
    const int before_v = t ? lv[t - 1] : 0, before_f = t ? lf[t - 1] : 0;
    const int carry = a.chunk_carry[ci];
    int bad = 0;
#pragma unroll
    for (int i = 0; i < JPEG_SCAN_ITEMS; ++i) {
        if (j0 + i >= n) break;
        int sum = v[i];
        if (!f[i]) {
            sum += before_v;
            if (!before_f) sum += carry;
        }
        if (KIND == JPEG_SCAN_PLACE) {
            a.h.first_block[j0 + i] = (int32_t)a.h.segs[a.h.sub_seg[j0 + i]].first_block + sum - own[i];
        } else {
            if (sum < -2048 || sum > 2047) bad = 1;                  // beyond what 8-bit samples can give (host_jpeg.c, decode_block)
            where[i][0] = (int16_t)sum;
        }
    }
    if (bad) atomicOr(a.h.status, ASEP_JPEG_STATUS_DAMAGED);
}

// PASS 1: one workgroup per component walks the chunk totals in tiles; thread 0 carries the running sum through a tile in LDS
template <int KIND>
__global__ __launch_bounds__(JPEG_SCAN_BLOCK) void jpeg_huff_carry_kernel(const JpegScanArgs a) {
    __shared__ int lv[JPEG_SCAN_BLOCK];
    __shared__ int lf[JPEG_SCAN_BLOCK];
    __shared__ int lc[JPEG_SCAN_BLOCK];
    const int c = (int)blockIdx.x, t = (int)threadIdx.x;
    const size_t base = (size_t)c * a.chunks;
    long long running = 0;                                           // only thread 0's is used
    for (int first = 0; first < a.chunks; first += JPEG_SCAN_BLOCK) {
        const int i = first + t;
        if (i < a.chunks) lv[t] = a.chunk_sum[base + i], lf[t] = a.chunk_head[base + i];
        __syncthreads();
        if (t == 0) {
            const int m = min(JPEG_SCAN_BLOCK, a.chunks - first);
            for (int k = 0; k < m; ++k) {
                lc[k] = (int)max(-(long long)JPEG_CARRY_LIMIT, min((long long)JPEG_CARRY_LIMIT, running));
                running = lf[k] ? (long long)lv[k] : running + lv[k];
            }
        }
        __syncthreads();
        if (i < a.chunks) a.chunk_carry[base + i] = lc[t];
        __syncthreads();
    }
}

// one thread per block of any component: sum of (coefficient * quantiser)^2 above the bound -> refused
__global__ __launch_bounds__(JPEG_SCAN_BLOCK) void jpeg_huff_energy_kernel(const JpegHuffArgs a, const int qt0, const int qt1, const int qt2,
                                                                           const long long total) {
    __shared__ uint16_t q[3][64];
    if (threadIdx.x < 192) {
        const int c = (int)threadIdx.x >> 6, k = (int)threadIdx.x & 63;
        q[c][k] = a.tables->qt[c == 0 ? qt0 : (c == 1 ? qt1 : qt2)][k];
    }
    __syncthreads();
    const long long b = (long long)blockIdx.x * JPEG_SCAN_BLOCK + threadIdx.x;
    if (b >= total) return;
    const int c = (a.ncomp > 2 && b >= a.comp_blocks[0] + a.comp_blocks[1]) ? 2 : ((a.ncomp > 1 && b >= a.comp_blocks[0]) ? 1 : 0);
    const uint4* src = reinterpret_cast<const uint4*>(a.coef + b * 64);  // the planes follow each other: block b of the whole buffer
    int energy = 0;
    bool over = false;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 w = src[r];
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x0 = (int)(int16_t)(u[k] & 0xffffu) * (int)q[c][r * 8 + 2 * k];
            const int x1 = (int)(int16_t)(u[k] >> 16) * (int)q[c][r * 8 + 2 * k + 1];
            // one term above 2000^2 decides alone; below that 64 terms stay far inside int32
            over = over || x0 > 2000 || x0 < -2000 || x1 > 2000 || x1 < -2000;
            energy += (over ? 0 : x0 * x0) + (over ? 0 : x1 * x1);
        }
    }
    if (over || energy > JPEG_MAX_BLOCK_ENERGY) atomicOr(a.status, ASEP_JPEG_STATUS_REFUSED);
}

}  // namespace asep
