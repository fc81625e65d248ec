// Relation net evaluation (article_separation/gnn/trainer/lav_rel.py of the reference): the device side of sklearn's
// _binary_clf_curve over every ordered pair of an evaluation list.  A pair travels as ONE 32-bit key
//     key = (float_bits(p) << 1) | label
// p being the class-1 probability (sign bit clear, so nothing is lost) and label the ground truth: the unsigned order of the
// keys is the order of (p, label), and no payload moves through the sort.  Everything below is integer work: the results do
// not depend on the launch geometry or on the order in which blocks run.
//
// Sort: least-significant-digit radix sort, 8 bits x 4 passes, each pass three launches
//     relev_hist_kernel     per tile the count of every digit value            table[digit][tile], totals[digit]
//     relev_scan_kernel     exclusive scan of the table in (digit, tile) order  (one block per digit row, a running carry)
//     relev_scatter_kernel  stable rank inside the tile, staged through LDS, written out as runs of equal digit
// No block waits for another block anywhere (no look-back chain): the order between the launches is the only dependency.
// Curve: three launches mark the first element of every run of equal p in the ascending keys and write, in descending
// order of p, the threshold, tps and fps; a fourth adds up A2 = sum (fps_k - fps_{k-1}) (tps_k + tps_{k-1}).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asep {

constexpr int RELEV_BLOCK = 256;                          // threads per block (4 waves of 64) in every kernel below
constexpr int RELEV_WAVES = RELEV_BLOCK / 64;
constexpr int RELEV_KPT = 16;                             // keys per thread
constexpr int RELEV_TILE = RELEV_BLOCK * RELEV_KPT;       // keys per block: 4096 (16 KiB of LDS in the scatter)
constexpr int RELEV_RADIX = 256;                          // digit values per pass (== RELEV_BLOCK: thread d owns digit d)
constexpr uint32_t RELEV_BITS_HALF = 0x3F000000u;         // float bits of 0.5: for 0 <= p <= 1, p > 0.5 <=> bits > this
constexpr uint32_t RELEV_BITS_ONE = 0x3F800000u;          // float bits of 1.0: bits above it are p > 1, p < 0, inf or NaN
static_assert(RELEV_RADIX == RELEV_BLOCK, "one thread per digit value");

// slots of the counter block (unsigned 64-bit each)
enum { RELEV_C_BAD = 0, RELEV_C_POS = 1, RELEV_C_CORRECT = 2, RELEV_C_BADGT = 3, RELEV_C_T = 4, RELEV_C_P = 5, RELEV_C_A2 = 6,
       RELEV_C_SLOTS = 8 };

__device__ __forceinline__ uint32_t relev_score_bits(float p) {
    const uint32_t b = __float_as_uint(p);
    return b == 0x80000000u ? 0u : b;                     // -0.0 is 0.0 (sklearn compares values)
}

// sum over the block of one value per thread; every thread gets it.  s_tmp holds RELEV_WAVES entries.
template <class T>
__device__ __forceinline__ T relev_block_sum(T v, T* s_tmp) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                      // (s_tmp may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    for (int w = 0; w < RELEV_WAVES; ++w) t += s_tmp[w];
    return t;
}

// exclusive scan over the block of one value per thread (in thread order); *total = the block's sum.
__device__ __forceinline__ uint32_t relev_block_excl_scan(uint32_t v, uint32_t* s_tmp, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) s_tmp[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < RELEV_WAVES; ++w) {
        const uint32_t t = s_tmp[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

// ---- append ------------------------------------------------------------------------------------------------------------------
// One page of the net: probs [R, num_classes], the last class column is the score.  keys[r] = bits << 1 (label 0 for now).
// Counts the scores the host must refuse and the pairs a label of 0 classifies correctly (p <= 0.5).
__global__ void __launch_bounds__(RELEV_BLOCK) relev_pack_page_kernel(const float* __restrict__ probs, int num_classes, uint32_t R,
                                                                      uint32_t* __restrict__ keys,
                                                                      unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    const uint32_t r = blockIdx.x * RELEV_BLOCK + threadIdx.x;
    uint32_t bad = 0, correct = 0;
    if (r < R) {
        const uint32_t bits = relev_score_bits(probs[(size_t)r * num_classes + (num_classes - 1)]);
        bad = bits > RELEV_BITS_ONE;
        correct = !(bits > RELEV_BITS_HALF);
        keys[r] = bits << 1;
    }
    const uint32_t both = relev_block_sum<uint32_t>(bad | (correct << 16), s_tmp);   // each <= 256
    if (threadIdx.x == 0) {
        if (both & 0xFFFFu) atomicAdd(&cnt[RELEV_C_BAD], (unsigned long long)(both & 0xFFFFu));
        if (both >> 16) atomicAdd(&cnt[RELEV_C_CORRECT], (unsigned long long)(both >> 16));
    }
}

// The page's ground truth rows (., i, j) set the label bit of pair i * N + j (input_dataset.py build_full_relations).  The
// thread that sets a bit first accounts for it: one more positive, and the pair is now correct when p > 0.5 instead of p <= 0.5.
__global__ void __launch_bounds__(RELEV_BLOCK) relev_label_page_kernel(const int32_t* __restrict__ gt, int G, int N,
                                                                       uint32_t* __restrict__ keys,
                                                                       unsigned long long* __restrict__ cnt) {
    const int g = blockIdx.x * RELEV_BLOCK + threadIdx.x;
    if (g >= G) return;
    const int i = gt[3 * g + 1], j = gt[3 * g + 2];
    if ((unsigned)i >= (unsigned)N || (unsigned)j >= (unsigned)N) {
        atomicAdd(&cnt[RELEV_C_BADGT], 1ull);
        return;
    }
    const uint32_t old = atomicOr(&keys[(size_t)i * N + j], 1u);
    if (!(old & 1u)) {
        atomicAdd(&cnt[RELEV_C_POS], 1ull);
        atomicAdd(&cnt[RELEV_C_CORRECT], (old >> 1) > RELEV_BITS_HALF ? 1ull : ~0ull);   // +1 or -1 (mod 2^64)
    }
}

// Scores and labels from arrays (append_host): the same key, the same counters.
__global__ void __launch_bounds__(RELEV_BLOCK) relev_pack_arrays_kernel(const float* __restrict__ probs,
                                                                        const uint8_t* __restrict__ labels, uint32_t n,
                                                                        uint32_t* __restrict__ keys,
                                                                        unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    uint32_t packed = 0;                                  // bad | pos << 10 | correct << 20, each <= 256 per block
    const uint32_t r = blockIdx.x * RELEV_BLOCK + threadIdx.x;
    if (r < n) {
        const uint32_t bits = relev_score_bits(probs[r]);
        const uint32_t lab = labels[r] != 0;
        keys[r] = (bits << 1) | lab;
        packed = (uint32_t)(bits > RELEV_BITS_ONE) | (lab << 10) | ((uint32_t)((bits > RELEV_BITS_HALF) == (lab != 0)) << 20);
    }
    packed = relev_block_sum<uint32_t>(packed, s_tmp);
    if (threadIdx.x == 0) {
        const uint32_t bad = packed & 0x3FFu, pos = (packed >> 10) & 0x3FFu, correct = packed >> 20;
        if (bad) atomicAdd(&cnt[RELEV_C_BAD], (unsigned long long)bad);
        if (pos) atomicAdd(&cnt[RELEV_C_POS], (unsigned long long)pos);
        if (correct) atomicAdd(&cnt[RELEV_C_CORRECT], (unsigned long long)correct);
    }
}

// ---- radix sort ----------------------------------------------------------------------------------------------------------------
// A tile is RELEV_TILE consecutive keys; wave w of the block owns the keys w * 64 * KPT .. of it and walks them in KPT rounds
// of 64 consecutive keys (lane l holds key round * 64 + l).  Per round the lanes that hold the same digit find each other with
// eight ballots (64-bit on wave64); `below` = how many of them sit in lower lanes.  s_cnt[w][d] runs along: the key's rank
// among the keys of digit d in its wave is s_cnt before the round + below.  Returns that rank (valid lanes only).
__device__ __forceinline__ uint32_t relev_rank_round(uint32_t digit, bool valid, uint32_t* s_cnt_wave) {
    const int lane = threadIdx.x & 63;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        same &= bit ? bal : ~bal;
    }
    const uint32_t below = __popcll(same & ((1ull << lane) - 1ull));
    const uint32_t count = __popcll(same);
    uint32_t old = 0;
    if (valid) old = s_cnt_wave[digit];
    __builtin_amdgcn_wave_barrier();                      // every lane has read before the first lane of each group writes
    if (valid && below == 0) s_cnt_wave[digit] = old + count;
    __builtin_amdgcn_wave_barrier();
    return old + below;
}

// table[d * n_tiles + tile] = number of keys of the tile whose digit (key >> shift) & 255 is d; totals[d] += the same.
__global__ void __launch_bounds__(RELEV_BLOCK) relev_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, int shift,
                                                                 uint32_t n_tiles, uint32_t* __restrict__ table,
                                                                 uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_cnt[RELEV_WAVES][RELEV_RADIX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < RELEV_WAVES; ++w) s_cnt[w][tid] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RELEV_TILE + wave * (64 * RELEV_KPT) + lane;
#pragma unroll
    for (int r = 0; r < RELEV_KPT; ++r) {
        const uint32_t idx = base + r * 64;
        const bool valid = idx < n;
        const uint32_t key = valid ? keys[idx] : 0u;
        relev_rank_round((key >> shift) & 255u, valid, s_cnt[wave]);
    }
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < RELEV_WAVES; ++w) tot += s_cnt[w][tid];
    table[(size_t)tid * n_tiles + blockIdx.x] = tot;
    if (tot) atomicAdd(&totals[tid], tot);                // device scope: the tiles of one digit run on every XCD
}

// grid = RELEV_RADIX blocks.  Block d turns row d of the table into exclusive offsets in the output: the keys of all lower
// digits (from totals) plus the keys of digit d in the tiles before.  One block walks its row with a carry.
__global__ void __launch_bounds__(RELEV_BLOCK) relev_scan_kernel(uint32_t* __restrict__ table, const uint32_t* __restrict__ totals,
                                                                 uint32_t n_tiles) {
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    const uint32_t d = blockIdx.x, tid = threadIdx.x;
    uint32_t carry = relev_block_sum<uint32_t>(tid < d ? totals[tid] : 0u, s_tmp);
    uint32_t* row = table + (size_t)d * n_tiles;
    for (uint32_t c0 = 0; c0 < n_tiles; c0 += RELEV_BLOCK * 4) {
        uint32_t v[4], sum = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t i = c0 + tid * 4 + e;
            v[e] = i < n_tiles ? row[i] : 0u;
            sum += v[e];
        }
        uint32_t total;
        uint32_t run = carry + relev_block_excl_scan(sum, s_tmp, &total);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t i = c0 + tid * 4 + e;
            if (i < n_tiles) row[i] = run;
            run += v[e];
        }
        carry += total;
    }
}

// Stable scatter of one tile: rank as in the histogram, place the tile's keys in LDS ordered by digit (stable), then write
// them out so that neighbouring threads write neighbouring addresses inside a run of equal digit.  table holds the scanned
// offsets; every target index is below n because the histogram counted exactly these keys.
__global__ void __launch_bounds__(RELEV_BLOCK) relev_scatter_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                    const uint32_t* __restrict__ table, uint32_t n, int shift,
                                                                    uint32_t n_tiles) {
    __shared__ uint32_t s_cnt[RELEV_WAVES][RELEV_RADIX];
    __shared__ uint32_t s_keys[RELEV_TILE];
    __shared__ uint32_t s_gbase[RELEV_RADIX], s_lstart[RELEV_RADIX];
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int w = 0; w < RELEV_WAVES; ++w) s_cnt[w][tid] = 0;
    s_gbase[tid] = table[(size_t)tid * n_tiles + blockIdx.x];
    __syncthreads();
    const uint32_t tile0 = blockIdx.x * (uint32_t)RELEV_TILE;
    const uint32_t base = tile0 + wave * (64 * RELEV_KPT) + lane;
    uint32_t key[RELEV_KPT], rank[RELEV_KPT];
#pragma unroll
    for (int r = 0; r < RELEV_KPT; ++r) {
        const uint32_t idx = base + r * 64;
        const bool valid = idx < n;
        key[r] = valid ? in[idx] : 0u;
        rank[r] = relev_rank_round((key[r] >> shift) & 255u, valid, s_cnt[wave]);
    }
    __syncthreads();
    // thread d: where digit d starts in the sorted tile, and where each wave's share of it starts
    uint32_t c[RELEV_WAVES], tot = 0;
#pragma unroll
    for (int w = 0; w < RELEV_WAVES; ++w) {
        c[w] = s_cnt[w][tid];
        tot += c[w];
    }
    uint32_t unused;
    uint32_t start = relev_block_excl_scan(tot, s_tmp, &unused);
    s_lstart[tid] = start;
#pragma unroll
    for (int w = 0; w < RELEV_WAVES; ++w) {
        s_cnt[w][tid] = start;
        start += c[w];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RELEV_KPT; ++r)
        if (base + r * 64 < n) s_keys[s_cnt[wave][(key[r] >> shift) & 255u] + rank[r]] = key[r];
    __syncthreads();
    const uint32_t tile_n = min((uint32_t)RELEV_TILE, n - tile0);
    for (uint32_t i = tid; i < tile_n; i += RELEV_BLOCK) {
        const uint32_t k = s_keys[i], d = (k >> shift) & 255u;
        out[s_gbase[d] + (i - s_lstart[d])] = k;
    }
}

// ---- curve ---------------------------------------------------------------------------------------------------------------------
// keys ascending.  Element i opens a run when i == 0 or its score differs from the one before it.  Thread t of a block owns
// the KPT consecutive elements tile0 + t * KPT ..: `runs` and `ones` count the run openings and the labels among them.
__device__ __forceinline__ void relev_curve_load(const uint32_t* __restrict__ keys, uint32_t n, uint32_t first,
                                                 uint32_t (&k)[RELEV_KPT], uint32_t& prev, uint32_t& runs, uint32_t& ones) {
    runs = ones = 0;
    prev = (first > 0 && first < n) ? keys[first - 1] >> 1 : 0xFFFFFFFFu;   // no score has these bits: element 0 opens a run
    if (first + RELEV_KPT <= n) {
        const uint4* p = reinterpret_cast<const uint4*>(keys + first);     // first is a multiple of 16 elements
#pragma unroll
        for (int q = 0; q < RELEV_KPT / 4; ++q) {
            const uint4 v = p[q];
            k[4 * q] = v.x, k[4 * q + 1] = v.y, k[4 * q + 2] = v.z, k[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < RELEV_KPT; ++e) k[e] = first + e < n ? keys[first + e] : 0u;
    }
    uint32_t last = prev;
#pragma unroll
    for (int e = 0; e < RELEV_KPT; ++e)
        if (first + e < n) {
            runs += (k[e] >> 1) != last;
            ones += k[e] & 1u;
            last = k[e] >> 1;
        }
}

__global__ void __launch_bounds__(RELEV_BLOCK) relev_curve_count_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                                        uint32_t* __restrict__ blk_runs,
                                                                        uint32_t* __restrict__ blk_ones) {
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    uint32_t k[RELEV_KPT], prev, runs, ones;
    relev_curve_load(keys, n, blockIdx.x * (uint32_t)RELEV_TILE + threadIdx.x * RELEV_KPT, k, prev, runs, ones);
    const uint32_t both = relev_block_sum<uint32_t>(runs | (ones << 16), s_tmp);      // each <= 4096
    if (threadIdx.x == 0) {
        blk_runs[blockIdx.x] = both & 0xFFFFu;
        blk_ones[blockIdx.x] = both >> 16;
    }
}

// one block: both per-tile arrays become exclusive offsets; cnt[T] = number of runs, cnt[P] = number of positives
__global__ void __launch_bounds__(RELEV_BLOCK) relev_curve_scan_kernel(uint32_t* __restrict__ blk_runs, uint32_t* __restrict__ blk_ones,
                                                                       uint32_t n_tiles, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    uint32_t carry_r = 0, carry_o = 0;
    for (uint32_t c0 = 0; c0 < n_tiles; c0 += RELEV_BLOCK) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t r = i < n_tiles ? blk_runs[i] : 0u, o = i < n_tiles ? blk_ones[i] : 0u;
        uint32_t tot_r, tot_o;
        const uint32_t ex_r = relev_block_excl_scan(r, s_tmp, &tot_r);
        const uint32_t ex_o = relev_block_excl_scan(o, s_tmp, &tot_o);
        if (i < n_tiles) {
            blk_runs[i] = carry_r + ex_r;
            blk_ones[i] = carry_o + ex_o;
        }
        carry_r += tot_r;
        carry_o += tot_o;
    }
    if (threadIdx.x == 0) {
        cnt[RELEV_C_T] = carry_r;
        cnt[RELEV_C_P] = carry_o;
    }
}

// The run opened by ascending element s is threshold number T - 1 - (runs before s) in descending order of p:
// tps = positives at or above it = P - (ones before s), fps = (n - s) - tps  (sklearn's _binary_clf_curve).
__global__ void __launch_bounds__(RELEV_BLOCK) relev_curve_write_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                                        const uint32_t* __restrict__ blk_runs,
                                                                        const uint32_t* __restrict__ blk_ones, uint32_t T, uint32_t P,
                                                                        float* __restrict__ thresholds, long long* __restrict__ tps,
                                                                        long long* __restrict__ fps) {
    __shared__ uint32_t s_tmp[RELEV_WAVES];
    const uint32_t first = blockIdx.x * (uint32_t)RELEV_TILE + threadIdx.x * RELEV_KPT;
    uint32_t k[RELEV_KPT], prev, runs, ones, unused;
    relev_curve_load(keys, n, first, k, prev, runs, ones);
    const uint32_t ex = relev_block_excl_scan(runs | (ones << 16), s_tmp, &unused);   // block sums <= 4096 each: no carry into bit 16
    uint32_t run = blk_runs[blockIdx.x] + (ex & 0xFFFFu), one = blk_ones[blockIdx.x] + (ex >> 16);
#pragma unroll
    for (int e = 0; e < RELEV_KPT; ++e)
        if (first + e < n) {
            if ((k[e] >> 1) != prev) {
                const uint32_t at = T - 1u - run;
                if (at < T) {                                  // always: run < T by construction
                    const uint32_t tp = P - one;
                    thresholds[at] = __uint_as_float(k[e] >> 1);
                    tps[at] = tp;
                    fps[at] = (n - (first + e)) - tp;
                }
                ++run;
            }
            one += k[e] & 1u;
            prev = k[e] >> 1;
        }
}

// cnt[A2] += sum over this block's thresholds of (fps_k - fps_{k-1}) (tps_k + tps_{k-1}); below 2^62 for n < 2^31
__global__ void __launch_bounds__(RELEV_BLOCK) relev_curve_a2_kernel(const long long* __restrict__ tps, const long long* __restrict__ fps,
                                                                     uint32_t T, unsigned long long* __restrict__ cnt) {
    __shared__ unsigned long long s_tmp[RELEV_WAVES];
    unsigned long long acc = 0;
    for (uint32_t k = blockIdx.x * RELEV_BLOCK + threadIdx.x; k < T; k += gridDim.x * RELEV_BLOCK) {
        const long long tp = tps[k], fp = fps[k], tp0 = k ? tps[k - 1] : 0, fp0 = k ? fps[k - 1] : 0;
        acc += (unsigned long long)(fp - fp0) * (unsigned long long)(tp + tp0);
    }
    acc = relev_block_sum<unsigned long long>(acc, s_tmp);
    if (threadIdx.x == 0 && acc) atomicAdd(&cnt[RELEV_C_A2], acc);
}

}  // namespace asep
