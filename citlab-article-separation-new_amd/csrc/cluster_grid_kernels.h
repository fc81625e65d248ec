// Clustering grid (clustering/dbscan.py, DBScanRelation.cluster_relations, and the split / merge counts of as_eval.py): one
// wavefront per (page, setting) problem.  The labels are the host class's, integer for integer: the neighbourhood and
// agreement comparisons are taken in the matrix dtype against the threshold rounded to that dtype, and the agreement mean
// is numpy's np.mean of the gathered row (np_mean below: pairwise summation in numpy's order, then one division).
// Compiled with -ffp-contract=off.  The summation template at the top needs no HIP: a host test compiles it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLG_HD __host__ __device__
#else
#define CLG_HD
#endif

namespace asep {

constexpr int CLG_MAX_NODES = 2048;    // nodes of one page: labels, owner queue and member values of a problem sit in LDS
constexpr int CLG_PAIRWISE_DEPTH = 6;  // halvings of np_pairwise_sum above its 128-element blocks

// numpy's pairwise_sum (the inner loop of np.add.reduce over a contiguous array) for n <= 128: below 8 a serial sum from
// 0, else eight running sums seeded with a[0..7] and stepped by 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the n % 8 tail added serially.
template <class T>
CLG_HD inline T np_block_sum(const T* a, int n) {
    if (n < 8) {
        T res = T(0);
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    T r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += a[i + 0];
        r1 += a[i + 1];
        r2 += a[i + 2];
        r3 += a[i + 3];
        r4 += a[i + 4];
        r5 += a[i + 5];
        r6 += a[i + 6];
        r7 += a[i + 7];
    }
    T res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

// Above 128 elements numpy splits at n2 = n/2 - (n/2) % 8 and adds the two halves' results.  DEPTH bounds the halvings
// (the recursion is unrolled by the template, no device stack): pairwise_depth() says how many a length needs.
template <class T, int DEPTH = CLG_PAIRWISE_DEPTH>
CLG_HD inline T np_pairwise_sum(const T* a, int n) {
    if constexpr (DEPTH > 0) {
        if (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            return np_pairwise_sum<T, DEPTH - 1>(a, n2) + np_pairwise_sum<T, DEPTH - 1>(a + n2, n - n2);
        }
    }
    return np_block_sum(a, n);
}

constexpr int pairwise_depth(int n) {
    int d = 0;
    while (n > 128) {      // the longer half: n - n2
        int n2 = n / 2;
        n2 -= n2 % 8;
        n -= n2;
        ++d;
    }
    return d;
}
static_assert(pairwise_depth(CLG_MAX_NODES) <= CLG_PAIRWISE_DEPTH && pairwise_depth(CLG_MAX_NODES - 1) <= CLG_PAIRWISE_DEPTH,
              "np_pairwise_sum cannot halve a row of CLG_MAX_NODES members down to 128");

// np.mean of a contiguous 1-D array of n >= 1 values, in the array's dtype
template <class T>
CLG_HD inline T np_mean(const T* a, int n) {
    return (T(0) + np_pairwise_sum<T>(a, n)) / T(n);
}

#if defined(__HIPCC__)

constexpr int CLG_WAVE = 64;
constexpr int CLG_MAX_PROBLEMS = 1 << 26;             // blocks of one launch: gridDim.x * blockDim.x stays below 2^32
constexpr int CLG_UNVISITED = 0, CLG_NOISE = -1;      // dbscan.py

// asep_cluster_setting (include/asep_hip.h)
struct ClgSetting {
    int32_t min_neighbors, assign_noise;
    double conf_thr, agree_thr;
};

__device__ __forceinline__ int clg_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// number of j != i with conf[i, j] > thr (region_query's length), lanes striding over the row
template <class T>
__device__ __forceinline__ int clg_reach_count(const T* __restrict__ row, int n, int i, T thr, int lane) {
    int cnt = 0;
    for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
        const int j = j0 + lane;
        const bool hit = j < n && j != i && row[j] > thr;
        cnt += __popcll(__ballot(hit));
    }
    return clg_uniform(cnt);
}

// grid n_pages * n_settings blocks of one wave, the settings of a page next to each other (they read the same matrix).
// Dynamic LDS: max_n member values (T), max_n labels, max_n queued owners.  Page k has the nodes node_off[k] ..
// node_off[k+1]-1 and its matrix at conf + conf_off[k]; out_labels [n_settings][node_off[n_pages]].
template <class T>
__global__ void __launch_bounds__(CLG_WAVE) cluster_grid_kernel(const T* __restrict__ conf, const int64_t* __restrict__ conf_off,
                                                                const int32_t* __restrict__ node_off,
                                                                const ClgSetting* __restrict__ settings, int n_settings, int n_pages,
                                                                int max_n, int32_t* __restrict__ out_labels) {
    extern __shared__ __align__(16) unsigned char clg_lds[];
    T* vals = (T*)clg_lds;
    int32_t* labels = (int32_t*)(vals + max_n);
    int32_t* queue = labels + max_n;

    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_settings, s = blockIdx.x % n_settings;
    const int n0 = node_off[page], n = node_off[page + 1] - n0;
    const T* __restrict__ m = conf + conf_off[page];
    const ClgSetting st = settings[s];
    const T conf_thr = (T)st.conf_thr, agree_thr = (T)st.agree_thr;   // numpy compares an array with a Python float in the array's dtype
    const int min_nb = st.min_neighbors;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;

    int32_t* out = out_labels + (size_t)s * node_off[n_pages] + n0;
    if (n == 2) {       // TextblockClustering.calc: two nodes are one article iff conf[0, 1] >= confidence_threshold, no clustering
        if (lane < 2) out[lane] = (lane == 0 || m[1] >= conf_thr) ? 1 : 2;
        return;
    }
    for (int i = lane; i < n; i += CLG_WAVE) labels[i] = CLG_UNVISITED;
    __syncthreads();

    int label = 0;
    for (int node = 0; node < n; ++node) {
        if (labels[node] != CLG_UNVISITED) continue;                  // (one address: the same value in every lane)
        if (clg_reach_count(m + (size_t)node * n, n, node, conf_thr, lane) < min_nb) {
            if (lane == 0) labels[node] = CLG_NOISE;
            __syncthreads();
            continue;
        }
        ++label;
        if (lane == 0) {
            labels[node] = label;
            queue[0] = node;
        }
        __syncthreads();
        // grow_cluster: the frontier is reach(seed) followed by reach(c) of every accepted owner c, in acceptance order;
        // an owner enters the queue once (it leaves UNVISITED when it does), so the queue holds at most n owners
        int q_len = 1;
        for (int q = 0; q < q_len; ++q) {
            const int owner = queue[q];
            const T* __restrict__ orow = m + (size_t)owner * n;
            for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
                const int j = j0 + lane;
                // a node that carries a label keeps it: only NOISE / UNVISITED candidates can still be taken
                const bool hit = j < n && j != owner && orow[j] > conf_thr && labels[j] <= 0;
                unsigned long long todo = __ballot(hit);
                while (todo) {
                    const int cand = j0 + (int)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    const int state = labels[cand];
                    if (state != CLG_NOISE && state != CLG_UNVISITED) continue;     // taken meanwhile, earlier in this row
                    // validate_cluster_agreement: the candidate's confidences to the members, ascending, then np.mean
                    const T* __restrict__ crow = m + (size_t)cand * n;
                    int n_mem = 0;
                    for (int k0 = 0; k0 < n; k0 += CLG_WAVE) {
                        const int k = k0 + lane;
                        const bool mem = k < n && labels[k] == label;
                        const unsigned long long mm = __ballot(mem);
                        if (mem) vals[n_mem + __popcll(mm & lanes_below)] = crow[k];
                        n_mem += __popcll(mm);
                    }
                    __syncthreads();
                    const bool agree = np_mean(vals, n_mem) > agree_thr;
                    __syncthreads();                                   // vals are read before the next gather overwrites them
                    if (!agree) continue;
                    bool expand = false;
                    if (state == CLG_UNVISITED) expand = clg_reach_count(crow, n, cand, conf_thr, lane) >= min_nb;
                    if (lane == 0) {
                        labels[cand] = label;
                        if (expand) queue[q_len] = cand;
                    }
                    if (expand) ++q_len;
                    __syncthreads();
                }
            }
        }
    }
    // create_clusters_for_noise_nodes: fresh labels in index order
    if (st.assign_noise) {
        for (int j0 = 0; j0 < n; j0 += CLG_WAVE) {
            const int j = j0 + lane;
            const bool noise = j < n && labels[j] == CLG_NOISE;
            const unsigned long long nm = __ballot(noise);
            if (noise) labels[j] = label + 1 + __popcll(nm & lanes_below);
            label += __popcll(nm);
        }
        __syncthreads();
    }
    for (int i = lane; i < n; i += CLG_WAVE) out[i] = labels[i];
}

// The counts of as_eval.SepPageBlComper for one (page, setting) per wave, over the labels the kernel above wrote.  Page
// k has the lines line_off[k] .. line_off[k+1]-1: line_node = the node the line hangs in, line_gt = its dense ground
// truth article or -1; and the listed ground truth blocks gtblk_off[k] .. gtblk_off[k+1]-1, block b the lines
// gtblk_lines[gtblk_line_off[b] .. gtblk_line_off[b+1]-1] (indices within the page).  out [n_settings][n_pages] =
// {hypNIs, n_inf, corrects, 0}.  Dynamic LDS: two int arrays of max_n + 2 (labels run from -1 to n).
__global__ void __launch_bounds__(CLG_WAVE) cluster_compare_kernel(const int32_t* __restrict__ labels_all,
                                                                   const int32_t* __restrict__ node_off,
                                                                   const int32_t* __restrict__ line_off,
                                                                   const int32_t* __restrict__ line_node,
                                                                   const int32_t* __restrict__ line_gt,
                                                                   const int32_t* __restrict__ gtblk_off,
                                                                   const int32_t* __restrict__ gtblk_line_off,
                                                                   const int32_t* __restrict__ gtblk_lines, int n_settings,
                                                                   int n_pages, int max_n, int4* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char clg_lds[];
    int32_t* n_lines_of = (int32_t*)clg_lds;          // [label + 1]: lines of the page that carry the label
    int32_t* seen = n_lines_of + max_n + 2;           // [label + 1]: the label occurs in the ground truth article at hand
    const int lane = threadIdx.x;
    const int page = blockIdx.x / n_settings, s = blockIdx.x % n_settings;
    const int n = node_off[page + 1] - node_off[page];
    const int32_t* __restrict__ lab = labels_all + (size_t)s * node_off[n_pages] + node_off[page];
    const int l0 = line_off[page], nl = line_off[page + 1] - l0;
    const int32_t* __restrict__ lnode = line_node + l0;
    const int32_t* __restrict__ lgt = line_gt + l0;

    for (int i = lane; i < n + 2; i += CLG_WAVE) n_lines_of[i] = 0;
    __syncthreads();
    int gt_max = -1;
    for (int i = lane; i < nl; i += CLG_WAVE) {
        atomicAdd(&n_lines_of[lab[lnode[i]] + 1], 1);
        gt_max = max(gt_max, lgt[i]);
    }
    for (int d = 32; d > 0; d >>= 1) gt_max = max(gt_max, __shfl_xor(gt_max, d));
    __syncthreads();
    int hyp = 0;
    for (int i = lane; i < n + 2; i += CLG_WAVE) hyp += n_lines_of[i] > 0;
    // distinct (ground truth article, label) pairs: article by article, the labels of its lines marked and counted
    int inf = 0;
    for (int g = 0; g <= gt_max; ++g) {
        for (int i = lane; i < n + 2; i += CLG_WAVE) seen[i] = 0;
        __syncthreads();
        for (int i = lane; i < nl; i += CLG_WAVE)
            if (lgt[i] == g) seen[lab[lnode[i]] + 1] = 1;
        __syncthreads();
        for (int i = lane; i < n + 2; i += CLG_WAVE) inf += seen[i];
        __syncthreads();
    }
    // a listed block is an article of the hypothesis when its lines share one label and no other line carries it
    int correct = 0;
    for (int b = gtblk_off[page] + lane; b < gtblk_off[page + 1]; b += CLG_WAVE) {
        const int e0 = gtblk_line_off[b], e1 = gtblk_line_off[b + 1];
        if (e1 == e0) continue;
        const int first = lab[lnode[gtblk_lines[e0]]];
        bool same = true;
        for (int e = e0 + 1; e < e1; ++e) same = same && lab[lnode[gtblk_lines[e]]] == first;
        correct += same && n_lines_of[first + 1] == e1 - e0;
    }
    for (int d = 32; d > 0; d >>= 1) {
        hyp += __shfl_xor(hyp, d);
        inf += __shfl_xor(inf, d);
        correct += __shfl_xor(correct, d);
    }
    if (lane == 0) out[(size_t)s * n_pages + page] = make_int4(hyp, inf, correct, 0);
}

#endif  // __HIPCC__

}  // namespace asep
