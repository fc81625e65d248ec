// Heading detection grid scoring (heading_evaluation.py / heading_evaluation_grid_search.py of the reference): one lane
// per setting, one block column per page.  The fusion rule of heading_net_post_processor.py:110-195 (as restated by
// apply_heading_values) on already normalised per-line confidences, the region rule behind it, and the four counts of
// the region labels against the ground truth.  Compiled with -ffp-contract=off: every double is the one Python computes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asep {

constexpr int HEVAL_BLOCK = 256;       // settings per block
constexpr int HEVAL_CHUNK = 512;       // region-ordered line entries staged in LDS at a time (16 KiB)
constexpr int HEVAL_FIELDS = 9;        // threshold, net_w, sw_w, th_w, net_thresh, sw_thresh, th_thresh, sw_th_thresh, tlp

// One line as a member of a region: the three confidences and whether the line already carries the heading tag.
struct HevalEntry {
    double sw, th, net;
    int32_t tagged, pad;
};

// grid (ceil(n_settings / HEVAL_BLOCK), n_pages).  Page k owns the regions reg_page_off[k] .. reg_page_off[k+1]-1;
// region r owns the entries reg_ent_off[r] .. reg_ent_off[r+1]-1 (its lines in order, a line listed once per region
// that holds it).  out[s][k] = {TP, FP, FN, TN} of the region labels of setting s on page k.
__global__ void __launch_bounds__(HEVAL_BLOCK) heval_grid_kernel(const HevalEntry* __restrict__ ent,
                                                                 const int32_t* __restrict__ reg_ent_off,
                                                                 const int32_t* __restrict__ reg_page_off,
                                                                 const uint8_t* __restrict__ gt, const uint8_t* __restrict__ use_swt,
                                                                 const int32_t* __restrict__ settings, int n_settings, int n_pages,
                                                                 int4* __restrict__ out) {
    __shared__ HevalEntry s_ent[HEVAL_CHUNK];
    const int page = blockIdx.y;
    const int s = blockIdx.x * HEVAL_BLOCK + threadIdx.x;
    const bool live = s < n_settings;
    const int32_t* st = settings + (size_t)(live ? s : 0) * HEVAL_FIELDS;
    // tenths -> doubles as Python does: k / 10 as a division; the text height weight is (10 - nw - sww) / 10
    const double thr = st[0] / 10.0, nw = st[1] / 10.0, sww = st[2] / 10.0, thw = st[3] / 10.0;
    const double nt = st[4] / 10.0, swt = st[5] / 10.0, tht = st[6] / 10.0, swth = st[7] / 10.0, tlp = st[8] / 10.0;
    const bool net_off = st[1] == 0;   // net weight 0: every net confidence is 0 (:102-104), the net clause included
    const bool swt_on = use_swt[page] != 0;

    const int r0 = reg_page_off[page], r1 = reg_page_off[page + 1];
    const int e_end = reg_ent_off[r1];
    int c0 = reg_ent_off[r0], c1 = c0; // entries [c0, c1) are in LDS
    int tp = 0, fp = 0, fn = 0, tn = 0;
    for (int r = r0; r < r1; ++r) {    // uniform over the block: the barriers below are reached by every lane
        const int e0 = reg_ent_off[r], e1 = reg_ent_off[r + 1];
        int n_head = 0;
        for (int e = e0; e < e1; ++e) {
            if (e >= c1) {
                __syncthreads();
                c0 = e;
                c1 = min(e + HEVAL_CHUNK, e_end);
                for (int i = threadIdx.x; i < c1 - c0; i += HEVAL_BLOCK) s_ent[i] = ent[c0 + i];
                __syncthreads();
            }
            const HevalEntry& x = s_ent[e - c0];
            const double net = net_off ? 0.0 : x.net;
            double conf;
            if (swt_on) {
                const double sw = x.sw, th = x.th;
                if (sw >= swt || th >= tht || (sw + th) / 2.0 >= swth || net >= nt)
                    conf = 1.0;
                else
                    conf = nw * net + sww * sw + thw * th;     // left to right, no contraction
            } else {
                conf = net;
            }
            n_head += (x.tagged || conf > thr) ? 1 : 0;
        }
        const int n_lines = e1 - e0;
        const bool hyp = n_lines > 0 && (double)n_head / (double)n_lines >= tlp;
        const bool truth = gt[r] != 0;
        tp += hyp && truth;
        fp += hyp && !truth;
        fn += !hyp && truth;
        tn += !hyp && !truth;
    }
    if (live) out[(size_t)s * n_pages + page] = make_int4(tp, fp, fn, tn);
}

}  // namespace asep
