// Host side of the segmentation net evaluation (include/asep_hip.h, "segmentation net evaluation" block): the page table of one scoring
// call, cut into launches of at most MAXP pages (launch_plan.h), the counter blocks, and the blend of a mask over a scan.
#include <string>
#include <vector>

#include "asep_common.h"
#include "launch_plan.h"
#include "seg_eval_kernels.h"

using namespace asep;

static_assert(SEG_MAXC == ASEP_SEG_EVAL_MAX_CLASSES, "the kernels serve the classes the header promises");
static_assert(ASEP_SEG_EVAL_FN + SEG_MAXC <= ASEP_SEG_EVAL_SLOTS, "a page's counter block holds every group");

struct asep_seg_eval {
    unsigned long long* d_cnt = nullptr;   // SEG_DEV_SLOTS counters per page of the largest call so far
    size_t cap_pages = 0;
    std::vector<unsigned long long> h_cnt;
    std::string launches;                  // kernels of the last call, one per line
    double kernel_us = 0.0;
    ~asep_seg_eval() {
        if (d_cnt) (void)hipFree(d_cnt);
    }
};

namespace {

constexpr long long SEG_MAX_VALUES = 1ll << 40;   // H * W * C of one page stays below this

template <int C>
void launch_seg(const SegArgs& a, int grid, bool thr, hipStream_t st) {
    if (thr) hipLaunchKernelGGL((seg_eval_kernel<C, true>), dim3((unsigned)grid), dim3(SEG_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((seg_eval_kernel<C, false>), dim3((unsigned)grid), dim3(SEG_BLOCK), 0, st, a);
}

void launch_seg_c(int C, const SegArgs& a, int grid, bool thr, hipStream_t st) {
    switch (C) {
        case 1: return launch_seg<1>(a, grid, thr, st);
        case 2: return launch_seg<2>(a, grid, thr, st);
        case 3: return launch_seg<3>(a, grid, thr, st);
        case 4: return launch_seg<4>(a, grid, thr, st);
        case 5: return launch_seg<5>(a, grid, thr, st);
        case 6: return launch_seg<6>(a, grid, thr, st);
        case 7: return launch_seg<7>(a, grid, thr, st);
        default: return launch_seg<8>(a, grid, thr, st);
    }
}

}  // namespace

asep_seg_eval* asep_seg_eval_create(void) {
    ASEP_GUARD_BEGIN
    return new asep_seg_eval();
    ASEP_GUARD_END_PTR
}

void asep_seg_eval_free(asep_seg_eval* h) { delete h; }

double asep_seg_eval_last_kernel_us(const asep_seg_eval* h) { return h ? h->kernel_us : 0.0; }

long asep_seg_eval_last_launches(const asep_seg_eval* h, char* buf, size_t max_bytes) {
    if (!h) {
        set_error("asep_seg_eval_last_launches: null handle");
        return ASEP_ERR_ARG;
    }
    if (buf && max_bytes) {
        const size_t n = std::min(max_bytes - 1, h->launches.size());
        memcpy(buf, h->launches.data(), n);
        buf[n] = 0;
    }
    return (long)h->launches.size();
}

int asep_seg_eval_pages_dev(asep_seg_eval* h, int n_pages, const float* const* d_probs, const uint8_t* const* d_gt,
                            uint8_t* const* d_masks, const int32_t* H, const int32_t* W, int C, int mask_threshold,
                            unsigned long long* out_counters, void* stream) {
    if (!h || n_pages < 0 || (n_pages && (!d_probs || !H || !W || !out_counters))) {
        set_error("asep_seg_eval_pages_dev: bad arguments (handle, n_pages %d >= 0, d_probs / H / W / out_counters given)", n_pages);
        return ASEP_ERR_ARG;
    }
    if (C < 1) {
        set_error("asep_seg_eval_pages_dev: C = %d: a net output has at least one class", C);
        return ASEP_ERR_ARG;
    }
    if (C > SEG_MAXC) {
        set_error("asep_seg_eval_pages_dev: C = %d: the scoring kernel is built for 1 .. %d classes", C, SEG_MAXC);
        return ASEP_ERR_UNSUPPORTED;
    }
    for (int b = 0; b < n_pages; ++b) {
        if (H[b] < 1 || W[b] < 1) {
            set_error("asep_seg_eval_pages_dev: page %d is %d x %d: a page has at least one pixel", b, H[b], W[b]);
            return ASEP_ERR_ARG;
        }
        if ((long long)H[b] * W[b] * C >= SEG_MAX_VALUES) {
            set_error("asep_seg_eval_pages_dev: page %d is %d x %d x %d: a page holds fewer than 2^40 values", b, H[b], W[b], C);
            return ASEP_ERR_UNSUPPORTED;
        }
        if (!d_probs[b]) {
            set_error("asep_seg_eval_pages_dev: page %d has no probabilities (null pointer)", b);
            return ASEP_ERR_ARG;
        }
        if (d_gt) {
            int given = 0;
            for (int c = 0; c < C; ++c) given += d_gt[(size_t)b * C + c] != nullptr;
            if (given != 0 && given != C) {
                set_error("asep_seg_eval_pages_dev: page %d has %d of %d ground truth planes: all of a page's planes or none", b, given, C);
                return ASEP_ERR_ARG;
            }
        }
    }
    ASEP_GUARD_BEGIN
    h->launches.clear();
    h->kernel_us = 0.0;
    if (n_pages == 0) return ASEP_OK;
    // the launches' block numbering first: nothing is queued for a call that cannot be served
    struct Launch { SegArgs a; int grid; };
    std::vector<Launch> plan(num_chunks((size_t)n_pages));
    for (size_t c = 0; c < plan.size(); ++c) {
        SegArgs& a = plan[c].a;
        a = SegArgs{};
        uint64_t total = 0;
        for (size_t b = chunk_begin(c); b < chunk_end((size_t)n_pages, c); ++b) {
            SegProb& p = a.p[b - chunk_begin(c)];
            p.npix = (long long)H[b] * W[b];
            p.blk_begin = (int)total;
            total += ((uint64_t)p.npix + SEG_UNIT - 1) / SEG_UNIT;
            if (total > (uint64_t)INT32_MAX) {
                set_error("asep_seg_eval_pages_dev: pages %zu .. %zu need more than 2^31 - 1 blocks in one launch", chunk_begin(c), b);
                return ASEP_ERR_UNSUPPORTED;
            }
        }
        a.nprob = (int)(chunk_end((size_t)n_pages, c) - chunk_begin(c));
        plan[c].grid = (int)total;
    }
    hipStream_t st = (hipStream_t)stream;
    if ((size_t)n_pages > h->cap_pages) {
        if (h->d_cnt) {
            ASEP_HIP_CHECK(hipStreamSynchronize(st));
            (void)hipFree(h->d_cnt);
            h->d_cnt = nullptr, h->cap_pages = 0;
        }
        ASEP_HIP_CHECK(hipMalloc((void**)&h->d_cnt, (size_t)n_pages * SEG_DEV_SLOTS * sizeof(unsigned long long)));
        h->cap_pages = (size_t)n_pages;
    }
    const size_t cnt_bytes = (size_t)n_pages * SEG_DEV_SLOTS * sizeof(unsigned long long);
    ASEP_HIP_CHECK(hipMemsetAsync(h->d_cnt, 0, cnt_bytes, st));
    for (size_t c = 0; c < plan.size(); ++c)
        for (size_t b = chunk_begin(c); b < chunk_end((size_t)n_pages, c); ++b) {
            SegProb& p = plan[c].a.p[b - chunk_begin(c)];
            p.prob = d_probs[b];
            p.vec = ((uintptr_t)d_probs[b] & 15) == 0;
            for (int k = 0; k < C; ++k) p.gt[k] = d_gt ? d_gt[b * C + k] : nullptr;
            p.masks = d_masks ? d_masks[b] : nullptr;
            p.cnt = h->d_cnt + b * SEG_DEV_SLOTS;
        }
    const std::string name = "seg_eval_kernel<" + std::to_string(C) + (mask_threshold ? ",true>" : ",false>");
    KernelTimer tm;
    tm.start(st);
    for (const Launch& l : plan) {
        launch_seg_c(C, l.a, l.grid, mask_threshold != 0, st);
        ASEP_HIP_CHECK(hipGetLastError());
        h->launches += name + "\n";
    }
    tm.stop(st);
    h->h_cnt.resize((size_t)n_pages * SEG_DEV_SLOTS);
    ASEP_HIP_CHECK(hipMemcpyAsync(h->h_cnt.data(), h->d_cnt, cnt_bytes, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    tm.read(h->kernel_us);
    for (int b = 0; b < n_pages; ++b) {
        const unsigned long long* d = h->h_cnt.data() + (size_t)b * SEG_DEV_SLOTS;
        unsigned long long* o = out_counters + (size_t)b * ASEP_SEG_EVAL_SLOTS;
        for (int i = 0; i < ASEP_SEG_EVAL_SLOTS; ++i) o[i] = 0;
        o[ASEP_SEG_EVAL_UNSURE] = d[SEG_D_UNSURE];
        o[ASEP_SEG_EVAL_PIXELS] = (unsigned long long)H[b] * (unsigned long long)W[b];
        const bool has_gt = d_gt && d_gt[(size_t)b * C] != nullptr;
        o[ASEP_SEG_EVAL_HAS_GT] = has_gt;
        for (int c = 0; c < C; ++c) {
            o[ASEP_SEG_EVAL_CLASS + c] = d[SEG_D_CLASS + c];
            if (!has_gt) continue;
            o[ASEP_SEG_EVAL_EQUAL + c] = d[SEG_D_EQUAL + c];
            o[ASEP_SEG_EVAL_TP + c] = d[SEG_D_TP + c];
            o[ASEP_SEG_EVAL_FP + c] = d[SEG_D_CLASS + c] - d[SEG_D_TP + c];      // arg max is c, gt is not 255
            o[ASEP_SEG_EVAL_FN + c] = d[SEG_D_GT + c] - d[SEG_D_TP + c];         // gt is 255, arg max is not c
        }
    }
    return ASEP_OK;
    ASEP_GUARD_END
}

int asep_seg_eval_blend_dev(asep_seg_eval* h, const uint8_t* d_scan, const uint8_t* d_mask, int H, int W, int r, int g, int b,
                            uint8_t* d_out, void* stream) {
    if (!h || !d_scan || !d_mask || !d_out || H < 1 || W < 1) {
        set_error("asep_seg_eval_blend_dev: bad arguments (handle, scan, mask and out given, %d x %d >= 1 x 1)", H, W);
        return ASEP_ERR_ARG;
    }
    if (r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255) {
        set_error("asep_seg_eval_blend_dev: colour (%d, %d, %d): bytes are expected", r, g, b);
        return ASEP_ERR_ARG;
    }
    const long long npix = (long long)H * W;
    const long long blocks = (npix + SEG_BLOCK * SEG_PIX - 1) / (SEG_BLOCK * SEG_PIX);
    if (blocks > INT32_MAX) {
        set_error("asep_seg_eval_blend_dev: %d x %d needs more than 2^31 - 1 blocks", H, W);
        return ASEP_ERR_UNSUPPORTED;
    }
    ASEP_GUARD_BEGIN
    const SegBlendArgs a{d_scan, d_mask, d_out, npix, {(uint32_t)r, (uint32_t)g, (uint32_t)b}};
    hipLaunchKernelGGL(seg_blend_kernel, dim3((unsigned)blocks), dim3(SEG_BLOCK), 0, (hipStream_t)stream, a);
    ASEP_HIP_CHECK(hipGetLastError());
    h->launches += "seg_blend_kernel\n";
    return ASEP_OK;
    ASEP_GUARD_END
}
