// Host side of the JPEG pixels (include/asep_hip.h, "JPEG pixels" block): checks the frame description against itself, so that nothing
// is indexed by a number the caller's file chose alone, lays the component planes out in the handle's scratch arena and queues the
// two kernels of jpeg_kernels.h.  A translation unit and code object of its own: nothing here touches the net engines.
#include <algorithm>
#include <string>

#include "asep_common.h"
#include "jpeg_kernels.h"

using namespace asep;

namespace {

thread_local std::string g_launches;         // kernels of the calling thread's last call, one name per line

void record(const char* name) { g_launches += name, g_launches += "\n"; }

// the block grid that width, height and sampling imply; false if `in` says anything else
bool consistent(const asep_jpeg_info& in) {
    if (in.width < 1 || in.height < 1 || in.width > 65535 || in.height > 65535) return false;
    if (in.ncomp != 1 && in.ncomp != 3) return false;
    const bool s11 = in.hs == 1 && in.vs == 1, s21 = in.hs == 2 && in.vs == 1, s22 = in.hs == 2 && in.vs == 2;
    if (!(s11 || ((s21 || s22) && in.ncomp == 3))) return false;
    const int mw = (in.width + 8 * in.hs - 1) / (8 * in.hs), mh = (in.height + 8 * in.vs - 1) / (8 * in.vs);
    if (in.mcus_w != mw || in.mcus_h != mh) return false;
    long long blocks = 0;
    for (int c = 0; c < in.ncomp; ++c) {
        if (in.blocks_w[c] != mw * (c == 0 ? in.hs : 1) || in.blocks_h[c] != mh * (c == 0 ? in.vs : 1)) return false;
        if (in.qt_index[c] < 0 || in.qt_index[c] > 3) return false;
        blocks += (long long)in.blocks_w[c] * in.blocks_h[c];
    }
    return in.coef_bytes == blocks * 64 * (long long)sizeof(int16_t);
}

int pixels_dev(asep_post* p, const asep_jpeg_info& in, const int16_t* d_coef, const uint16_t* qt, int order, uint8_t* d_out,
               hipStream_t st) {
    JpegIdctArgs ia{};
    memcpy(ia.qt, qt, sizeof ia.qt);
    ia.ncomp = in.ncomp;
    long long first = 0, plane_bytes = 0;
    uint8_t* planes = nullptr;
    if (in.ncomp == 3) {
        for (int c = 0; c < 3; ++c) plane_bytes += (long long)in.blocks_w[c] * in.blocks_h[c] * 64;
        planes = (uint8_t*)post_pool(p).get((size_t)plane_bytes);
    }
    long long plane_off = 0;
    for (int c = 0; c < in.ncomp; ++c) {
        JpegIdctComp& k = ia.c[c];
        k.coef = d_coef + first * 64;
        k.blocks_w = in.blocks_w[c];
        k.first = (int)first;
        k.qt = in.qt_index[c];
        if (in.ncomp == 1) {
            k.out = d_out, k.stride = in.width, k.crop_w = in.width, k.crop_h = in.height;
        } else {
            k.out = planes + plane_off, k.stride = (long long)in.blocks_w[c] * 8;
            k.crop_w = in.blocks_w[c] * 8, k.crop_h = in.blocks_h[c] * 8;
            plane_off += (long long)in.blocks_w[c] * in.blocks_h[c] * 64;
        }
        first += (long long)in.blocks_w[c] * in.blocks_h[c];
    }
    ia.total = (int)first;                                           // <= 3 * 8192 * 8192 blocks
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(ia.total, JPEG_IDCT_BLOCK)), dim3(JPEG_IDCT_BLOCK), 0, st, ia);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_idct_kernel");
    if (in.ncomp == 1) return ASEP_OK;
    JpegColourArgs ca{};
    ca.y = ia.c[0].out, ca.cb = ia.c[1].out, ca.cr = ia.c[2].out;
    ca.out = d_out;
    ca.y_stride = in.blocks_w[0] * 8, ca.c_stride = in.blocks_w[1] * 8;
    ca.W = in.width, ca.H = in.height;
    ca.hs = in.hs, ca.vs = in.vs;
    ca.dw = (in.width + in.hs - 1) / in.hs, ca.dh = (in.height + in.vs - 1) / in.vs;
    ca.order = order;
    ca.groups_w = cdiv(in.width, JPEG_COLOUR_PIX);
    const long long threads = (long long)ca.groups_w * in.height;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((threads + JPEG_COLOUR_BLOCK - 1) / JPEG_COLOUR_BLOCK)), dim3(JPEG_COLOUR_BLOCK),
                       0, st, ca);
    ASEP_HIP_CHECK(hipGetLastError());
    record("jpeg_colour_kernel");
    return ASEP_OK;
}

int check_args(const char* fn, asep_post* p, const asep_jpeg_info* info, const void* coef, const uint16_t* qt, int order, const void* out) {
    if (!p || !info || !coef || !qt || !out) {
        set_error("%s: null argument", fn);
        return ASEP_ERR_ARG;
    }
    if (order != ASEP_JPEG_ORDER_GRAY && order != ASEP_JPEG_ORDER_BGR && order != ASEP_JPEG_ORDER_RGB) {
        set_error("%s: order %d: ASEP_JPEG_ORDER_GRAY, _BGR and _RGB are served", fn, order);
        return ASEP_ERR_ARG;
    }
    if (!consistent(*info)) {
        set_error("%s: the frame description contradicts itself (%d x %d, %d components, sampling %d x %d, %lld coefficient bytes)", fn,
                  info->width, info->height, info->ncomp, info->hs, info->vs, (long long)info->coef_bytes);
        return ASEP_ERR_ARG;
    }
    return ASEP_OK;
}

size_t out_bytes(const asep_jpeg_info& in, int order) {
    return (size_t)in.width * in.height * (in.ncomp == 1 || order == ASEP_JPEG_ORDER_GRAY ? 1 : 3);
}

}  // namespace

int asep_jpeg_pixels_dev(asep_post* p, const asep_jpeg_info* info, const int16_t* d_coef, const uint16_t* qt, int order, uint8_t* d_out,
                         void* stream) {
    if (int rc = check_args("asep_jpeg_pixels_dev", p, info, d_coef, qt, order, d_out)) return rc;
    ASEP_GUARD_BEGIN
    g_launches.clear();
    post_pool(p).begin();
    return pixels_dev(p, *info, d_coef, qt, order, d_out, (hipStream_t)stream);
    ASEP_GUARD_END
}

int asep_jpeg_pixels(asep_post* p, const asep_jpeg_info* info, const int16_t* coef, const uint16_t* qt, int order, uint8_t* out) {
    if (int rc = check_args("asep_jpeg_pixels", p, info, coef, qt, order, out)) return rc;
    ASEP_GUARD_BEGIN
    hipStream_t st = post_stream(p);
    BufferPool& pool = post_pool(p);
    g_launches.clear();
    pool.begin();
    int16_t* d_coef = (int16_t*)pool.get((size_t)info->coef_bytes);
    const size_t nout = out_bytes(*info, order);
    uint8_t* d_out = (uint8_t*)pool.get(nout);
    ASEP_HIP_CHECK(hipMemcpyAsync(d_coef, coef, (size_t)info->coef_bytes, hipMemcpyHostToDevice, st));
    if (int rc = pixels_dev(p, *info, d_coef, qt, order, d_out, st)) return rc;
    ASEP_HIP_CHECK(hipMemcpyAsync(out, d_out, nout, hipMemcpyDeviceToHost, st));
    ASEP_HIP_CHECK(hipStreamSynchronize(st));
    return ASEP_OK;
    ASEP_GUARD_END
}

long asep_jpeg_last_launches(char* buf, size_t max_bytes) {
    if (buf && max_bytes) {
        const size_t n = std::min(max_bytes - 1, g_launches.size());
        memcpy(buf, g_launches.data(), n);
        buf[n] = 0;
    }
    return (long)g_launches.size();
}
