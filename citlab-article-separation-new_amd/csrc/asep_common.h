// Shared host-side helpers of libasep_hip.so (error reporting, weight-blob parsing, device buffers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/asep_hip.h"
#include "host_tensor.h"

namespace asep {

void set_error(const char* fmt, ...);
const char* get_error();
void warn_ignored_switches();   // stderr, once per process: ASEP_* switches of earlier rounds that this build no longer reads

#define ASEP_HIP_CHECK(expr)                                                                    \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            asep::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                            __LINE__);                                                          \
            return ASEP_ERR_HIP;                                                                \
        }                                                                                       \
    } while (0)

#define ASEP_HIP_CHECK_THROW(expr)                                                              \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            asep::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                            __LINE__);                                                          \
            throw asep::HipError();                                                             \
        }                                                                                       \
    } while (0)

struct HipError {};
struct ArgError {};

// Every extern "C" entry runs its body between these two: no C++ exception (HipError / ArgError of the helpers,
// std::bad_alloc or std::length_error of the std::vector / std::map / std::string code) crosses the C ABI.
#define ASEP_GUARD_BEGIN try {
#define ASEP_GUARD_END_WITH(HIP_RC, ARG_RC)                                                     \
    }                                                                                           \
    catch (const asep::HipError&) { return HIP_RC; }                                            \
    catch (const asep::ArgError&) { return ARG_RC; }                                            \
    catch (const std::bad_alloc&) {                                                             \
        asep::set_error("%s: out of host memory", __func__);                                    \
        return HIP_RC;                                                                          \
    }                                                                                           \
    catch (const std::exception& e) {                                                           \
        asep::set_error("%s: exception: %s", __func__, e.what());                               \
        return HIP_RC;                                                                          \
    }                                                                                           \
    catch (...) {                                                                               \
        asep::set_error("%s: unknown exception", __func__);                                     \
        return HIP_RC;                                                                          \
    }
#define ASEP_GUARD_END ASEP_GUARD_END_WITH(ASEP_ERR_HIP, ASEP_ERR_ARG)
#define ASEP_GUARD_END_PTR ASEP_GUARD_END_WITH(nullptr, nullptr)

// Parses the "ASEPW001" container (weights.py).  Returns false (and sets the error) on malformed input.
bool parse_blob(const void* blob, size_t nbytes, std::map<std::string, HostTensor>& out);

// Buffers requested in a deterministic order by a forward pass; re-used across calls.
class BufferPool {
public:
    ~BufferPool() { release(); }
    void begin() { next_ = 0; }
    void* get(size_t bytes);   // throws HipError
    void release();
    size_t total_bytes() const;
private:
    struct Buf { void* p; size_t n; };
    std::vector<Buf> bufs_;
    size_t next_ = 0;
};

// n elements of host memory in the pool's next buffer (never an empty request); throws HipError
template <class T>
T* upload(BufferPool& pool, hipStream_t st, const T* src, size_t n) {
    T* d = (T*)pool.get((n ? n : 1) * sizeof(T));
    if (n) ASEP_HIP_CHECK_THROW(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return d;
}

// Device time between start and stop on one stream, read once the stream has been synchronised; throws HipError
struct KernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~KernelTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void start(hipStream_t st) {
        ASEP_HIP_CHECK_THROW(hipEventCreate(&e0));
        ASEP_HIP_CHECK_THROW(hipEventCreate(&e1));
        ASEP_HIP_CHECK_THROW(hipEventRecord(e0, st));
    }
    void stop(hipStream_t st) { ASEP_HIP_CHECK_THROW(hipEventRecord(e1, st)); }
    void read(double& us) {
        float ms = 0.f;
        ASEP_HIP_CHECK_THROW(hipEventElapsedTime(&ms, e0, e1));
        us = 1000.0 * ms;
    }
};

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Device pointer + {H, W, C} of a named end point of the last ARU forward (aru_engine.hip); library-internal.
int aru_endpoint_dev(asep_aru* m, const char* name, const float** d_ptr, int dims[3], int* is_bf16 = nullptr);
// Number of channels the end point `name` will have for this model's configuration, or -1 if unknown.
int aru_endpoint_channels(const asep_aru* m, const char* name);
// Number of output classes (channels of the logits / probability map) of the model.
int aru_num_classes(const asep_aru* m);
// Number of image channels a page of the model has (1 = gray, 3 = interleaved RGB).
int aru_input_channels(const asep_aru* m);
// Brackets launches queued on the stream of the model's last forward with one record of its launch profile (asep_aru_profile); begin returns
// nullptr while nothing is recorded, end takes that too.  `name` as rocprofv3 prints the kernel, `detail` the layer text of mode 2.
void* aru_prof_begin(asep_aru* m, const char* name, const char* detail, double flops, double bytes);
void aru_prof_end(void* scope);
// The per-image moments of n pages in two launches over a page table in device memory (launch_plan.h MomentsPage; grid = begin[n]), recorded
// in the model's launch profile; and the statistics a following forward of `m` reads instead of computing its own: stats[b] = page b's
// {mean, 1 / sd} in device memory, nullptr = back to the model's own (aru_engine.hip).
struct MomentsPage;
struct ResizePage;
int aru_moments_pages(asep_aru* m, const MomentsPage* d_pages, const int32_t* d_begin, int n, int grid, hipStream_t st);
void aru_set_page_stats(asep_aru* m, const float* const* stats);
void aru_prof_stream(asep_aru* m, hipStream_t st);      // the stream aru_prof_begin records on, for launches queued IN FRONT of a forward
bool aru_mvn(const asep_aru* m);
// The TF1 bilinear resize of n uint8 scans in one launch over a page table in device memory (post_engine.hip: compiled without contraction)
int resize_tf1_pages_launch(const ResizePage* d_pages, const int32_t* d_begin, int n, int grid, hipStream_t st);
// Stream and buffer pool of an asep_post handle (post_engine.hip), for the entry points of other translation units that run
// on that handle (textblock_engine.hip).
hipStream_t post_stream(asep_post* p);
BufferPool& post_pool(asep_post* p);

}  // namespace asep
