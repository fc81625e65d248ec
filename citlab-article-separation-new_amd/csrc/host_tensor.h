// A named tensor of a weight blob on the host.  Plain C++17 without HIP (asep_common.h and aru_pack.h share it).
#pragma once
#include <cstddef>
#include <vector>

namespace asep {

struct HostTensor {
    std::vector<int> dims;
    std::vector<float> data;       // copied out of the caller's blob (payloads may be unaligned)
    size_t count() const {
        size_t n = 1;
        for (int d : dims) n *= (size_t)d;
        return n;
    }
};

}  // namespace asep
