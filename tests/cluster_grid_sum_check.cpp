// np_mean of csrc/cluster_grid_kernels.h on the host (tests/test_cluster_grid_host.py): reads rows of `width` values of
// type f32 or f64 from a raw file and writes, for every row and every length n = 1 .. width, np_mean(row, n) to another.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cluster_grid_kernels.h"

template <class T>
static int run(const char* in_path, const char* out_path, int width) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return 2;
    std::vector<T> data;
    T buf[256];
    size_t got;
    while ((got = std::fread(buf, sizeof(T), 256, f)) > 0) data.insert(data.end(), buf, buf + got);
    std::fclose(f);
    if (width <= 0 || data.size() % (size_t)width) return 3;
    std::vector<T> out;
    for (size_t r = 0; r < data.size() / (size_t)width; ++r)
        for (int n = 1; n <= width; ++n) out.push_back(asep::np_mean(data.data() + r * (size_t)width, n));
    f = std::fopen(out_path, "wb");
    if (!f) return 4;
    std::fwrite(out.data(), sizeof(T), out.size(), f);
    std::fclose(f);
    std::printf("cluster grid sum ok: %zu means\n", out.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 5) return 1;
    const int width = std::atoi(argv[4]);
    return std::strcmp(argv[1], "f64") == 0 ? run<double>(argv[2], argv[3], width) : run<float>(argv[2], argv[3], width);
}
