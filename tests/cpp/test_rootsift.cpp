// sift_cuda::Detector::setRootSift and sift_cuda::rootSiftDevice / rootSiftHost
// on the GPU (tests/test_gpu_rootsift_cxx.py): on a 256 x 256 synthetic frame
// a root detector's rows equal rootSiftDevice applied to a plain detector's
// copied rows (out of place and in place) and rootSiftHost applied to its host
// rows, keypoints are identical, and the setter throws after the warm-up.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "sift_cuda/Detector.hh"
#include "sift_hip.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

using sift_cuda::Detector;
using sift_cuda::Half;

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

int main() {
    const int w = 256, h = 256;
    CudaSiftConfig cfg;
    cfg.col_width = w;
    cfg.row_width = h;
    cfg.upscale = false;
    cfg.numFeatures = 0;
    Imagef img(h, w);
    REQUIRE(sift_synth_frame(1, w, h, img.m_data->data()) == SIFT_HIP_OK);

    Detector plain(cfg), root(cfg);
    REQUIRE(!root.rootSift());
    root.setRootSift(true);
    REQUIRE(root.rootSift() && !plain.rootSift());
    REQUIRE(plain.gpuWarmUpAndAllocate() && root.gpuWarmUpAndAllocate());
    for (bool v : {false, true}) {  // after the warm-up the norm is part of the graphs
        bool threw = false;
        try {
            root.setRootSift(v);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        REQUIRE(threw && root.rootSift());
    }

    plain.detectAndCompute(img);
    root.detectAndCompute(img);
    plain.copyToHost(true);
    root.copyToHost(true);
    const int n = plain.total_size;
    REQUIRE(n > 50 && root.total_size == n);
    REQUIRE(same(plain.final_kpts, root.final_kpts) && same(plain.final_features, root.final_features));
    REQUIRE(!same(plain.descriptors, root.descriptors));

    const size_t bytes = sizeof(Half) * 128 * (size_t)n;
    void *src = nullptr, *dst = nullptr;
    REQUIRE(sift_hip_malloc(&src, bytes) == SIFT_HIP_OK && sift_hip_malloc(&dst, bytes) == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_d2d(src, plain.device_descriptor.data(), bytes, nullptr) == SIFT_HIP_OK);
    std::vector<Half> got((size_t)n * 128);
    sift_cuda::rootSiftDevice(static_cast<const Half*>(src), n, static_cast<Half*>(dst));
    REQUIRE(sift_hip_memcpy_d2h(got.data(), dst, bytes) == SIFT_HIP_OK);
    REQUIRE(same(got, root.descriptors));
    sift_cuda::rootSiftDevice(static_cast<const Half*>(src), n, static_cast<Half*>(src));  // in place
    REQUIRE(sift_hip_memcpy_d2h(got.data(), src, bytes) == SIFT_HIP_OK);
    REQUIRE(same(got, root.descriptors));
    std::vector<Half> hostOut((size_t)n * 128);
    sift_cuda::rootSiftHost(plain.descriptors.data(), n, hostOut.data());
    REQUIRE(same(hostOut, root.descriptors));

    bool threw = false;
    try {
        sift_cuda::rootSiftDevice(static_cast<const Half*>(src), n, static_cast<Half*>(src) + 128);  // partial overlap
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    REQUIRE(threw);
    sift_hip_free(src);
    sift_hip_free(dst);
    std::printf("rootsift ok: %d rows\n", n);
    return 0;
}
