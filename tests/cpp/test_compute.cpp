// sift_cuda::Detector::compute on the GPU (tests/test_gpu_compute_cxx.py):
// a synthetic frame's own keypoints, handed back through compute(), give the
// bytes detectAndCompute gave -- descriptors, keypoints and features, in the
// same order -- for the float and the 8-bit image; an invalid keypoint and a
// list above the result capacity throw std::invalid_argument and leave the
// results current.
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
using sift_cuda::KeyPoint;

static std::vector<KeyPoint> own_keypoints(const Detector& d) {
    std::vector<KeyPoint> k(d.final_kpts.size());
    for (size_t i = 0; i < k.size(); i++) {
        const auto& p = d.final_kpts[i];
        const auto& f = d.final_features[i];
        k[i] = KeyPoint{p.x, p.y, f.y, f.w, f.z, (int)f.x};
    }
    return k;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

int main() {
    const int w = 257, h = 191;
    CudaSiftConfig cfg;
    cfg.col_width = w;
    cfg.row_width = h;
    cfg.upscale = true;
    cfg.numFeatures = 0;
    Imagef img(h, w);
    REQUIRE(sift_synth_frame(2, w, h, img.m_data->data()) == SIFT_HIP_OK);
    Image8U img8(h, w);
    for (size_t i = 0; i < img.m_data->size(); i++) (*img8.m_data)[i] = (unsigned char)(*img.m_data)[i];

    Detector det(cfg);
    REQUIRE(det.gpuWarmUpAndAllocate());
    det.detectAndCompute(img);
    det.copyToHost(true);
    const int n = det.total_size;
    REQUIRE(n > 20);
    const auto k3 = det.final_kpts;
    const auto f4 = det.final_features;
    const auto desc = det.descriptors;
    const std::vector<KeyPoint> kpts = own_keypoints(det);

    det.compute(img, kpts);
    REQUIRE(det.total_size == n);
    det.copyToHost(true);
    REQUIRE(same(det.descriptors, desc));
    REQUIRE(same(det.final_kpts, k3) && same(det.final_features, f4));

    det.compute(img8, kpts);  // the synthetic frame holds integers: the 8-bit frame is the same frame
    REQUIRE(det.total_size == n);
    det.copyToHost(true);
    REQUIRE(same(det.descriptors, desc));

    // Refused lists throw and leave the last results current.
    std::vector<KeyPoint> bad = kpts;
    bad[3].size = 0.f;
    bool threw = false;
    try {
        det.compute(img, bad);
    } catch (const std::invalid_argument& e) {
        threw = std::strstr(e.what(), "keypoint 3") != nullptr;
    }
    REQUIRE(threw);
    int cap = 0;
    REQUIRE(sift_hip_capacities(det.handle(), nullptr, nullptr, nullptr, &cap) == SIFT_HIP_OK);
    threw = false;
    try {
        det.compute(img, std::vector<KeyPoint>((size_t)cap + 1, kpts[0]));
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    REQUIRE(threw);
    REQUIRE(det.total_size == n);
    det.copyToHost(true);
    REQUIRE(same(det.descriptors, desc));

    det.compute(img, {});
    REQUIRE(det.total_size == 0);
    det.detectAndCompute(img);
    det.copyToHost(true);
    REQUIRE(det.total_size == n && same(det.descriptors, desc) && same(det.final_kpts, k3));
    std::printf("compute ok: %d keypoints\n", n);
    return 0;
}
