// sift_cuda::Detector::detectAndCompute(image, mask) on the GPU
// (tests/test_gpu_mask_cxx.py): on a 256 x 256 synthetic frame the two host
// overloads (Imagef, Image8U) and the device overload return the unmasked
// result with the masked-out rows deleted -- keypoints, features and
// descriptor bytes, in the same order -- where a row is deleted when
// mask[(int)(y + 0.5f)][(int)(x + 0.5f)] == 0; a mask of the wrong size throws
// std::invalid_argument and leaves the results current.
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

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

struct Rows {
    std::vector<sift_cuda::Float3> k3;
    std::vector<sift_cuda::Float4> f4;
    std::vector<sift_cuda::Half> desc;
};

static Rows rows_of(Detector& d) {
    d.copyToHost(true);
    return Rows{d.final_kpts, d.final_features, d.descriptors};
}

static bool same_rows(const Rows& a, const Rows& b) { return same(a.k3, b.k3) && same(a.f4, b.f4) && same(a.desc, b.desc); }

int main() {
    const int w = 256, h = 256;
    CudaSiftConfig cfg;
    cfg.col_width = w;
    cfg.row_width = h;
    cfg.upscale = false;
    cfg.numFeatures = 60;  // retainBest active: the mask acts on the 60 best
    Imagef img(h, w);
    REQUIRE(sift_synth_frame(1, w, h, img.m_data->data()) == SIFT_HIP_OK);
    Image8U img8(h, w);
    for (size_t i = 0; i < img.m_data->size(); i++) (*img8.m_data)[i] = (unsigned char)(*img.m_data)[i];
    Image8U mask(h, w);  // a diagonal split, values 0 and 3
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) mask.at(y, x) = x + y < w ? 3 : 0;

    Detector det(cfg);
    REQUIRE(det.gpuWarmUpAndAllocate());
    det.detectAndCompute(img);
    const Rows full = rows_of(det);
    const int n = det.total_size;
    REQUIRE(n >= 60);
    Rows exp;
    for (int i = 0; i < n; i++) {
        if (!mask.at((int)(full.k3[i].y + 0.5f), (int)(full.k3[i].x + 0.5f))) continue;
        exp.k3.push_back(full.k3[i]);
        exp.f4.push_back(full.f4[i]);
        exp.desc.insert(exp.desc.end(), full.desc.begin() + (size_t)i * 128, full.desc.begin() + (size_t)(i + 1) * 128);
    }
    const int kept = (int)exp.k3.size();
    REQUIRE(kept > 0 && kept < n);

    det.detectAndCompute(img, mask);
    REQUIRE(det.total_size == kept);
    REQUIRE(same_rows(rows_of(det), exp));
    const Detector::HostResults hr = det.hostResults(true);
    REQUIRE(hr.count == kept && std::memcmp(hr.descriptors, exp.desc.data(), sizeof(sift_cuda::Half) * 128 * kept) == 0);

    det.detectAndCompute(img8, mask);  // the synthetic frame holds integers: the 8-bit frame is the same frame
    REQUIRE(det.total_size == kept);
    REQUIRE(same_rows(rows_of(det), exp));

    void *dimg = nullptr, *dmask = nullptr;
    REQUIRE(sift_hip_malloc(&dimg, sizeof(float) * w * h) == SIFT_HIP_OK && sift_hip_malloc(&dmask, (size_t)w * h) == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_h2d(dimg, img.m_data->data(), sizeof(float) * w * h) == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_h2d(dmask, mask.m_data->data(), (size_t)w * h) == SIFT_HIP_OK);
    det.detectAndComputeDevice(dimg, sizeof(float) * w, false, static_cast<const uint8_t*>(dmask), (size_t)w);
    REQUIRE(det.total_size == kept);
    REQUIRE(same_rows(rows_of(det), exp));
    det.detectAndComputeDevice(dimg, sizeof(float) * w, false, nullptr, 0);  // a null mask: the unmasked call
    REQUIRE(det.total_size == n);
    REQUIRE(same_rows(rows_of(det), full));

    // A mask of the wrong size throws and leaves the last results current.
    for (const Image8U& bad : {Image8U(h, w + 1), Image8U(h - 1, w), Image8U()}) {
        bool threw = false;
        try {
            det.detectAndCompute(img, bad);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        REQUIRE(threw);
        threw = false;
        try {
            det.detectAndCompute(img8, bad);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        REQUIRE(threw);
    }
    REQUIRE(det.total_size == n);
    REQUIRE(same_rows(rows_of(det), full));
    sift_hip_free(dimg);
    sift_hip_free(dmask);
    std::printf("mask ok: %d of %d keypoints kept\n", kept, n);
    return 0;
}
