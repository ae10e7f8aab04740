// sift_cuda::matchList on the GPU (tests/test_gpu_match_list_cxx.py): two
// 256 x 256 frames (a synthetic frame and its copy shifted by (3, 2) pixels) go
// through detectAndCompute, and matchList(prev_descriptor, n0,
// device_descriptor, n1) -- the default filter: ratio 0.8 on distances, cross
// check -- must equal the same rule applied in C++ to the top-2 of both
// directions as the C ABI's sift_hip_match_device returns them (idx2 / d2):
// same records, same order, distance = sqrtf(d2[2 i]).  Also: without the
// cross check and with matchBruteForce's squared ratio the list is
// matchBruteForce's result compacted, and an empty set gives an empty list.
#include <cmath>
#include <cstdio>
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

struct Top2 {
    std::vector<int> idx;  // 2 per row
    std::vector<float> d2;
};

static bool top2(sift_hip_matcher_t m, const sift_cuda::Half* q, int nq, const sift_cuda::Half* t, int nt, Top2& out) {
    void *di = nullptr, *dd = nullptr;
    if (sift_hip_malloc(&di, sizeof(int) * 2 * nq) != SIFT_HIP_OK || sift_hip_malloc(&dd, sizeof(float) * 2 * nq) != SIFT_HIP_OK)
        return false;
    out.idx.resize(2 * (size_t)nq);
    out.d2.resize(2 * (size_t)nq);
    const bool ok = sift_hip_match_device(m, reinterpret_cast<const uint16_t*>(q), nq, reinterpret_cast<const uint16_t*>(t),
                                          nt, 0.8f, 0, static_cast<int*>(di), static_cast<float*>(dd), nullptr,
                                          nullptr) == SIFT_HIP_OK &&
                    sift_hip_device_sync() == SIFT_HIP_OK &&
                    sift_hip_memcpy_d2h(out.idx.data(), di, sizeof(int) * 2 * nq) == SIFT_HIP_OK &&
                    sift_hip_memcpy_d2h(out.d2.data(), dd, sizeof(float) * 2 * nq) == SIFT_HIP_OK;
    sift_hip_free(di);
    sift_hip_free(dd);
    return ok;
}

static bool ratio_pass(const Top2& r, int row, float ratio) {
    if (r.idx[2 * row] < 0) return false;
    if (r.idx[2 * row + 1] < 0) return true;
    const float a = std::sqrt(r.d2[2 * row]), b = std::sqrt(r.d2[2 * row + 1]);
    const float rb = ratio * b;
    return a < rb;
}

int main() {
    const int w = 256, h = 256, dx = 3, dy = 2;
    CudaSiftConfig cfg;
    cfg.col_width = w;
    cfg.row_width = h;
    cfg.upscale = false;
    cfg.numFeatures = 0;
    const int PW = w + dx, PH = h + dy;
    std::vector<float> big((size_t)PW * PH);
    REQUIRE(sift_synth_frame(7, PW, PH, big.data()) == SIFT_HIP_OK);
    sift_cuda::Detector det(cfg);
    REQUIRE(det.gpuWarmUpAndAllocate());
    int n[2] = {0, 0};
    for (int f = 0; f < 2; f++) {
        Imagef img(h, w);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) img.at(y, x) = big[(size_t)(y + f * dy) * PW + x + f * dx];
        det.detectAndCompute(img);
        n[f] = det.total_size;
    }
    const int n0 = n[0], n1 = n[1];
    REQUIRE(n0 > 20 && n1 > 20);

    sift_hip_matcher_t m = nullptr;
    const int cap = n0 > n1 ? n0 : n1;
    REQUIRE(sift_hip_matcher_create(-1, cap, cap, 1, &m) == SIFT_HIP_OK);
    Top2 fwd, rev;
    REQUIRE(top2(m, det.prev_descriptor.data(), n0, det.device_descriptor.data(), n1, fwd));
    REQUIRE(top2(m, det.device_descriptor.data(), n1, det.prev_descriptor.data(), n0, rev));
    REQUIRE(sift_hip_matcher_destroy(m) == SIFT_HIP_OK);

    // the mutual test on the two per-query results
    std::vector<sift_cuda::DMatch> expect;
    int one_way = 0;
    for (int i = 0; i < n0; i++) {
        const int i1 = fwd.idx[2 * i];
        if (i1 < 0 || !ratio_pass(fwd, i, 0.8f)) continue;
        one_way++;
        if (rev.idx[2 * i1] != i) continue;
        expect.push_back(sift_cuda::DMatch{i, i1, 0, std::sqrt(fwd.d2[2 * i])});
    }
    REQUIRE(!expect.empty() && (int)expect.size() < n0);

    const std::vector<sift_cuda::DMatch> got =
        sift_cuda::matchList(det.prev_descriptor, n0, det.device_descriptor, n1);  // the default filter
    REQUIRE(got.size() == expect.size());
    for (size_t k = 0; k < got.size(); k++) {
        REQUIRE(got[k].queryIdx == expect[k].queryIdx && got[k].trainIdx == expect[k].trainIdx);
        REQUIRE(got[k].imgIdx == 0 && got[k].distance == expect[k].distance);
    }

    sift_cuda::MatchFilter plain;
    plain.cross_check = 0;
    const auto ratio_only = sift_cuda::matchList(det.prev_descriptor, n0, det.device_descriptor, n1, plain);
    REQUIRE((int)ratio_only.size() == one_way && ratio_only.size() >= got.size());

    // matchBruteForce's convention (ratio 0.8 on squared distances), compacted
    plain.ratio_on_squared = 1;
    const auto squared = sift_cuda::matchList(det.prev_descriptor, n0, det.device_descriptor, n1, plain);
    const std::vector<int> mb = sift_cuda::matchBruteForce(det.prev_descriptor, n0, det.device_descriptor, n1);
    size_t k = 0;
    for (int i = 0; i < n0; i++) {
        if (mb[i] < 0) continue;
        REQUIRE(k < squared.size() && squared[k].queryIdx == i && squared[k].trainIdx == mb[i]);
        k++;
    }
    REQUIRE(k == squared.size());

    REQUIRE(sift_cuda::matchList(det.prev_descriptor, 0, det.device_descriptor, n1).empty());
    REQUIRE(sift_cuda::matchList(det.prev_descriptor, n0, det.device_descriptor, 0).empty());
    std::printf("match list ok: %zu mutual of %d one-way matches, %d x %d keypoints\n", got.size(), one_way, n0, n1);
    return 0;
}
