// sift_cuda::matchKnn / matchKnnList on the GPU (tests/test_gpu_match_knn_cxx.py):
// two 256 x 256 frames (a synthetic frame and its copy shifted by (3, 2) pixels)
// go through detectAndCompute; the descriptor rows of both are read back and the
// k nearest neighbours of every prev_descriptor row are computed here by brute
// force on exact integer distances, ties to the lower train index.  matchKnn(k =
// 5) must return those rows with distance = sqrtf(d^2); matchKnnList(k = 3,
// max_distance) the same neighbours within the cap as one flat list in (queryIdx,
// rank) order; k = 1 the nearest neighbour of matchList without a filter; a k
// outside 1..8 throws, and empty sets give empty results.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <utility>
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

// fp16 bits of an integer 0..255 (what the detector writes) -> its value.
static int half_to_int(uint16_t h) {
    if (h == 0) return 0;
    const int e = (h >> 10) & 31, m = h & 1023;
    return (int)std::ldexp((double)(1024 + m), e - 25);
}

static bool rows(const sift_cuda::Half* dev, int n, std::vector<int>& out) {
    std::vector<uint16_t> raw((size_t)n * 128);
    if (sift_hip_memcpy_d2h(raw.data(), dev, raw.size() * 2) != SIFT_HIP_OK) return false;
    out.resize(raw.size());
    for (size_t i = 0; i < raw.size(); i++) out[i] = half_to_int(raw[i]);
    return true;
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
    REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
    std::vector<int> q, t;
    REQUIRE(rows(det.prev_descriptor.data(), n0, q) && rows(det.device_descriptor.data(), n1, t));

    // the rule, by brute force: (d^2, train index) ascending
    std::vector<std::vector<std::pair<int, int>>> order((size_t)n0);
    for (int i = 0; i < n0; i++) {
        for (int j = 0; j < n1; j++) {
            int d = 0;
            for (int c = 0; c < 128; c++) {
                const int e = q[(size_t)i * 128 + c] - t[(size_t)j * 128 + c];
                d += e * e;
            }
            order[(size_t)i].push_back({d, j});
        }
        std::sort(order[(size_t)i].begin(), order[(size_t)i].end());
    }

    const int k = 5;
    const auto knn = sift_cuda::matchKnn(det.prev_descriptor, n0, det.device_descriptor, n1, k);
    REQUIRE((int)knn.size() == n0);
    for (int i = 0; i < n0; i++) {
        REQUIRE((int)knn[(size_t)i].size() == std::min(k, n1));
        for (int j = 0; j < (int)knn[(size_t)i].size(); j++) {
            const sift_cuda::DMatch& m = knn[(size_t)i][(size_t)j];
            REQUIRE(m.queryIdx == i && m.imgIdx == 0 && m.trainIdx == order[(size_t)i][(size_t)j].second);
            REQUIRE(m.distance == std::sqrt((float)order[(size_t)i][(size_t)j].first));
        }
    }

    // the capped list: a cap at the median nearest distance keeps some and drops some
    std::vector<float> nearest;
    for (int i = 0; i < n0; i++) nearest.push_back(std::sqrt((float)order[(size_t)i][0].first));
    std::sort(nearest.begin(), nearest.end());
    const float cap = nearest[nearest.size() / 2];
    std::vector<sift_cuda::DMatch> expect;
    for (int i = 0; i < n0; i++)
        for (int j = 0; j < 3 && j < n1; j++) {
            const float d = std::sqrt((float)order[(size_t)i][(size_t)j].first);
            if (d <= cap) expect.push_back(sift_cuda::DMatch{i, order[(size_t)i][(size_t)j].second, 0, d});
        }
    REQUIRE(!expect.empty() && (int)expect.size() < 3 * n0);
    const auto list = sift_cuda::matchKnnList(det.prev_descriptor, n0, det.device_descriptor, n1, 3, cap);
    REQUIRE(list.size() == expect.size());
    REQUIRE(std::memcmp(list.data(), expect.data(), sizeof(sift_cuda::DMatch) * list.size()) == 0);
    REQUIRE((int)sift_cuda::matchKnnList(det.prev_descriptor, n0, det.device_descriptor, n1, 8).size() ==
            n0 * std::min(8, n1));

    // k = 1 is the nearest neighbour of an unfiltered matchList
    sift_cuda::MatchFilter none;
    none.ratio = 0.f;
    none.cross_check = 0;
    const auto nn = sift_cuda::matchList(det.prev_descriptor, n0, det.device_descriptor, n1, none);
    const auto one = sift_cuda::matchKnnList(det.prev_descriptor, n0, det.device_descriptor, n1, 1);
    REQUIRE(nn.size() == one.size() && std::memcmp(nn.data(), one.data(), sizeof(sift_cuda::DMatch) * nn.size()) == 0);

    for (int bad : {0, 9, -1}) {
        bool thrown = false;
        try {
            (void)sift_cuda::matchKnn(det.prev_descriptor, n0, det.device_descriptor, n1, bad);
        } catch (const std::invalid_argument&) {
            thrown = true;
        }
        REQUIRE(thrown);
    }
    REQUIRE(sift_cuda::matchKnn(det.prev_descriptor, 0, det.device_descriptor, n1, 3).empty());
    REQUIRE(sift_cuda::matchKnnList(det.prev_descriptor, n0, det.device_descriptor, 0, 3).empty());
    const auto empty_rows = sift_cuda::matchKnn(det.prev_descriptor, n0, det.device_descriptor, 0, 3);
    REQUIRE((int)empty_rows.size() == n0 && empty_rows[0].empty());
    std::printf("match knn ok: %zu of %d capped neighbours, %d x %d keypoints\n", list.size(), 3 * n0, n0, n1);
    return 0;
}
