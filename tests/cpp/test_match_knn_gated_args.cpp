// Argument checks of the gated k-NN C++ surface (csrc/match_batched_cxx.cpp: matchKnnGuided, matchKnnEpipolar,
// matchKnnListGuided, matchKnnListEpipolar) and of the C ABI's gated k-NN calls that need no matcher, CPU only (run
// under -fsanitize=address,undefined by tests/test_match_knn_gated_asan.py): a k outside 1..SIFT_HIP_KNN_MAX throws
// std::invalid_argument before anything else is looked at, and the ABI refuses a bad k, a NaN max_distance and every
// defect of a gate with SIFT_HIP_ERR_INVALID and a message naming it, before the matcher is looked at, writing nothing.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

template <class F>
static bool invalid(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    } catch (...) {
    }
    return false;
}

static bool refused(int rc, const char* word) {
    return rc == SIFT_HIP_ERR_INVALID && std::strstr(sift_hip_last_error(), word) != nullptr;
}

int main() {
    std::vector<sift_cuda::Half> rows(4 * 128);  // host memory: never read, the calls below stop before a device call
    std::vector<float> xy(4 * 3, 1.f);
    const sift_cuda::DeviceBuffer<sift_cuda::Half> des(rows.data(), 4), src(rows.data(), 4);
    sift_cuda::MatchGate win;
    win.query_xy = win.train_xy = xy.data();
    win.radius = 5.f;
    sift_cuda::EpipolarGate band;
    band.query_xy = band.train_xy = xy.data();
    band.max_error = 2.f;
    band.F[1] = -1.f, band.F[3] = 1.f;
    for (int k : {0, -1, SIFT_HIP_KNN_MAX + 1, 1 << 30}) {
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnnGuided(des, 4, src, 4, win, k); }));
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnnEpipolar(des, 4, src, 4, band, k); }));
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnnListGuided(des, 4, src, 4, win, k, 1.f); }));
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnnListEpipolar(des, 4, src, 4, band, k, 1.f); }));
    }

    // the C ABI: k, max_distance, then the gate -- none of which needs a matcher or a device
    const uint16_t* q = reinterpret_cast<const uint16_t*>(rows.data());
    int idx[8], count = -7, nq = 1;
    float d2[8];
    sift_hip_dmatch rec[8];
    std::memset(idx, 0x5a, sizeof idx);
    std::memset(d2, 0x5a, sizeof d2);
    std::memset(rec, 0x5a, sizeof rec);
    auto fake = reinterpret_cast<sift_hip_matcher_t>(rows.data());  // never dereferenced by a call refused here
    const float inf = std::numeric_limits<float>::infinity();
    const sift_hip_match_gate g{xy.data(), 3, xy.data(), 3, 5.f};
    sift_hip_match_epipolar_gate e{xy.data(), 3, xy.data(), 3, inf, {0, -1, 0, 1, 0, 0, 0, 0, 0}, 2.f};
    const sift_hip_match_positions pos{xy.data(), xy.data()};
    for (int k : {0, SIFT_HIP_KNN_MAX + 1}) {
        REQUIRE(refused(sift_hip_match_knn_guided_device(fake, q, 1, q, 1, &g, k, idx, d2, nullptr), "k outside"));
        REQUIRE(refused(sift_hip_match_knn_epipolar_host(fake, q, 1, q, 1, &e, k, idx, d2), "k outside"));
        REQUIRE(refused(sift_hip_match_knn_guided_batched(fake, 1, &q, &nq, &q, &nq, &pos, 3, 3, 5.f, k, idx, d2, nullptr),
                        "k outside"));
        REQUIRE(refused(sift_hip_match_knn_list_epipolar_batched(fake, 1, &q, &nq, &q, &nq, &pos, 3, 3, inf, xy.data(), 36,
                                                                 2.f, k, 0.f, rec, &count, nullptr),
                        "k outside"));
        REQUIRE(refused(sift_hip_match_knn_list_guided_host(fake, q, 1, q, 1, &g, k, 0.f, rec, 8, &count), "k outside"));
        count = -7;
    }
    REQUIRE(refused(sift_hip_match_knn_list_guided_device(fake, q, 1, q, 1, &g, 2, NAN, rec, &count, nullptr), "NaN"));
    REQUIRE(refused(sift_hip_match_knn_list_epipolar_device(fake, q, 1, q, 1, &e, 2, NAN, rec, &count, nullptr), "NaN"));
    sift_hip_match_gate bad = g;
    bad.query_stride = 1;
    REQUIRE(refused(sift_hip_match_knn_guided_device(fake, q, 1, q, 1, &bad, 2, idx, d2, nullptr), "stride"));
    bad = g;
    bad.radius = 0.f;
    REQUIRE(refused(sift_hip_match_knn_guided_host(fake, q, 1, q, 1, &bad, 2, idx, d2), "radius"));
    REQUIRE(refused(sift_hip_match_knn_guided_device(fake, q, 1, q, 1, nullptr, 2, idx, d2, nullptr), "gate"));
    sift_hip_match_epipolar_gate be = e;
    be.max_error = inf;
    REQUIRE(refused(sift_hip_match_knn_epipolar_device(fake, q, 1, q, 1, &be, 2, idx, d2, nullptr), "max_error"));
    be = e;
    be.F[4] = NAN;
    REQUIRE(refused(sift_hip_match_knn_epipolar_device(fake, q, 1, q, 1, &be, 2, idx, d2, nullptr), "non-finite"));
    be = e;
    be.F[1] = be.F[3] = 0.f;
    REQUIRE(refused(sift_hip_match_knn_list_epipolar_device(fake, q, 1, q, 1, &be, 2, 0.f, rec, &count, nullptr),
                    "all zero"));
    REQUIRE(refused(sift_hip_match_knn_epipolar_batched(fake, 1, &q, &nq, &q, &nq, &pos, 3, 3, inf, nullptr, 36, 2.f, 2, idx,
                                                        d2, nullptr),
                    "null geometry"));
    for (int stride : {32, 38})
        REQUIRE(refused(sift_hip_match_knn_epipolar_batched(fake, 1, &q, &nq, &q, &nq, &pos, 3, 3, inf, xy.data(), stride,
                                                            2.f, 2, idx, d2, nullptr),
                        "geometry_stride"));
    REQUIRE(refused(sift_hip_match_knn_guided_device(nullptr, q, 1, q, 1, &g, 2, idx, d2, nullptr), "null matcher"));
    REQUIRE(refused(sift_hip_match_knn_epipolar_batched(nullptr, 1, &q, &nq, &q, &nq, &pos, 3, 3, inf, xy.data(), 36, 2.f, 2,
                                                        idx, d2, nullptr),
                    "null matcher"));
    // nothing was written
    for (int i = 0; i < 8; i++) REQUIRE(idx[i] == 0x5a5a5a5a && rec[i].queryIdx == 0x5a5a5a5a);
    REQUIRE(count == -7);
    std::printf("match knn gated args ok\n");
    return 0;
}
