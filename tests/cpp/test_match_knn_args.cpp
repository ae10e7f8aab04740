// Argument checks of sift_cuda::matchKnn / matchKnnList (csrc/match_batched_cxx.cpp)
// and of the C ABI's k-NN calls that need no matcher, CPU only (run under
// -fsanitize=address,undefined by tests/test_match_knn_asan.py): a k outside
// 1..SIFT_HIP_KNN_MAX throws std::invalid_argument before anything else is
// looked at, empty sets give empty results without a device call, and the ABI
// refuses a bad k, a NaN max_distance and a null matcher with
// SIFT_HIP_ERR_INVALID and a message, writing nothing.
#include <cmath>
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

int main() {
    std::vector<sift_cuda::Half> rows(4 * 128);  // host memory: never read, the calls below stop before a device call
    const sift_cuda::DeviceBuffer<sift_cuda::Half> des(rows.data(), 4), src(rows.data(), 4), none;
    for (int k : {0, -1, SIFT_HIP_KNN_MAX + 1, 1 << 30}) {
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnn(des, 4, src, 4, k); }));
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnnList(des, 4, src, 4, k, 1.f); }));
        REQUIRE(invalid([&] { (void)sift_cuda::matchKnn(none, 0, none, 0, k); }));  // judged before the sizes
    }
    // empty sets: one (empty) row per query, an empty list
    REQUIRE(sift_cuda::matchKnn(none, 0, src, 4, 3).empty());
    const auto rows_of_nothing = sift_cuda::matchKnn(des, 4, none, 0, 3);
    REQUIRE(rows_of_nothing.size() == 4 && rows_of_nothing[0].empty() && rows_of_nothing[3].empty());
    REQUIRE(sift_cuda::matchKnnList(des, 4, none, 0, 3).empty() && sift_cuda::matchKnnList(none, 0, src, 4, 8).empty());

    // the C ABI: k, then max_distance, then the matcher -- none of which needs a device
    const uint16_t* q = reinterpret_cast<const uint16_t*>(rows.data());
    int idx[8], count = -7, nq = 1;
    float d2[8];
    sift_hip_dmatch rec[8];
    std::memset(idx, 0x5a, sizeof idx);
    std::memset(d2, 0x5a, sizeof d2);
    std::memset(rec, 0x5a, sizeof rec);
    auto fake = reinterpret_cast<sift_hip_matcher_t>(rows.data());  // never dereferenced when k is refused
    for (int k : {0, SIFT_HIP_KNN_MAX + 1}) {
        REQUIRE(sift_hip_match_knn_device(fake, q, 1, q, 1, k, idx, d2, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(std::strstr(sift_hip_last_error(), "k outside"));
        REQUIRE(sift_hip_match_knn_batched(fake, 1, &q, &nq, &q, &nq, k, idx, d2, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_match_knn_host(fake, q, 1, q, 1, k, idx, d2) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_match_knn_list_device(fake, q, 1, q, 1, k, 0.f, rec, &count, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_match_knn_list_host(fake, q, 1, q, 1, k, 0.f, rec, 8, &count) == SIFT_HIP_ERR_INVALID);
        REQUIRE(std::strstr(sift_hip_last_error(), "k outside"));
        count = -7;
    }
    REQUIRE(sift_hip_match_knn_list_device(fake, q, 1, q, 1, 2, NAN, rec, &count, nullptr) == SIFT_HIP_ERR_INVALID);
    REQUIRE(std::strstr(sift_hip_last_error(), "NaN"));
    REQUIRE(sift_hip_match_knn_device(nullptr, q, 1, q, 1, 2, idx, d2, nullptr) == SIFT_HIP_ERR_INVALID);
    REQUIRE(std::strstr(sift_hip_last_error(), "null matcher"));
    REQUIRE(sift_hip_match_knn_list_batched(nullptr, 1, &q, &nq, &q, &nq, 2, 0.f, rec, &count, nullptr) ==
            SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_match_knn_codes_batched(nullptr, reinterpret_cast<const int8_t*>(q), idx, 1, &nq, &nq, &nq, &nq, &nq,
                                             &nq, 2, idx, d2, nullptr) == SIFT_HIP_ERR_INVALID);
    int splits = -1;
    REQUIRE(sift_hip_match_knn_plan(300, 257, 1, 8, &splits) == SIFT_HIP_OK && splits == 2);
    REQUIRE(sift_hip_match_knn_plan(300, 257, 1, 9, &splits) == SIFT_HIP_ERR_INVALID && splits == 2);
    REQUIRE(sift_hip_match_knn_plan(300, 257, 1, 8, nullptr) == SIFT_HIP_ERR_INVALID);
    // nothing was written
    for (int i = 0; i < 8; i++) REQUIRE(idx[i] == 0x5a5a5a5a && rec[i].queryIdx == 0x5a5a5a5a);
    REQUIRE(count == -7);
    std::printf("match knn args ok\n");
    return 0;
}
