// Argument validation of the homography surface -- sift_cuda::Verifier::verifyHomography*,
// verifyHomography, projectHomographyDevice (csrc/verify_cxx.cpp) and the C ABI
// under them -- as a stand-alone CPU program, built by `make asan` with
// -fsanitize=address,undefined beside test_verify_args
// (tests/test_homography_asan.py).  It makes no device call: every refusal is
// reached on a null handle, on a block of zeros standing in for one, or, for
// the handle-free projection, on host memory that is never touched.
#include <climits>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "sift_cuda/Verify.hh"
#include "sift_hip.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// 0: no exception, 1: std::invalid_argument, 2: another std::exception.
template <class Fn>
static int thrown(Fn fn) {
    try {
        fn();
    } catch (const std::invalid_argument&) {
        return 1;
    } catch (const std::exception&) {
        return 2;
    }
    return 0;
}

int main() {
    sift_hip_verify_params abi;
    sift_hip_default_verify_params(&abi);
    std::vector<sift_cuda::DMatch> list(16);
    sift_hip_homography_result r{};
    const sift_hip_dmatch* recs = reinterpret_cast<const sift_hip_dmatch*>(list.data());
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // A null handle.
    REQUIRE(sift_hip_verify_homography_host(nullptr, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi, &r, nullptr, nullptr) ==
            SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_verify_homography_hypotheses_host(nullptr, nullptr, nullptr, nullptr, 1) == SIFT_HIP_ERR_INVALID);

    // A block of zeros standing in for a verifier: limits 0, no verify call has run.
    long long zeros[64] = {0};
    sift_hip_verifier_t fake = reinterpret_cast<sift_hip_verifier_t>(zeros);
    auto host = [&](int cap, int qs, int ts, float max_error, const sift_hip_dmatch* m, const float* q) {
        sift_hip_verify_params p = abi;
        p.max_error = max_error;
        return sift_hip_verify_homography_host(fake, m, nullptr, cap, q, qs, 4, xy, ts, 4, &p, &r, nullptr, nullptr);
    };
    REQUIRE(host(-1, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(65537, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 1, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 0, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, nullptr, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, recs, nullptr) == SIFT_HIP_ERR_INVALID);
    for (float bad : {0.f, -2.f, NAN, INFINITY}) REQUIRE(host(16, 2, 2, bad, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);  // the stand-in's limits
    REQUIRE(sift_hip_verify_homography_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi,
                                              reinterpret_cast<sift_hip_homography_result*>(zeros + 32),
                                              const_cast<sift_hip_dmatch*>(recs) + 3, nullptr, nullptr, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // out overlaps matches
    int counts[4] = {0, 0, 0, 0};
    REQUIRE(sift_hip_score_homography_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, nullptr, 4, 1.5f, counts, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // null H
    REQUIRE(sift_hip_verify_homography_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);
    REQUIRE(sift_hip_verify_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);

    // The projection: refused before anything is launched, whatever the extents.
    float rows[64] = {0};
    const float H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(nullptr, rows, 2, 4, rows + 32); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 1, 4, rows + 32); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 2, 4, rows + 32, 1); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 2, -1, rows + 32); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, nullptr, 2, 4, rows + 32); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 2, 4, nullptr); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 2, 4, rows + 2); }) == 1);      // shifted rows
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 3, 4, rows, 2); }) == 1);       // same start, other strides
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows + 8, 2, 4, rows, 4); }) == 1);   // xy inside out_xy
    // extents as large as the address space still overlap: no wrap-around in the check
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, INT_MAX, INT_MAX, rows + 32, INT_MAX); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows + 32, 2, 4, rows, INT_MAX); }) == 1);
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, rows, 2, 0, rows); }) == 0);          // nothing to do
    REQUIRE(thrown([&] { sift_cuda::projectHomographyDevice(H, nullptr, 2, 0, nullptr); }) == 0);

    for (long long z : zeros) REQUIRE(z == 0);
    for (float v : rows) REQUIRE(v == 0.f);
    for (int c : counts) REQUIRE(c == 0);
    std::printf("homography args ok\n");
    return 0;
}
