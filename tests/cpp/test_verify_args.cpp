// Argument validation of sift_cuda::Verifier / verifyFundamental
// (csrc/verify_cxx.cpp) as a stand-alone CPU program, built by `make asan` with
// -fsanitize=address,undefined beside test_multi (tests/test_verify_asan.py).
// It makes no device call: limits outside the ABI's are std::invalid_argument
// before any, and every per-call refusal is reached on a null handle or on a
// block of zeros standing in for one.
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
    for (int m : {0, -1, 65537}) REQUIRE(thrown([&] { sift_cuda::Verifier v(m, 64); }) == 1);
    for (int k : {0, -7, 4097}) REQUIRE(thrown([&] { sift_cuda::Verifier v(100, k); }) == 1);

    sift_cuda::VerifyParams d;
    sift_hip_verify_params abi;
    sift_hip_default_verify_params(&abi);
    REQUIRE(d.hypotheses == abi.hypotheses && d.seed == abi.seed && d.max_error == abi.max_error);

    // The C ABI on a null handle and host memory that is never touched.
    std::vector<sift_cuda::DMatch> list(16);
    sift_hip_verify_result r{};
    const sift_hip_dmatch* recs = reinterpret_cast<const sift_hip_dmatch*>(list.data());
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    REQUIRE(sift_hip_verify_fundamental_host(nullptr, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi, &r, nullptr, nullptr) ==
            SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_verify_hypotheses_host(nullptr, nullptr, nullptr, nullptr, 1) == SIFT_HIP_ERR_INVALID);

    // Every refusal that is judged before the handle is looked at, on a block of zeros standing in for a verifier
    // (limits 0, so a call that got past them would still be refused at the limits, before any device call).
    long long zeros[32] = {0};
    sift_hip_verifier_t fake = reinterpret_cast<sift_hip_verifier_t>(zeros);
    auto host = [&](int cap, int qs, int ts, float max_error, const sift_hip_dmatch* m, const float* q) {
        sift_hip_verify_params p = abi;
        p.max_error = max_error;
        return sift_hip_verify_fundamental_host(fake, m, nullptr, cap, q, qs, 4, xy, ts, 4, &p, &r, nullptr, nullptr);
    };
    REQUIRE(host(-1, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(65537, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 1, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 0, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, nullptr, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, recs, nullptr) == SIFT_HIP_ERR_INVALID);
    for (float bad : {0.f, -2.f, NAN, INFINITY}) REQUIRE(host(16, 2, 2, bad, recs, xy) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);  // the stand-in's limits
    REQUIRE(sift_hip_verify_fundamental_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi,
                                               reinterpret_cast<sift_hip_verify_result*>(zeros + 16),
                                               const_cast<sift_hip_dmatch*>(recs) + 3, nullptr, nullptr, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // out overlaps matches
    for (long long z : zeros) REQUIRE(z == 0);
    std::printf("verify args ok\n");
    return 0;
}
