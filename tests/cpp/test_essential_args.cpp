// Argument validation of the essential surface -- sift_cuda::Verifier's camera
// rule for batches (csrc/verify_cxx.cpp) and the C ABI of
// sift_hip_verifier_reserve_essential and sift_hip_verify_essential_* -- as a
// stand-alone CPU program, built by `make asan` with
// -fsanitize=address,undefined beside test_affine_args
// (tests/test_essential_asan.py).  It makes no device call: every refusal is
// reached on a null handle or on a block standing in for one, with host memory
// that is never touched.
#include <cmath>
#include <cstdio>
#include <cstring>
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
    static_assert(sizeof(sift_hip_verify_result) == 52 && sizeof(sift_cuda::VerifyResult) == 52, "the record");
    static_assert(SIFT_HIP_ABI_VERSION == 1, "the ABI version stays");
    sift_hip_verify_params abi;
    sift_hip_default_verify_params(&abi);
    abi.hypotheses = 16;
    std::vector<sift_cuda::DMatch> list(16);
    sift_hip_verify_result r{};
    const sift_hip_dmatch* recs = reinterpret_cast<const sift_hip_dmatch*>(list.data());
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const sift_hip_camera good{700.f, 710.f, 320.f, 240.f};

    // A block standing in for a verifier: the four leading ints are device, max_matches, max_hypotheses, max_pairs;
    // everything behind them is zero -- no essential scratch, no verify call has run.
    long long block[64] = {0};
    const int head[4] = {0, 64, 0, 2};
    std::memcpy(block, head, sizeof head);
    sift_hip_verifier_t fake = reinterpret_cast<sift_hip_verifier_t>(block);

    // A null handle.
    REQUIRE(sift_hip_verifier_reserve_essential(nullptr, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_verify_essential_host(nullptr, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &good, &good, &abi, &r, nullptr,
                                           nullptr) == SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_verify_essential_hypotheses_host(nullptr, nullptr, nullptr, nullptr, 1) == SIFT_HIP_ERR_INVALID);
    // The reservation's range.
    for (int n : {0, -1, 4097}) REQUIRE(sift_hip_verifier_reserve_essential(fake, n) == SIFT_HIP_ERR_INVALID);

    auto host = [&](int cap, int qs, int ts, float max_error, const sift_hip_dmatch* m, const float* q,
                    const sift_hip_camera* cq, const sift_hip_camera* ct, int K) {
        sift_hip_verify_params p = abi;
        p.max_error = max_error, p.hypotheses = K;
        return sift_hip_verify_essential_host(fake, m, nullptr, cap, q, qs, 4, xy, ts, 4, cq, ct, &p, &r, nullptr, nullptr);
    };
    REQUIRE(host(-1, 2, 2, 1.5f, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(65537, 2, 2, 1.5f, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 1, 2, 1.5f, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 0, 1.5f, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, nullptr, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, recs, nullptr, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    for (float bad : {0.f, -2.f, NAN, INFINITY})
        REQUIRE(host(16, 2, 2, bad, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);
    for (int K : {0, -1, 4097}) REQUIRE(host(16, 2, 2, 1.5f, recs, xy, &good, &good, K) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(65, 2, 2, 1.5f, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_INVALID);  // the stand-in's max_matches
    // The cameras: the pose calls' rules.
    REQUIRE(host(16, 2, 2, 1.5f, recs, xy, nullptr, &good, 16) == SIFT_HIP_ERR_INVALID);
    REQUIRE(host(16, 2, 2, 1.5f, recs, xy, &good, nullptr, 16) == SIFT_HIP_ERR_INVALID);
    for (const sift_hip_camera bad : {sift_hip_camera{0.f, 700.f, 320.f, 240.f}, sift_hip_camera{700.f, -1.f, 320.f, 240.f},
                                      sift_hip_camera{NAN, 700.f, 320.f, 240.f}, sift_hip_camera{700.f, INFINITY, 320.f, 240.f},
                                      sift_hip_camera{700.f, 700.f, NAN, 240.f}, sift_hip_camera{700.f, 700.f, 320.f, INFINITY}}) {
        REQUIRE(host(16, 2, 2, 1.5f, recs, xy, &bad, &good, 16) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(16, 2, 2, 1.5f, recs, xy, &good, &bad, 16) == SIFT_HIP_ERR_INVALID);
    }
    // Every argument in order: the verifier has not reserved.  The sample count is not bound by max_hypotheses (0).
    REQUIRE(host(16, 2, 2, 1.5f, recs, xy, &good, &good, 16) == SIFT_HIP_ERR_STATE);
    REQUIRE(host(16, 2, 2, 1.5f, recs, xy, &good, &good, 4096) == SIFT_HIP_ERR_STATE);
    REQUIRE(host(0, 2, 2, 1.5f, nullptr, nullptr, &good, &good, 16) == SIFT_HIP_ERR_STATE);  // cap == 0 reaches it too
    REQUIRE(sift_hip_verify_essential_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &good, &good, &abi, &r,
                                             const_cast<sift_hip_dmatch*>(recs) + 3, nullptr, nullptr, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // out overlaps matches
    REQUIRE(sift_hip_verify_essential_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &good, &good, &abi, &r, nullptr,
                                             nullptr, nullptr, nullptr) == SIFT_HIP_ERR_STATE);

    // The batched calls' own rules.
    const sift_hip_verify_pair pair{xy, xy, 4, 4, 16};
    const sift_hip_camera cams[2] = {good, good};
    auto batched = [&](int P, const sift_hip_verify_pair* pairs, const sift_hip_camera* cq) {
        return sift_hip_verify_essential_batched_host(fake, recs, nullptr, P, pairs, 2, 2, cq, cams, &abi, &r, nullptr, nullptr);
    };
    REQUIRE(batched(0, &pair, cams) == SIFT_HIP_ERR_INVALID);
    REQUIRE(batched(65, &pair, cams) == SIFT_HIP_ERR_INVALID);
    REQUIRE(batched(1, nullptr, cams) == SIFT_HIP_ERR_INVALID);
    REQUIRE(batched(1, &pair, nullptr) == SIFT_HIP_ERR_INVALID);
    REQUIRE(batched(1, &pair, cams) == SIFT_HIP_ERR_STATE);
    REQUIRE(sift_hip_verify_essential_batched_device(fake, recs, nullptr, 1, &pair, 2, 2, cams, cams, &abi, &r, nullptr,
                                                     nullptr, nullptr, nullptr) == SIFT_HIP_ERR_STATE);

    // The getters: none answers on a verifier without a verify call.
    REQUIRE(sift_hip_verify_essential_hypotheses_host(fake, nullptr, nullptr, nullptr, -1) == SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_verify_essential_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);
    REQUIRE(sift_hip_verify_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);
    REQUIRE(sift_hip_verify_homography_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);

    // The C++ surface: one camera per pair and side, judged before the handle is used (a Verifier cannot be made
    // without a device, so the methods are reached through a block of its size; the rule throws first).
    {
        alignas(sift_cuda::Verifier) unsigned char store[sizeof(sift_cuda::Verifier)] = {0};
        sift_cuda::Verifier& v = *reinterpret_cast<sift_cuda::Verifier*>(store);  // m_handle == nullptr
        const std::vector<sift_cuda::VerifyPair> pairs(2);
        const std::vector<sift_cuda::Camera> one(1), two(2);
        sift_cuda::VerifyResult res[2] = {};
        REQUIRE(thrown([&] { v.verifyEssentialBatchedDevice(list.data(), nullptr, pairs, 2, 2, one, two, {}, res); }) == 1);
        REQUIRE(thrown([&] { v.verifyEssentialBatchedDevice(list.data(), nullptr, pairs, 2, 2, two, one, {}, res); }) == 1);
        REQUIRE(thrown([&] { (void)v.verifyEssentialBatchedHost(list.data(), nullptr, pairs, 2, 2, one, two); }) == 1);
        REQUIRE(thrown([&] { v.reserveEssential(16); }) == 1);  // the null handle: the ABI's refusal, thrown
    }

    for (size_t i = 2; i < 64; i++) REQUIRE(block[i] == 0);
    REQUIRE(std::memcmp(block, head, sizeof head) == 0);
    for (float x : r.F) REQUIRE(x == 0.f);
    REQUIRE(r.inliers == 0 && r.hypothesis == 0);
    std::printf("essential args ok\n");
    return 0;
}
