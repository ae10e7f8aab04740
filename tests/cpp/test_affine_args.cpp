// Argument validation of the affine surface -- sift_cuda::verifyAffine's model
// rule (csrc/verify_cxx.cpp) and the C ABI of sift_hip_verify_affine_*,
// sift_hip_score_affine_device and sift_hip_refine_affine_* -- as a stand-alone
// CPU program, built by `make asan` with -fsanitize=address,undefined beside
// test_homography_args (tests/test_affine_asan.py).  It makes no device call:
// every refusal is reached on a null handle or on a block of zeros standing in
// for one, with host memory that is never touched.
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
    static_assert(SIFT_HIP_MODEL_AFFINE == 0 && SIFT_HIP_MODEL_SIMILARITY == 1, "the model constants");
    static_assert(sizeof(sift_hip_affine_result) == 52 && sizeof(sift_cuda::AffineResult) == 52, "the shared record");
    static_assert((int)sift_cuda::AffineModel::Affine == SIFT_HIP_MODEL_AFFINE &&
                      (int)sift_cuda::AffineModel::Similarity == SIFT_HIP_MODEL_SIMILARITY,
                  "the enum is the ABI's constants");
    sift_hip_verify_params abi;
    sift_hip_default_verify_params(&abi);
    std::vector<sift_cuda::DMatch> list(16);
    sift_hip_affine_result r{};
    const sift_hip_dmatch* recs = reinterpret_cast<const sift_hip_dmatch*>(list.data());
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned char mask[16] = {0};

    // A block of zeros standing in for a verifier: limits 0, no verify call has run.
    long long zeros[64] = {0};
    sift_hip_verifier_t fake = reinterpret_cast<sift_hip_verifier_t>(zeros);

    for (int model : {SIFT_HIP_MODEL_AFFINE, SIFT_HIP_MODEL_SIMILARITY}) {
        // A null handle.
        REQUIRE(sift_hip_verify_affine_host(nullptr, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_refine_affine_host(nullptr, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, &r, mask, nullptr,
                                            nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_hypotheses_host(nullptr, model, nullptr, nullptr, nullptr, 1) == SIFT_HIP_ERR_INVALID);

        auto host = [&](int cap, int qs, int ts, float max_error, const sift_hip_dmatch* m, const float* q) {
            sift_hip_verify_params p = abi;
            p.max_error = max_error;
            return sift_hip_verify_affine_host(fake, model, m, nullptr, cap, q, qs, 4, xy, ts, 4, &p, &r, nullptr, nullptr);
        };
        REQUIRE(host(-1, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(65537, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(16, 1, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(16, 2, 0, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(16, 2, 2, 1.5f, nullptr, xy) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(16, 2, 2, 1.5f, recs, nullptr) == SIFT_HIP_ERR_INVALID);
        for (float bad : {0.f, -2.f, NAN, INFINITY}) REQUIRE(host(16, 2, 2, bad, recs, xy) == SIFT_HIP_ERR_INVALID);
        REQUIRE(host(16, 2, 2, 1.5f, recs, xy) == SIFT_HIP_ERR_INVALID);  // the stand-in's limits
        REQUIRE(host(0, 2, 2, 1.5f, nullptr, nullptr) == SIFT_HIP_ERR_INVALID);  // cap == 0 reaches them too
        REQUIRE(sift_hip_verify_affine_device(fake, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi,
                                              reinterpret_cast<sift_hip_affine_result*>(zeros + 32),
                                              const_cast<sift_hip_dmatch*>(recs) + 3, nullptr, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);  // out overlaps matches
        auto refine = [&](int rounds, unsigned char* k, sift_hip_affine_result* res) {
            return sift_hip_refine_affine_host(fake, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, rounds, res, k, nullptr,
                                               nullptr, nullptr);
        };
        REQUIRE(refine(0, mask, &r) == SIFT_HIP_ERR_INVALID);
        REQUIRE(refine(9, mask, &r) == SIFT_HIP_ERR_INVALID);
        REQUIRE(refine(1, nullptr, &r) == SIFT_HIP_ERR_INVALID);
        REQUIRE(refine(1, mask, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(refine(1, mask, &r) == SIFT_HIP_ERR_INVALID);  // the stand-in's limits
        REQUIRE(sift_hip_verify_affine_hypotheses_host(fake, model, nullptr, nullptr, nullptr, -1) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_hypotheses_host(fake, model, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);
    }

    // A model that is neither constant: refused by every call that takes one, single and batched.
    const sift_hip_verify_pair pair{xy, xy, 4, 4, 16};
    for (int model : {-1, 2, 1 << 30}) {
        REQUIRE(sift_hip_verify_affine_host(fake, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_device(fake, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, &abi, &r, nullptr, nullptr,
                                              nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_refine_affine_host(fake, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, &r, mask, nullptr,
                                            nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_refine_affine_device(fake, model, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, &r, mask, nullptr,
                                              nullptr, nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_batched_host(fake, model, recs, nullptr, 1, &pair, 2, 2, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_batched_device(fake, model, recs, nullptr, 1, &pair, 2, 2, &abi, &r, nullptr, nullptr,
                                                      nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_refine_affine_batched_host(fake, model, recs, nullptr, 1, &pair, 2, 2, 1.5f, 1, &r, mask, nullptr,
                                                    nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_refine_affine_batched_device(fake, model, recs, nullptr, 1, &pair, 2, 2, 1.5f, 1, &r, mask, nullptr,
                                                      nullptr, nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_hypotheses_host(fake, model, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_INVALID);
        // the C++ surface refuses it before it creates a verifier
        REQUIRE(thrown([&] {
                    (void)sift_cuda::verifyAffine(list, xy, 4, xy, 4, static_cast<sift_cuda::AffineModel>(model));
                }) == 1);
    }

    // The batched calls' own rules.
    for (int model : {SIFT_HIP_MODEL_AFFINE, SIFT_HIP_MODEL_SIMILARITY}) {
        REQUIRE(sift_hip_verify_affine_batched_host(fake, model, recs, nullptr, 0, &pair, 2, 2, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_batched_host(fake, model, recs, nullptr, 65, &pair, 2, 2, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_batched_host(fake, model, recs, nullptr, 1, nullptr, 2, 2, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);
        REQUIRE(sift_hip_verify_affine_batched_host(fake, model, recs, nullptr, 1, &pair, 2, 2, &abi, &r, nullptr, nullptr) ==
                SIFT_HIP_ERR_INVALID);  // the stand-in's limits
    }

    // The score takes no model: its own refusals.
    int counts[4] = {0, 0, 0, 0};
    REQUIRE(sift_hip_score_affine_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, nullptr, 4, 1.5f, counts, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // null A
    REQUIRE(sift_hip_score_affine_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, xy, 4, 1.5f, nullptr, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // null counts
    REQUIRE(sift_hip_score_affine_device(fake, recs, nullptr, 16, xy, 2, 4, xy, 2, 4, xy, 4, 1.5f, counts, nullptr) ==
            SIFT_HIP_ERR_INVALID);  // the stand-in's limits
    // The other models' getters refuse the stand-in as before.
    REQUIRE(sift_hip_verify_homography_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);
    REQUIRE(sift_hip_verify_hypotheses_host(fake, nullptr, nullptr, nullptr, 4) == SIFT_HIP_ERR_STATE);

    for (long long z : zeros) REQUIRE(z == 0);
    for (unsigned char k : mask) REQUIRE(k == 0);
    for (int c : counts) REQUIRE(c == 0);
    for (float x : r.H) REQUIRE(x == 0.f);
    std::printf("affine args ok\n");
    return 0;
}
