// Argument validation of the refit calls of sift_cuda::Verifier
// (csrc/verify_cxx.cpp) as a stand-alone CPU program, built by `make asan` with
// -fsanitize=address,undefined beside test_verify_batched_args
// (tests/test_refit_asan.py).  It makes no device call: every refusal is
// reached on a null handle or on a block of zeros standing in for one, and on
// host memory that is never read or written.
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

// A sift_cuda::Verifier whose handle is a block of zeros (limits 0), built in place so that no constructor reaches
// the device and no destructor runs: the class holds the handle alone.
struct FakeVerifier {
    long long zeros[32] = {0};
    alignas(sift_cuda::Verifier) unsigned char object[sizeof(sift_cuda::Verifier)];
    sift_cuda::Verifier& get() {
        static_assert(sizeof(sift_cuda::Verifier) == sizeof(void*), "Verifier holds its handle alone");
        void* handle = zeros;
        std::memcpy(object, &handle, sizeof handle);
        return *reinterpret_cast<sift_cuda::Verifier*>(object);
    }
};

int main() {
    std::vector<sift_cuda::DMatch> list(16);
    const sift_cuda::DMatch* recs = list.data();
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const std::vector<sift_cuda::VerifyPair> two = {{xy, xy, 4, 4, 9}, {xy, xy, 4, 4, 7}};
    std::vector<uint8_t> mask(16, 0);

    // The C ABI on a null handle.
    sift_hip_verify_result r[2] = {};
    REQUIRE(sift_hip_refine_fundamental_host(nullptr, reinterpret_cast<const sift_hip_dmatch*>(recs), nullptr, 16, xy, 2, 4,
                                             xy, 2, 4, 1.5f, 1, r, mask.data(), nullptr, nullptr,
                                             nullptr) == SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_refine_homography_batched_device(nullptr, reinterpret_cast<const sift_hip_dmatch*>(recs), nullptr, 2,
                                                      reinterpret_cast<const sift_hip_verify_pair*>(two.data()), 2, 2, 1.5f,
                                                      1, reinterpret_cast<sift_hip_homography_result*>(r), mask.data(),
                                                      nullptr, nullptr, nullptr, nullptr) == SIFT_HIP_ERR_INVALID);

    FakeVerifier fake;
    sift_cuda::Verifier& v = fake.get();
    sift_cuda::VerifyResult fres[2] = {};
    sift_cuda::HomographyResult hres[2] = {};
    std::vector<sift_cuda::VerifyResult> fvec(2);
    std::vector<sift_cuda::HomographyResult> hvec(2);

    // The single-pair forms: every refusal is std::invalid_argument.
    auto single4 = [&](const sift_cuda::DMatch* m, int cap, const float* q, int qs, int nq, const float* t, int ts, int nt,
                       float e, int rounds, std::vector<uint8_t>& k) {
        return thrown([&] { v.refineDevice(m, nullptr, cap, q, qs, nq, t, ts, nt, e, rounds, fres, k.data()); }) == 1 &&
               thrown([&] { v.refineHomographyDevice(m, nullptr, cap, q, qs, nq, t, ts, nt, e, rounds, hres, k.data()); }) == 1 &&
               thrown([&] { (void)v.refineHost(m, nullptr, cap, q, qs, nq, t, ts, nt, e, rounds, fvec[0], k); }) == 1 &&
               thrown([&] { (void)v.refineHomographyHost(m, nullptr, cap, q, qs, nq, t, ts, nt, e, rounds, hvec[0], k); }) == 1;
    };
    REQUIRE(single4(recs, 16, xy, 2, 4, xy, 2, 4, 1.5f, 0, mask));       // rounds outside 1..8
    REQUIRE(single4(recs, 16, xy, 2, 4, xy, 2, 4, 1.5f, 9, mask));
    REQUIRE(single4(recs, -1, xy, 2, 4, xy, 2, 4, 1.5f, 1, mask));       // a negative cap
    REQUIRE(single4(recs, 65537, xy, 2, 4, xy, 2, 4, 1.5f, 1, mask));    // a cap over 65536
    REQUIRE(single4(nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, mask));    // null matches
    REQUIRE(single4(recs, 16, nullptr, 2, 4, xy, 2, 4, 1.5f, 1, mask));  // null positions
    REQUIRE(single4(recs, 16, xy, 1, 4, xy, 2, 4, 1.5f, 1, mask));       // a stride below 2
    REQUIRE(single4(recs, 16, xy, 2, -1, xy, 2, 4, 1.5f, 1, mask));      // a negative row count
    for (float bad : {0.f, -2.f, NAN, INFINITY}) REQUIRE(single4(recs, 16, xy, 2, 4, xy, 2, 4, bad, 1, mask));
    REQUIRE(single4(recs, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, mask));       // the stand-in's limits
    std::vector<uint8_t> short_mask(15, 0);                              // the host forms: one mask byte per row
    REQUIRE(thrown([&] { (void)v.refineHost(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, fvec[0], short_mask); }) == 1);
    REQUIRE(thrown([&] { v.refineDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, fres, nullptr); }) == 1);  // null mask
    REQUIRE(thrown([&] { v.refineDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, nullptr, mask.data()); }) == 1);
    REQUIRE(thrown([&] { v.refineDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, 1.5f, 1, fres, mask.data(),
                                        list.data() + 15); }) == 1);  // out overlaps matches

    // The batched forms.
    auto batch4 = [&](const sift_cuda::DMatch* m, const std::vector<sift_cuda::VerifyPair>& pairs, int qs, int ts, float e,
                      int rounds) {
        std::vector<sift_cuda::VerifyResult> fr(pairs.size());
        std::vector<sift_cuda::HomographyResult> hr(pairs.size());
        return thrown([&] { v.refineBatchedDevice(m, nullptr, pairs, qs, ts, e, rounds, fres, mask.data()); }) == 1 &&
               thrown([&] { v.refineHomographyBatchedDevice(m, nullptr, pairs, qs, ts, e, rounds, hres, mask.data()); }) == 1 &&
               thrown([&] { (void)v.refineBatchedHost(m, nullptr, pairs, qs, ts, e, rounds, fr, mask); }) == 1 &&
               thrown([&] { (void)v.refineHomographyBatchedHost(m, nullptr, pairs, qs, ts, e, rounds, hr, mask); }) == 1;
    };
    REQUIRE(batch4(recs, {}, 2, 2, 1.5f, 1));                                                   // P < 1
    REQUIRE(batch4(recs, std::vector<sift_cuda::VerifyPair>(65, {xy, xy, 4, 4, 0}), 2, 2, 1.5f, 1));  // P > 64
    REQUIRE(batch4(recs, {{xy, xy, 4, 4, -1}, two[1]}, 2, 2, 1.5f, 1));                          // a negative cap
    REQUIRE(batch4(recs, {two[0], {xy, xy, 4, 4, 65537}}, 2, 2, 1.5f, 1));                       // a cap over 65536
    REQUIRE(batch4(recs, two, 1, 2, 1.5f, 1));                                                  // a stride below 2
    REQUIRE(batch4(nullptr, two, 2, 2, 1.5f, 1));                                               // null matches
    REQUIRE(batch4(recs, two, 2, 2, NAN, 1));                                                   // max_error
    REQUIRE(batch4(recs, two, 2, 2, 1.5f, 0) && batch4(recs, two, 2, 2, 1.5f, 9));              // rounds
    REQUIRE(batch4(recs, two, 2, 2, 1.5f, 1));                                                  // the stand-in's limits
    REQUIRE(thrown([&] { (void)v.refineBatchedHost(recs, nullptr, two, 2, 2, 1.5f, 1, fvec, short_mask); }) == 1);
    std::vector<sift_cuda::VerifyResult> one(1);
    REQUIRE(thrown([&] { (void)v.refineBatchedHost(recs, nullptr, two, 2, 2, 1.5f, 1, one, mask); }) == 1);

    for (long long z : fake.zeros) REQUIRE(z == 0);
    for (const sift_cuda::DMatch& m : list) REQUIRE(m.queryIdx == 0 && m.trainIdx == 0 && m.distance == 0.f);
    for (uint8_t b : mask) REQUIRE(b == 0);
    for (int i = 0; i < 2; i++)
        REQUIRE(fres[i].hypothesis == 0 && hres[i].hypothesis == 0 && r[i].hypothesis == 0 && fvec[i].hypothesis == 0);
    std::printf("refit args ok\n");
    return 0;
}
