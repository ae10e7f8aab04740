// Argument validation of the batched calls of sift_cuda::Verifier
// (csrc/verify_cxx.cpp) as a stand-alone CPU program, built by `make asan` with
// -fsanitize=address,undefined beside test_verify_args
// (tests/test_verify_batched_asan.py).  It makes no device call: limits outside
// the ABI's are std::invalid_argument before any, and every per-call refusal is
// reached on a null handle or on a block of zeros standing in for one.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
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
    for (int m : {0, -1, 64 * 65536 + 1}) REQUIRE(thrown([&] { sift_cuda::Verifier v(m, 64, 0, 4); }) == 1);
    for (int k : {0, -7, 4097}) REQUIRE(thrown([&] { sift_cuda::Verifier v(100, k, 0, 4); }) == 1);
    for (int p : {0, -1, 65}) REQUIRE(thrown([&] { sift_cuda::Verifier v(100, 64, 0, p); }) == 1);

    std::vector<sift_cuda::DMatch> list(16);
    const sift_cuda::DMatch* recs = list.data();
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const sift_cuda::VerifyParams good;
    const std::vector<sift_cuda::VerifyPair> two = {{xy, xy, 4, 4, 9}, {xy, xy, 4, 4, 7}};

    // The C ABI on a null handle and host memory that is never touched.
    sift_hip_verify_params abi;
    sift_hip_default_verify_params(&abi);
    sift_hip_verify_result r[2] = {};
    REQUIRE(sift_hip_verify_fundamental_batched_host(nullptr, reinterpret_cast<const sift_hip_dmatch*>(recs), nullptr, 2,
                                                     reinterpret_cast<const sift_hip_verify_pair*>(two.data()), 2, 2, &abi,
                                                     r, nullptr, nullptr) == SIFT_HIP_ERR_INVALID);

    // Every refusal through the C++ methods, on the stand-in: std::invalid_argument, nothing read or written.
    FakeVerifier fake;
    sift_cuda::Verifier& v = fake.get();
    sift_cuda::VerifyResult fres[2] = {};
    sift_cuda::HomographyResult hres[2] = {};
    auto all4 = [&](const sift_cuda::DMatch* m, const std::vector<sift_cuda::VerifyPair>& pairs, int qs, int ts,
                    const sift_cuda::VerifyParams& p) {
        return thrown([&] { v.verifyBatchedDevice(m, nullptr, pairs, qs, ts, p, fres); }) == 1 &&
               thrown([&] { v.verifyHomographyBatchedDevice(m, nullptr, pairs, qs, ts, p, hres); }) == 1 &&
               thrown([&] { (void)v.verifyBatchedHost(m, nullptr, pairs, qs, ts, p); }) == 1 &&
               thrown([&] { (void)v.verifyHomographyBatchedHost(m, nullptr, pairs, qs, ts, p); }) == 1;
    };
    REQUIRE(all4(recs, {}, 2, 2, good));                                                    // P < 1
    REQUIRE(all4(recs, std::vector<sift_cuda::VerifyPair>(65, two[0]), 2, 2, good));          // P > 64
    REQUIRE(all4(recs, {{xy, xy, 4, 4, -1}, two[1]}, 2, 2, good));                           // a negative cap
    REQUIRE(all4(recs, {two[0], {xy, xy, 4, 4, 65537}}, 2, 2, good));                        // a cap over 65536
    REQUIRE(all4(recs, {{xy, xy, 4, 4, 65536}, {xy, xy, 4, 4, 70000}}, 2, 2, good));         // the SPILL caps
    REQUIRE(all4(recs, {{xy, xy, -1, 4, 9}, two[1]}, 2, 2, good));                           // a negative nq
    REQUIRE(all4(recs, {two[0], {xy, xy, 4, -2, 7}}, 2, 2, good));                           // a negative nt
    REQUIRE(all4(recs, two, 1, 2, good) && all4(recs, two, 2, 0, good));                     // a stride below 2
    REQUIRE(all4(recs, {{nullptr, xy, 4, 4, 9}, two[1]}, 2, 2, good));                       // null positions, cap > 0
    REQUIRE(all4(recs, {two[0], {xy, nullptr, 4, 4, 7}}, 2, 2, good));
    REQUIRE(all4(nullptr, two, 2, 2, good));                                                 // null matches, rows > 0
    for (float bad : {0.f, -2.f, NAN, INFINITY}) {
        sift_cuda::VerifyParams p = good;
        p.max_error = bad;
        REQUIRE(all4(recs, two, 2, 2, p));
    }
    for (int k : {0, -1, 4097}) {
        sift_cuda::VerifyParams p = good;
        p.hypotheses = k;
        REQUIRE(all4(recs, two, 2, 2, p));
    }
    REQUIRE(all4(recs, two, 2, 2, good));                                 // the stand-in's limits
    REQUIRE(all4(nullptr, {{nullptr, nullptr, 0, 0, 0}}, 2, 2, good));    // an empty pair is no error: the limits again
    REQUIRE(thrown([&] { v.verifyBatchedDevice(recs, nullptr, two, 2, 2, good, fres, list.data() + 15); }) == 1);  // out
    REQUIRE(thrown([&] { v.verifyBatchedDevice(recs, nullptr, two, 2, 2, good, nullptr); }) == 1);  // null results
    for (long long z : fake.zeros) REQUIRE(z == 0);
    for (const sift_cuda::DMatch& m : list) REQUIRE(m.queryIdx == 0 && m.trainIdx == 0 && m.distance == 0.f);
    for (int i = 0; i < 2; i++) REQUIRE(fres[i].hypothesis == 0 && hres[i].hypothesis == 0 && r[i].hypothesis == 0);
    std::printf("verify batched args ok\n");
    return 0;
}
