// Argument validation of the plane pose calls of sift_cuda::Verifier
// (csrc/verify_cxx.cpp) as a stand-alone CPU program, built by `make asan` with
// -fsanitize=address,undefined beside test_pose_args
// (tests/test_pose_homography_asan.py).  It makes no device call: every refusal is
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
    using sift_cuda::Camera;
    using sift_cuda::PoseParams;
    std::vector<sift_cuda::DMatch> list(16);
    const sift_cuda::DMatch* recs = list.data();
    const float xy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const std::vector<sift_cuda::VerifyPair> two = {{xy, xy, 4, 4, 9}, {xy, xy, 4, 4, 7}};
    std::vector<uint8_t> mask(16, 0);
    const Camera cam{500.f, 510.f, 320.f, 240.f};
    const std::vector<Camera> cams(2, cam);
    const PoseParams params;

    sift_hip_pose_params defaults{0.f, 0.f};
    sift_hip_default_pose_params(&defaults);
    static_assert(sizeof(sift_cuda::PlanePoseResult) == 96 && sizeof(sift_cuda::PlaneCandidate) == 64 &&
                      sizeof(sift_cuda::PoseResult) == 80,
                  "the plane pose record is a pose record and 16 bytes");

    // The C ABI on a null handle.
    sift_hip_homography_result r[2] = {};
    sift_hip_plane_pose_result pr[2] = {};
    const sift_hip_camera ac{500.f, 510.f, 320.f, 240.f};
    const sift_hip_camera acs[2] = {ac, ac};
    REQUIRE(sift_hip_recover_pose_homography_host(nullptr, reinterpret_cast<const sift_hip_dmatch*>(recs), nullptr, 16, xy, 2, 4, xy, 2,
                                       4, r, mask.data(), &ac, &ac, &defaults, pr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr) == SIFT_HIP_ERR_INVALID);
    REQUIRE(sift_hip_recover_pose_homography_batched_device(nullptr, reinterpret_cast<const sift_hip_dmatch*>(recs), nullptr, 2,
                                                 reinterpret_cast<const sift_hip_verify_pair*>(two.data()), 2, 2, r,
                                                 mask.data(), acs, acs, &defaults, pr, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr, nullptr) == SIFT_HIP_ERR_INVALID);

    FakeVerifier fake;
    sift_cuda::Verifier& v = fake.get();
    sift_cuda::HomographyResult res[2] = {};
    sift_cuda::PlanePoseResult pose[2] = {};
    sift_cuda::PlaneCandidate cands[8] = {};
    const std::vector<sift_cuda::HomographyResult> rvec(2);

    // The single-pair forms: every refusal is std::invalid_argument.
    auto single2 = [&](const sift_cuda::DMatch* m, int cap, const float* q, int qs, int nq, const float* t, int ts, int nt,
                       const Camera& cq, const Camera& ct, const PoseParams& p, const std::vector<uint8_t>& k) {
        return thrown([&] { v.recoverPoseHomographyDevice(m, nullptr, cap, q, qs, nq, t, ts, nt, res, k.data(), cq, ct, p, pose); }) == 1 &&
               thrown([&] { (void)v.recoverPoseHomographyHost(m, nullptr, cap, q, qs, nq, t, ts, nt, rvec[0], k, cq, ct, p); }) == 1;
    };
    REQUIRE(single2(recs, -1, xy, 2, 4, xy, 2, 4, cam, cam, params, mask));       // a negative cap
    REQUIRE(single2(recs, 65537, xy, 2, 4, xy, 2, 4, cam, cam, params, mask));    // a cap over 65536
    REQUIRE(single2(nullptr, 16, xy, 2, 4, xy, 2, 4, cam, cam, params, mask));    // null matches
    REQUIRE(single2(recs, 16, nullptr, 2, 4, xy, 2, 4, cam, cam, params, mask));  // null positions
    REQUIRE(single2(recs, 16, xy, 1, 4, xy, 2, 4, cam, cam, params, mask));       // a stride below 2
    REQUIRE(single2(recs, 16, xy, 2, -1, xy, 2, 4, cam, cam, params, mask));      // a negative row count
    for (float bad : {0.f, -2.f, NAN, INFINITY}) {                               // fx, fy: > 0 and finite
        REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, Camera{bad, 500.f, 1.f, 1.f}, cam, params, mask));
        REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, cam, Camera{500.f, bad, 1.f, 1.f}, params, mask));
    }
    for (float bad : {NAN, INFINITY, -INFINITY}) {                               // cx, cy: finite
        REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, Camera{500.f, 500.f, bad, 1.f}, cam, params, mask));
        REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, cam, Camera{500.f, 500.f, 1.f, bad}, params, mask));
    }
    for (float bad : {0.f, -1.f, NAN}) REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, cam, cam, PoseParams{bad, 0.5f}, mask));
    for (float bad : {1.5f, -1.5f, NAN, INFINITY})
        REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, cam, cam, PoseParams{50.f, bad}, mask));
    REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, cam, cam, PoseParams{INFINITY, -1.f}, mask));  // allowed: the limits
    REQUIRE(single2(recs, 16, xy, 2, 4, xy, 2, 4, cam, cam, params, mask));                      // the stand-in's limits
    std::vector<uint8_t> short_mask(15, 0);  // the host form: one mask byte per row
    REQUIRE(thrown([&] { (void)v.recoverPoseHomographyHost(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, rvec[0], short_mask, cam, cam); }) == 1);
    REQUIRE(thrown([&] { v.recoverPoseHomographyDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, res, nullptr, cam, cam, params, pose); }) == 1);
    REQUIRE(thrown([&] { v.recoverPoseHomographyDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, nullptr, mask.data(), cam, cam, params, pose); }) == 1);
    REQUIRE(thrown([&] { v.recoverPoseHomographyDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, res, mask.data(), cam, cam, params, nullptr); }) == 1);
    REQUIRE(thrown([&] {
                v.recoverPoseHomographyDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, res, mask.data(), cam, cam, params, pose, nullptr,
                                    nullptr, list.data() + 15);
            }) == 1);  // out overlaps matches

    // The batched forms.
    auto batch2 = [&](const sift_cuda::DMatch* m, const std::vector<sift_cuda::VerifyPair>& pairs, int qs, int ts,
                      const std::vector<Camera>& cq, const std::vector<Camera>& ct, const PoseParams& p) {
        const std::vector<sift_cuda::HomographyResult> rr(pairs.size());
        return thrown([&] { v.recoverPoseHomographyBatchedDevice(m, nullptr, pairs, qs, ts, res, mask.data(), cq, ct, p, pose); }) == 1 &&
               thrown([&] { (void)v.recoverPoseHomographyBatchedHost(m, nullptr, pairs, qs, ts, rr, mask, cq, ct, p); }) == 1;
    };
    REQUIRE(batch2(recs, {}, 2, 2, {}, {}, params));                                                         // P < 1
    REQUIRE(batch2(recs, std::vector<sift_cuda::VerifyPair>(65, {xy, xy, 4, 4, 0}), 2, 2, std::vector<Camera>(65, cam),
                   std::vector<Camera>(65, cam), params));                                                   // P > 64
    REQUIRE(batch2(recs, {{xy, xy, 4, 4, -1}, two[1]}, 2, 2, cams, cams, params));                           // a negative cap
    REQUIRE(batch2(recs, two, 1, 2, cams, cams, params));                                                    // a stride below 2
    REQUIRE(batch2(nullptr, two, 2, 2, cams, cams, params));                                                 // null matches
    REQUIRE(batch2(recs, two, 2, 2, std::vector<Camera>(1, cam), cams, params));                             // a camera short
    REQUIRE(batch2(recs, two, 2, 2, cams, {cam, Camera{500.f, 0.f, 1.f, 1.f}}, params));                     // fy of pair 1
    REQUIRE(batch2(recs, two, 2, 2, cams, cams, PoseParams{NAN, 0.5f}));                                     // max_depth
    REQUIRE(batch2(recs, two, 2, 2, cams, cams, PoseParams{50.f, 2.f}));                                     // max_cos_parallax
    REQUIRE(batch2(recs, two, 2, 2, cams, cams, params));                                                    // the stand-in's limits
    REQUIRE(thrown([&] { (void)v.recoverPoseHomographyBatchedHost(recs, nullptr, two, 2, 2, rvec, short_mask, cams, cams); }) == 1);
    const std::vector<sift_cuda::HomographyResult> one(1);
    REQUIRE(thrown([&] { (void)v.recoverPoseHomographyBatchedHost(recs, nullptr, two, 2, 2, one, mask, cams, cams); }) == 1);

    for (long long z : fake.zeros) REQUIRE(z == 0);
    for (const sift_cuda::DMatch& m : list) REQUIRE(m.queryIdx == 0 && m.trainIdx == 0 && m.distance == 0.f);
    for (uint8_t b : mask) REQUIRE(b == 0);
    REQUIRE(thrown([&] {
                v.recoverPoseHomographyDevice(recs, nullptr, 16, xy, 2, 4, xy, 2, 4, res, mask.data(), cam, cam,
                                              PoseParams{0.f, 0.5f}, pose, nullptr, nullptr, nullptr, nullptr, cands);
            }) == 1);
    for (const sift_cuda::PlaneCandidate& c : cands) REQUIRE(c.distance == 0.f && c.R[0] == 0.f);
    for (int i = 0; i < 2; i++)
        REQUIRE(pose[i].distance == 0.f && pr[i].distance == 0.f);
    for (int i = 0; i < 2; i++)
        REQUIRE(res[i].hypothesis == 0 && pose[i].candidate == 0 && pose[i].fit == 0 && pr[i].candidate == 0 && r[i].hypothesis == 0);
    std::printf("pose homography args ok\n");
    return 0;
}
