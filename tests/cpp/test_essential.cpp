// sift_cuda::verifyEssential / Verifier::verifyEssential* on the GPU
// (tests/test_gpu_essential_cxx.py): the 300 + 60 list of tests/essential_cases.py,
// dumped by the Python test into the directory given as argv[1]; argv[2] is the
// number of samples.
//   matches.bin   n sift_cuda::DMatch records        q_xy.bin / t_xy.bin   rows x 2 float
//   cams.bin      two sift_cuda::Camera: the query side, the train side
// The program writes what the device form left, for the Python test's checker:
//   verify_result.bin   sift_cuda::VerifyResult      verify_out.bin   n records, prefilled with the byte 0x5A
//   verify_mask.bin     n bytes                      verify_count.bin one int
//   pose.bin            the sift_cuda::PoseResult of recoverPoseDevice on that record and mask, on the same stream
// and itself holds the host, one-shot and batched forms to the device form byte for byte.
// What the ABI refuses throws.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
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

using sift_cuda::Camera;
using sift_cuda::DMatch;
using sift_cuda::TwoViewGeometry;
using sift_cuda::VerifyResult;

template <class T>
static std::vector<T> load(const std::string& path) {
    std::vector<T> out;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        out.resize((size_t)bytes / sizeof(T));
        if (bytes % (long)sizeof(T) || std::fread(out.data(), sizeof(T), out.size(), f) != out.size()) out.clear();
        std::fclose(f);
    }
    return out;
}

static bool store(const std::string& path, const void* data, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

struct Device {
    void* p = nullptr;
    size_t bytes;
    Device(const void* host, size_t n) : bytes(n) {
        if (sift_hip_malloc(&p, bytes ? bytes : 1) != SIFT_HIP_OK) std::abort();
        if (bytes && host && sift_hip_memcpy_h2d(p, host, bytes) != SIFT_HIP_OK) std::abort();
    }
    ~Device() { (void)sift_hip_free(p); }
    template <class T>
    std::vector<T> read() const {
        std::vector<T> out(bytes / sizeof(T));
        if (bytes && sift_hip_memcpy_d2h(out.data(), p, bytes) != SIFT_HIP_OK) std::abort();
        return out;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    const std::string dir = std::string(argv[1]) + "/";
    const int K = std::atoi(argv[2]);
    const std::vector<DMatch> list = load<DMatch>(dir + "matches.bin");
    const std::vector<float> qxy = load<float>(dir + "q_xy.bin"), txy = load<float>(dir + "t_xy.bin");
    const std::vector<Camera> cams = load<Camera>(dir + "cams.bin");
    REQUIRE(!list.empty() && !qxy.empty() && qxy.size() == txy.size() && cams.size() == 2);
    const int n = (int)list.size(), rows = (int)qxy.size() / 2;

    const Device dq(qxy.data(), sizeof(float) * qxy.size()), dt(txy.data(), sizeof(float) * txy.size());
    const float* q = dq.as<const float>();
    const float* t = dt.as<const float>();
    const Device dm(list.data(), sizeof(DMatch) * list.size());
    const DMatch* m = dm.as<const DMatch>();

    sift_cuda::VerifyParams params;
    params.hypotheses = K;
    params.seed = 0;

    sift_cuda::Verifier v(2 * n, 1, -1, 2);
    const std::vector<uint8_t> fill(sizeof(DMatch) * (size_t)n, 0x5A);
    const Device dres(fill.data(), sizeof(VerifyResult)), dmask(fill.data(), (size_t)n);

    // a verifier that has not reserved refuses, and writes nothing
    REQUIRE(throws([&] { v.verifyEssentialDevice(m, nullptr, n, q, 2, rows, t, 2, rows, cams[0], cams[1], params, dres.as<VerifyResult>()); }));
    REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
    REQUIRE(same(dres.read<uint8_t>(), std::vector<uint8_t>(sizeof(VerifyResult), 0x5A)));
    v.reserveEssential(K);
    REQUIRE(throws([&] { v.reserveEssential(K); }));  // once

    // the device form, and the pose from its record and mask with no read in between
    VerifyResult verified{};
    std::vector<uint8_t> verified_mask;
    std::vector<DMatch> verified_list;
    {
        const Device dout(fill.data(), fill.size()), dcnt(fill.data(), sizeof(int)), dpose(fill.data(), sizeof(sift_cuda::PoseResult));
        v.verifyEssentialDevice(m, nullptr, n, q, 2, rows, t, 2, rows, cams[0], cams[1], params, dres.as<VerifyResult>(),
                                dout.as<DMatch>(), dcnt.as<int>(), dmask.as<uint8_t>());
        v.recoverPoseDevice(m, nullptr, n, q, 2, rows, t, 2, rows, dres.as<VerifyResult>(), dmask.as<uint8_t>(), cams[0],
                            cams[1], {}, dpose.as<sift_cuda::PoseResult>());
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        verified = dres.read<VerifyResult>()[0];
        verified_mask = dmask.read<uint8_t>();
        const int count = dcnt.read<int>()[0];
        REQUIRE(count == verified.inliers && count >= 0 && count <= n);
        verified_list = dout.read<DMatch>();
        verified_list.resize((size_t)count);
        REQUIRE(store(dir + "verify_result.bin", &verified, sizeof verified));
        REQUIRE(store(dir + "verify_out.bin", dout.read<uint8_t>().data(), fill.size()));
        REQUIRE(store(dir + "verify_count.bin", &count, sizeof count));
        REQUIRE(store(dir + "verify_mask.bin", verified_mask.data(), (size_t)n));
        REQUIRE(store(dir + "pose.bin", dpose.read<uint8_t>().data(), sizeof(sift_cuda::PoseResult)));
    }

    // the host form and the one shot equal the device form
    {
        const TwoViewGeometry g = v.verifyEssentialHost(m, nullptr, n, q, 2, rows, t, 2, rows, cams[0], cams[1], params);
        REQUIRE(g.hypothesis == verified.hypothesis && std::memcmp(g.F, verified.F, sizeof g.F) == 0);
        REQUIRE(same(g.inliers, verified_list));
        const TwoViewGeometry one = sift_cuda::verifyEssential(list, q, rows, t, rows, cams[0], cams[1], params, 2, 2);
        REQUIRE(one.hypothesis == verified.hypothesis && std::memcmp(one.F, verified.F, sizeof one.F) == 0);
        REQUIRE(same(one.inliers, verified_list));
        // with a refit round: the fundamental refit on the same record and mask
        VerifyResult r = verified;
        std::vector<uint8_t> mask = verified_mask;
        std::vector<DMatch> inliers;
        (void)v.refineHost(m, nullptr, n, q, 2, rows, t, 2, rows, params.max_error, 1, r, mask, &inliers);
        const TwoViewGeometry fit = sift_cuda::verifyEssential(list, q, rows, t, rows, cams[0], cams[1], params, 2, 2, 1);
        REQUIRE(std::memcmp(fit.F, r.F, sizeof r.F) == 0 && same(fit.inliers, inliers));
    }

    // the batched forms: the list twice; pair 0 is the single call, pair 1 the single call with seed + 1
    {
        std::vector<DMatch> twice = list;
        twice.insert(twice.end(), list.begin(), list.end());
        const Device dm2(twice.data(), sizeof(DMatch) * twice.size());
        const std::vector<sift_cuda::VerifyPair> pairs(2, sift_cuda::VerifyPair{q, t, rows, rows, n});
        const std::vector<Camera> cq(2, cams[0]), ct(2, cams[1]);
        const std::vector<TwoViewGeometry> g = v.verifyEssentialBatchedHost(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, cq, ct, params);
        REQUIRE(g.size() == 2 && g[0].hypothesis == verified.hypothesis && std::memcmp(g[0].F, verified.F, sizeof verified.F) == 0);
        REQUIRE(same(g[0].inliers, verified_list));
        sift_cuda::VerifyParams next = params;
        next.seed = 1;
        const TwoViewGeometry one = v.verifyEssentialHost(m, nullptr, n, q, 2, rows, t, 2, rows, cams[0], cams[1], next);
        REQUIRE(g[1].hypothesis == one.hypothesis && std::memcmp(g[1].F, one.F, sizeof one.F) == 0 && same(g[1].inliers, one.inliers));
        const Device dres2(fill.data(), 2 * sizeof(VerifyResult)), dmask2(fill.data(), 2 * (size_t)n);
        v.verifyEssentialBatchedDevice(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, cq, ct, params, dres2.as<VerifyResult>(),
                                       nullptr, nullptr, dmask2.as<uint8_t>());
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        const std::vector<VerifyResult> r2 = dres2.read<VerifyResult>();
        REQUIRE(std::memcmp(&r2[0], &verified, sizeof verified) == 0);
        REQUIRE(std::memcmp(dmask2.read<uint8_t>().data(), verified_mask.data(), (size_t)n) == 0);
        REQUIRE(throws([&] {
            v.verifyEssentialBatchedDevice(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, {cams[0]}, ct, params, dres2.as<VerifyResult>());
        }));
    }

    // too few matches: the empty result, not an error
    {
        const std::vector<DMatch> few(list.begin(), list.begin() + 4);
        const TwoViewGeometry e = sift_cuda::verifyEssential(few, q, rows, t, rows, cams[0], cams[1], params, 2, 2);
        REQUIRE(e.hypothesis == -1 && e.inliers.empty());
        for (float x : e.F) REQUIRE(x == 0.f);
    }

    // what the ABI refuses throws
    for (float bad : {0.f, -1.5f, NAN, INFINITY}) {
        sift_cuda::VerifyParams p = params;
        p.max_error = bad;
        REQUIRE(throws([&] { (void)sift_cuda::verifyEssential(list, q, rows, t, rows, cams[0], cams[1], p, 2, 2); }));
    }
    REQUIRE(throws([&] { (void)sift_cuda::verifyEssential(list, q, rows, t, rows, Camera{0.f, 700.f, 320.f, 240.f}, cams[1], params, 2, 2); }));
    REQUIRE(throws([&] { (void)sift_cuda::verifyEssential(list, q, rows, t, rows, cams[0], cams[1], params, 1, 2); }));
    {
        sift_cuda::VerifyParams p = params;
        p.hypotheses = K + 1;  // above the reservation
        REQUIRE(throws([&] { (void)v.verifyEssentialHost(m, nullptr, n, q, 2, rows, t, 2, rows, cams[0], cams[1], p); }));
    }
    std::printf("essential ok: slot %d, %d inliers of %d\n", verified.hypothesis, verified.inliers, n);
    return 0;
}
