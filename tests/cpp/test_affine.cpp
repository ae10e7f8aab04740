// sift_cuda::verifyAffine / Verifier::verifyAffine* / refineAffine* on the GPU
// (tests/test_gpu_affine_cxx.py): the main case of tests/affine_cases.py, dumped
// by the Python test into the directory given as argv[1]; argv[2] is the model
// (0: affine map, 1: similarity), argv[3] the hypotheses, argv[4] the refit rounds.
//   matches.bin   n sift_cuda::DMatch records        q_xy.bin / t_xy.bin   rows x 2 float
// The program writes what the device forms left, for the Python test's checker:
//   verify_result.bin / refine_result.bin   sift_cuda::AffineResult
//   verify_out.bin / refine_out.bin         n records, prefilled with the byte 0x5A
//   verify_mask.bin / refine_mask.bin       n bytes       verify_count.bin / refine_count.bin   one int
//   refine_accepted.bin                     one int
//   oneshot.bin       sift_cuda::AffineResult of verifyAffine(..., refit): H and hypothesis, inliers = the list's size
//   oneshot_list.bin  its inlier records
// and itself holds the host and batched forms to the device forms byte for byte.
// What the ABI refuses throws std::invalid_argument.
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

using sift_cuda::AffineModel;
using sift_cuda::AffineResult;
using sift_cuda::DMatch;

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
static bool throws_invalid(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 5);
    const std::string dir = std::string(argv[1]) + "/";
    const AffineModel model = std::atoi(argv[2]) ? AffineModel::Similarity : AffineModel::Affine;
    const int K = std::atoi(argv[3]), rounds = std::atoi(argv[4]);
    const std::vector<DMatch> list = load<DMatch>(dir + "matches.bin");
    const std::vector<float> qxy = load<float>(dir + "q_xy.bin"), txy = load<float>(dir + "t_xy.bin");
    REQUIRE(!list.empty() && !qxy.empty() && qxy.size() == txy.size());
    const int n = (int)list.size(), rows = (int)qxy.size() / 2;

    const Device dq(qxy.data(), sizeof(float) * qxy.size()), dt(txy.data(), sizeof(float) * txy.size());
    const float* q = dq.as<const float>();
    const float* t = dt.as<const float>();
    const Device dm(list.data(), sizeof(DMatch) * list.size());
    const DMatch* m = dm.as<const DMatch>();

    sift_cuda::VerifyParams params;
    params.hypotheses = K;
    params.seed = 0;

    sift_cuda::Verifier v(2 * n, K, -1, 2);
    const std::vector<uint8_t> fill(sizeof(DMatch) * (size_t)n, 0x5A);

    // the device forms: verify, then refine in place on its record and mask
    const Device dres(fill.data(), sizeof(AffineResult)), dmask(fill.data(), (size_t)n);
    std::vector<uint8_t> verified_mask;
    AffineResult verified{};
    {
        const Device dout(fill.data(), fill.size()), dcnt(fill.data(), sizeof(int));
        v.verifyAffineDevice(m, nullptr, n, q, 2, rows, t, 2, rows, model, params, dres.as<AffineResult>(), dout.as<DMatch>(),
                             dcnt.as<int>(), dmask.as<uint8_t>());
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        verified = dres.read<AffineResult>()[0];
        verified_mask = dmask.read<uint8_t>();
        REQUIRE(store(dir + "verify_result.bin", &verified, sizeof verified));
        REQUIRE(store(dir + "verify_out.bin", dout.read<uint8_t>().data(), fill.size()));
        REQUIRE(store(dir + "verify_count.bin", dcnt.read<int>().data(), sizeof(int)));
        REQUIRE(store(dir + "verify_mask.bin", verified_mask.data(), (size_t)n));
    }
    AffineResult refined{};
    std::vector<uint8_t> refined_mask;
    std::vector<DMatch> refined_list;
    int accepted = -1;
    {
        const Device dout(fill.data(), fill.size()), dcnt(fill.data(), sizeof(int)), dacc(fill.data(), sizeof(int));
        v.refineAffineDevice(m, nullptr, n, q, 2, rows, t, 2, rows, model, params.max_error, rounds, dres.as<AffineResult>(),
                             dmask.as<uint8_t>(), dout.as<DMatch>(), dcnt.as<int>(), dacc.as<int>());
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        refined = dres.read<AffineResult>()[0];
        refined_mask = dmask.read<uint8_t>();
        accepted = dacc.read<int>()[0];
        const int count = dcnt.read<int>()[0];
        REQUIRE(count >= 0 && count <= n);
        refined_list = dout.read<DMatch>();
        refined_list.resize((size_t)count);
        REQUIRE(store(dir + "refine_result.bin", &refined, sizeof refined));
        REQUIRE(store(dir + "refine_out.bin", dout.read<uint8_t>().data(), fill.size()));
        REQUIRE(store(dir + "refine_count.bin", &count, sizeof count));
        REQUIRE(store(dir + "refine_mask.bin", refined_mask.data(), (size_t)n));
        REQUIRE(store(dir + "refine_accepted.bin", &accepted, sizeof accepted));
    }

    // the host forms equal the device forms
    {
        const sift_cuda::PlanarGeometry g = v.verifyAffineHost(m, nullptr, n, q, 2, rows, t, 2, rows, model, params);
        REQUIRE(g.hypothesis == verified.hypothesis && std::memcmp(g.H, verified.H, sizeof g.H) == 0);
        REQUIRE((int)g.inliers.size() == verified.inliers);
        AffineResult r = verified;
        std::vector<uint8_t> mask = verified_mask;
        std::vector<DMatch> inliers;
        REQUIRE(v.refineAffineHost(m, nullptr, n, q, 2, rows, t, 2, rows, model, params.max_error, rounds, r, mask,
                                   &inliers) == accepted);
        REQUIRE(std::memcmp(&r, &refined, sizeof r) == 0 && same(mask, refined_mask) && same(inliers, refined_list));
    }

    // the one shot with refit rounds
    {
        const sift_cuda::PlanarGeometry g = sift_cuda::verifyAffine(list, q, rows, t, rows, model, params, 2, 2, rounds);
        AffineResult r = refined;
        std::memcpy(r.H, g.H, sizeof r.H);
        r.hypothesis = g.hypothesis, r.inliers = (int)g.inliers.size();
        REQUIRE(store(dir + "oneshot.bin", &r, sizeof r));
        REQUIRE(store(dir + "oneshot_list.bin", g.inliers.data(), sizeof(DMatch) * g.inliers.size()));
        const sift_cuda::PlanarGeometry plain = sift_cuda::verifyAffine(list, q, rows, t, rows, model, params, 2, 2);
        REQUIRE(plain.hypothesis == verified.hypothesis && std::memcmp(plain.H, verified.H, sizeof plain.H) == 0);
    }

    // the batched forms: the list twice; pair 0 is the single call, pair 1 the single call with seed + 1
    {
        std::vector<DMatch> twice = list;
        twice.insert(twice.end(), list.begin(), list.end());
        const Device dm2(twice.data(), sizeof(DMatch) * twice.size());
        const std::vector<sift_cuda::VerifyPair> pairs(2, sift_cuda::VerifyPair{q, t, rows, rows, n});
        const std::vector<sift_cuda::PlanarGeometry> g =
            v.verifyAffineBatchedHost(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, model, params);
        REQUIRE(g.size() == 2 && g[0].hypothesis == verified.hypothesis && std::memcmp(g[0].H, verified.H, sizeof verified.H) == 0);
        sift_cuda::VerifyParams next = params;
        next.seed = 1;
        const sift_cuda::PlanarGeometry one = v.verifyAffineHost(m, nullptr, n, q, 2, rows, t, 2, rows, model, next);
        REQUIRE(g[1].hypothesis == one.hypothesis && std::memcmp(g[1].H, one.H, sizeof one.H) == 0 && same(g[1].inliers, one.inliers));
        // device: verify both pairs, refine both, and pair 0 is the single refine
        const Device dres2(fill.data(), 2 * sizeof(AffineResult)), dmask2(fill.data(), 2 * (size_t)n), dacc2(fill.data(), 2 * sizeof(int));
        v.verifyAffineBatchedDevice(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, model, params, dres2.as<AffineResult>(), nullptr,
                                    nullptr, dmask2.as<uint8_t>());
        v.refineAffineBatchedDevice(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, model, params.max_error, rounds,
                                    dres2.as<AffineResult>(), dmask2.as<uint8_t>(), nullptr, nullptr, dacc2.as<int>());
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        const std::vector<AffineResult> r2 = dres2.read<AffineResult>();
        const std::vector<uint8_t> m2 = dmask2.read<uint8_t>();
        REQUIRE(std::memcmp(&r2[0], &refined, sizeof refined) == 0 && dacc2.read<int>()[0] == accepted);
        REQUIRE(std::memcmp(m2.data(), refined_mask.data(), (size_t)n) == 0);
        // the batched host refine on the batched device verify's state
        std::vector<AffineResult> hr(2, verified);
        std::vector<uint8_t> hm = verified_mask;
        hm.insert(hm.end(), verified_mask.begin(), verified_mask.end());
        std::vector<DMatch> out;
        std::vector<int> counts;
        const std::vector<int> acc = v.refineAffineBatchedHost(dm2.as<const DMatch>(), nullptr, pairs, 2, 2, model,
                                                               params.max_error, rounds, hr, hm, &out, &counts);
        REQUIRE(acc.size() == 2 && acc[0] == accepted && acc[1] == accepted && counts[0] == (int)refined_list.size());
        REQUIRE(std::memcmp(&hr[0], &refined, sizeof refined) == 0 && std::memcmp(&hr[1], &refined, sizeof refined) == 0);
        REQUIRE(std::memcmp(out.data(), refined_list.data(), sizeof(DMatch) * refined_list.size()) == 0);
    }

    // too few matches: the empty result, not an error
    {
        const std::vector<DMatch> few(list.begin(), list.begin() + 1);
        const sift_cuda::PlanarGeometry e = sift_cuda::verifyAffine(few, q, rows, t, rows, model, params, 2, 2, rounds);
        REQUIRE(e.hypothesis == -1 && e.inliers.empty());
        for (float x : e.H) REQUIRE(x == 0.f);
    }

    // what the ABI refuses throws std::invalid_argument
    for (float bad : {0.f, -1.5f, NAN, INFINITY}) {
        sift_cuda::VerifyParams p = params;
        p.max_error = bad;
        REQUIRE(throws_invalid([&] { (void)sift_cuda::verifyAffine(list, q, rows, t, rows, model, p, 2, 2); }));
    }
    REQUIRE(throws_invalid([&] { (void)sift_cuda::verifyAffine(list, q, rows, t, rows, model, params, 1, 2); }));
    REQUIRE(throws_invalid([&] { (void)sift_cuda::verifyAffine(list, q, rows, t, rows, static_cast<AffineModel>(2), params, 2, 2); }));
    REQUIRE(throws_invalid([&] {
        v.refineAffineDevice(m, nullptr, n, q, 2, rows, t, 2, rows, model, params.max_error, 9, dres.as<AffineResult>(),
                             dmask.as<uint8_t>());
    }));
    std::printf("affine ok: model %d, hypothesis %d, %d -> %d inliers, %d accepted\n", (int)model, verified.hypothesis,
                verified.inliers, refined.inliers, accepted);
    return 0;
}
