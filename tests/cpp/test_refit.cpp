// The refit forms of sift_cuda::Verifier and the `refit` argument of verifyFundamental / verifyHomography on the GPU
// (tests/test_gpu_refit_cxx.py writes the inputs and the bytes the Python surface returns; see there for the files).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
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

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

struct Reader {
    const std::vector<char>& b;
    size_t at = 0;
    template <class T>
    T get() {
        T v;
        std::memcpy(&v, b.data() + at, sizeof v);
        at += sizeof v;
        return v;
    }
    template <class T>
    std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (n) std::memcpy(v.data(), b.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

template <class T>
static T* upload(const std::vector<T>& v) {
    void* p = nullptr;
    if (sift_hip_malloc(&p, v.size() * sizeof(T) + 1) != SIFT_HIP_OK) return nullptr;
    if (!v.empty() && sift_hip_memcpy_h2d(p, v.data(), v.size() * sizeof(T)) != SIFT_HIP_OK) return nullptr;
    return static_cast<T*>(p);
}

// One model: Record is VerifyResult / HomographyResult, the member pointers select the model's calls.
template <class Record, class Geometry, class Verify, class Refine, class RefineHost, class OneShot>
static int run(Reader& in, const std::vector<char>& want, Verify verify, Refine refine, RefineHost refineHost,
               OneShot oneShot, float (Geometry::*model)[9]) {
    const int n = in.get<int>(), nq = in.get<int>(), nt = in.get<int>(), K = in.get<int>(), rounds = in.get<int>();
    const float max_error = in.get<float>();
    const auto matches = in.many<sift_cuda::DMatch>((size_t)n);
    const auto q_xy = in.many<float>(2 * (size_t)nq), t_xy = in.many<float>(2 * (size_t)nt);
    Reader w{want};
    const auto record = w.many<char>(sizeof(Record));
    const int accepted = w.get<int>(), k = w.get<int>();
    const auto list = w.many<sift_cuda::DMatch>((size_t)k);
    const auto mask = w.many<uint8_t>((size_t)n);

    sift_cuda::DMatch* dm = upload(matches);
    float *dq = upload(q_xy), *dt = upload(t_xy);
    REQUIRE(dm && dq && dt);
    sift_cuda::VerifyParams params;
    params.hypotheses = K, params.max_error = max_error;

    // The one shot with refit rounds.
    const Geometry g = oneShot(matches, dq, nq, dt, nt, params, rounds);
    Record expect;
    std::memcpy(&expect, record.data(), sizeof expect);
    REQUIRE(std::memcmp(g.*model, &expect, 36) == 0 && g.hypothesis == expect.hypothesis);
    REQUIRE((int)g.inliers.size() == k && (k == 0 || std::memcmp(g.inliers.data(), list.data(), sizeof(sift_cuda::DMatch) * k) == 0));

    // verify -> refine on the device, one stream, no read-back between them.
    sift_cuda::Verifier v(n, K);
    void *dres = nullptr, *dmask = nullptr, *dout = nullptr, *dints = nullptr;
    REQUIRE(sift_hip_malloc(&dres, sizeof(Record)) == SIFT_HIP_OK && sift_hip_malloc(&dmask, (size_t)n) == SIFT_HIP_OK &&
            sift_hip_malloc(&dout, sizeof(sift_cuda::DMatch) * (size_t)n) == SIFT_HIP_OK &&
            sift_hip_malloc(&dints, 2 * sizeof(int)) == SIFT_HIP_OK);
    (v.*verify)(dm, nullptr, n, dq, 2, nq, dt, 2, nt, params, static_cast<Record*>(dres), nullptr, nullptr,
                static_cast<uint8_t*>(dmask), nullptr);
    Record verified;
    std::vector<uint8_t> verified_mask((size_t)n);
    REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_d2h(&verified, dres, sizeof verified) == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_d2h(verified_mask.data(), dmask, (size_t)n) == SIFT_HIP_OK);
    (v.*refine)(dm, nullptr, n, dq, 2, nq, dt, 2, nt, max_error, rounds, static_cast<Record*>(dres),
                static_cast<uint8_t*>(dmask), static_cast<sift_cuda::DMatch*>(dout), static_cast<int*>(dints),
                static_cast<int*>(dints) + 1, nullptr);
    REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
    Record got;
    int ints[2];
    std::vector<uint8_t> got_mask((size_t)n);
    std::vector<sift_cuda::DMatch> got_list((size_t)k);
    REQUIRE(sift_hip_memcpy_d2h(&got, dres, sizeof got) == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_d2h(ints, dints, sizeof ints) == SIFT_HIP_OK);
    REQUIRE(sift_hip_memcpy_d2h(got_mask.data(), dmask, (size_t)n) == SIFT_HIP_OK);
    REQUIRE(std::memcmp(&got, &expect, sizeof got) == 0 && ints[0] == k && ints[1] == accepted && got_mask == mask);
    if (k) REQUIRE(sift_hip_memcpy_d2h(got_list.data(), dout, sizeof(sift_cuda::DMatch) * k) == SIFT_HIP_OK);
    REQUIRE(k == 0 || std::memcmp(got_list.data(), list.data(), sizeof(sift_cuda::DMatch) * k) == 0);

    // The host form on the verified state read back above.
    std::vector<sift_cuda::DMatch> host_list;
    const int host_accepted = (v.*refineHost)(dm, nullptr, n, dq, 2, nq, dt, 2, nt, max_error, rounds, verified,
                                              verified_mask, &host_list);
    REQUIRE(host_accepted == accepted && std::memcmp(&verified, &expect, sizeof expect) == 0 && verified_mask == mask);
    REQUIRE((int)host_list.size() == k && (k == 0 || std::memcmp(host_list.data(), list.data(), sizeof(sift_cuda::DMatch) * k) == 0));
    for (void* p : {(void*)dm, (void*)dq, (void*)dt, dres, dmask, dout, dints}) (void)sift_hip_free(p);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const std::vector<char> input = slurp(argv[1]), f = slurp(argv[2]), h = slurp(argv[3]);
    Reader in{input};
    using sift_cuda::Verifier;
    auto oneF = [](const std::vector<sift_cuda::DMatch>& m, const float* q, int nq, const float* t, int nt,
                   const sift_cuda::VerifyParams& p, int refit) {
        return sift_cuda::verifyFundamental(m, q, nq, t, nt, p, 2, 2, refit);
    };
    auto oneH = [](const std::vector<sift_cuda::DMatch>& m, const float* q, int nq, const float* t, int nt,
                   const sift_cuda::VerifyParams& p, int refit) {
        return sift_cuda::verifyHomography(m, q, nq, t, nt, p, 2, 2, refit);
    };
    if (int rc = run<sift_cuda::VerifyResult, sift_cuda::TwoViewGeometry>(in, f, &Verifier::verifyDevice, &Verifier::refineDevice,
                                                                         &Verifier::refineHost, oneF,
                                                                         &sift_cuda::TwoViewGeometry::F))
        return rc;
    if (int rc = run<sift_cuda::HomographyResult, sift_cuda::PlanarGeometry>(
            in, h, &Verifier::verifyHomographyDevice, &Verifier::refineHomographyDevice, &Verifier::refineHomographyHost, oneH,
            &sift_cuda::PlanarGeometry::H))
        return rc;
    std::printf("refit cxx ok\n");
    return 0;
}
