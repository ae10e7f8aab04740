// sift_cuda::verifyHomography / Verifier::verifyHomography* / projectHomographyDevice
// on the GPU (tests/test_gpu_homography_cxx.py): the main case of
// tests/homography_cases.py and what sift_amd.cv.ransac_homography and
// cv.project_homography make of it, dumped by the Python test into the directory
// given as argv[1]:
//   matches.bin   n sift_cuda::DMatch records        q_xy.bin / t_xy.bin   rows x 2 float
//   ref.bin       sift_cuda::HomographyResult (H, inliers, hypothesis, matches, valid_hypotheses)
//   list.bin      the inlier records                  proj.bin              rows x 2 float: q_xy through H
// H, the winner, the inlier records and the projected positions must equal the
// dump byte for byte.  What the ABI refuses throws std::invalid_argument.
#include <cmath>
#include <cstdint>
#include <cstdio>
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

struct Device {
    void* p = nullptr;
    Device(const void* host, size_t bytes) {
        if (sift_hip_malloc(&p, bytes ? bytes : 1) != SIFT_HIP_OK) std::abort();
        if (bytes && host && sift_hip_memcpy_h2d(p, host, bytes) != SIFT_HIP_OK) std::abort();
    }
    ~Device() { (void)sift_hip_free(p); }
};

static bool same_list(const std::vector<sift_cuda::DMatch>& a, const std::vector<sift_cuda::DMatch>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(sift_cuda::DMatch) * a.size()) == 0);
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
    REQUIRE(argc == 2);
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<sift_cuda::DMatch> list = load<sift_cuda::DMatch>(dir + "matches.bin");
    const std::vector<float> qxy = load<float>(dir + "q_xy.bin"), txy = load<float>(dir + "t_xy.bin");
    const std::vector<sift_cuda::HomographyResult> refs = load<sift_cuda::HomographyResult>(dir + "ref.bin");
    const std::vector<sift_cuda::DMatch> ref_list = load<sift_cuda::DMatch>(dir + "list.bin");
    const std::vector<float> ref_proj = load<float>(dir + "proj.bin");
    REQUIRE(!list.empty() && !qxy.empty() && qxy.size() == txy.size() && refs.size() == 1 && ref_proj.size() == qxy.size());
    const sift_cuda::HomographyResult ref = refs[0];
    const int n = (int)list.size(), rows = (int)qxy.size() / 2;
    REQUIRE(ref.matches == n && ref.hypothesis >= 0 && ref.inliers == (int)ref_list.size() && ref.inliers >= 4);

    const Device dq(qxy.data(), sizeof(float) * qxy.size()), dt(txy.data(), sizeof(float) * txy.size());
    const float* q = static_cast<const float*>(dq.p);
    const float* t = static_cast<const float*>(dt.p);

    sift_cuda::VerifyParams params;
    params.hypotheses = 512;
    params.seed = 0;

    const sift_cuda::PlanarGeometry g = sift_cuda::verifyHomography(list, q, rows, t, rows, params, 2, 2);
    REQUIRE(g.hypothesis == ref.hypothesis);
    REQUIRE(std::memcmp(g.H, ref.H, sizeof g.H) == 0);
    REQUIRE(same_list(g.inliers, ref_list));

    // the handle form, with the list's length on the device and records behind it that must not count
    {
        std::vector<sift_cuda::DMatch> padded = list;
        for (int j = 0; j < 40; j++) padded.push_back(list[(size_t)j]);
        const int count = n;
        const Device dm(padded.data(), sizeof(sift_cuda::DMatch) * padded.size()), dc(&count, sizeof count);
        sift_cuda::Verifier v((int)padded.size(), 512);
        const sift_cuda::PlanarGeometry h =
            v.verifyHomographyHost(static_cast<const sift_cuda::DMatch*>(dm.p), static_cast<const int*>(dc.p),
                                   (int)padded.size(), q, 2, rows, t, 2, rows, params);
        REQUIRE(h.hypothesis == ref.hypothesis && std::memcmp(h.H, ref.H, sizeof h.H) == 0 && same_list(h.inliers, ref_list));
        // the device form, and the projection reading H from the result record on the device
        sift_cuda::HomographyResult zero{};
        const Device dres(&zero, sizeof zero), dproj(nullptr, sizeof(float) * qxy.size());
        v.verifyHomographyDevice(static_cast<const sift_cuda::DMatch*>(dm.p), static_cast<const int*>(dc.p),
                                 (int)padded.size(), q, 2, rows, t, 2, rows, params,
                                 static_cast<sift_cuda::HomographyResult*>(dres.p));
        sift_cuda::projectHomographyDevice(static_cast<const float*>(dres.p), q, 2, rows, static_cast<float*>(dproj.p));
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        sift_cuda::HomographyResult r{};
        REQUIRE(sift_hip_memcpy_d2h(&r, dres.p, sizeof r) == SIFT_HIP_OK);
        REQUIRE(std::memcmp(&r, &ref, sizeof r) == 0);
        std::vector<float> proj(qxy.size());
        REQUIRE(sift_hip_memcpy_d2h(proj.data(), dproj.p, sizeof(float) * proj.size()) == SIFT_HIP_OK);
        REQUIRE(std::memcmp(proj.data(), ref_proj.data(), sizeof(float) * proj.size()) == 0);
        // a fundamental call on the same verifier still runs (the models share the handle)
        const sift_cuda::TwoViewGeometry f =
            v.verifyHost(static_cast<const sift_cuda::DMatch*>(dm.p), static_cast<const int*>(dc.p), (int)padded.size(), q, 2,
                         rows, t, 2, rows, params);
        REQUIRE(f.hypothesis >= -1);
    }

    // fewer than 4 matches: the empty result, not an error
    {
        const std::vector<sift_cuda::DMatch> few(list.begin(), list.begin() + 3);
        const sift_cuda::PlanarGeometry e = sift_cuda::verifyHomography(few, q, rows, t, rows, params, 2, 2);
        REQUIRE(e.hypothesis == -1 && e.inliers.empty());
        for (float x : e.H) REQUIRE(x == 0.f);
        const sift_cuda::PlanarGeometry none = sift_cuda::verifyHomography({}, q, rows, t, rows, params, 2, 2);
        REQUIRE(none.hypothesis == -1 && none.inliers.empty());
    }

    // what the ABI refuses throws std::invalid_argument
    for (float bad : {0.f, -1.5f, NAN, INFINITY}) {
        sift_cuda::VerifyParams p = params;
        p.max_error = bad;
        REQUIRE(throws_invalid([&] { (void)sift_cuda::verifyHomography(list, q, rows, t, rows, p, 2, 2); }));
    }
    REQUIRE(throws_invalid([&] { (void)sift_cuda::verifyHomography(list, q, rows, t, rows, params, 1, 2); }));
    {
        const Device dout(nullptr, sizeof(float) * qxy.size());
        float* out = static_cast<float*>(dout.p);
        REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyDevice(nullptr, q, 2, rows, out); }));
        REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyDevice(t, q, 1, rows, out); }));
        REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyDevice(t, q, 2, -1, out); }));
        REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyDevice(t, q, 2, rows, nullptr); }));
        REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyDevice(t, out, 2, rows, out + 2); }));  // a partial overlap
        sift_cuda::projectHomographyDevice(t, q, 2, 0, nullptr);  // nothing to do
    }
    std::printf("homography ok: hypothesis %d, %d inliers, %d valid hypotheses\n", ref.hypothesis, ref.inliers,
                ref.valid_hypotheses);
    return 0;
}
