// sift_cuda::verifyFundamental / Verifier on the GPU
// (tests/test_gpu_verify_cxx.py): a match list of 100 true pairs of a
// two-camera scene and 60 pairs of unrelated positions, its records indexing
// shuffled position arrays (stride 3, the third float a NaN that must not be
// read as a coordinate), is uploaded and verified; F, the winning hypothesis
// and the inlier records must equal, byte for byte, the plain C++ restatement
// of the rule of include/sift_hip.h in verify_rule.hh (this file is compiled
// with -ffp-contract=off).  A bad max_error throws std::invalid_argument.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "sift_cuda/Verify.hh"
#include "sift_hip.h"
#include "verify_rule.hh"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

struct Lcg {
    uint32_t s;
    uint32_t next() { return s = s * 1664525u + 1013904223u, s >> 8; }
    double unit() { return next() / 16777216.0; }
};

static float grid(double v) { return (float)(std::floor(v * 4.0 + 0.5) / 4.0); }

struct Device {
    void* p = nullptr;
    Device(const void* host, size_t bytes) {
        if (sift_hip_malloc(&p, bytes ? bytes : 1) != SIFT_HIP_OK) std::abort();
        if (bytes && sift_hip_memcpy_h2d(p, host, bytes) != SIFT_HIP_OK) std::abort();
    }
    ~Device() { (void)sift_hip_free(p); }
};

static bool same_list(const std::vector<sift_cuda::DMatch>& a, const std::vector<sift_cuda::DMatch>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(sift_cuda::DMatch) * a.size()) == 0);
}

int main() {
    const int n_in = 100, n_out = 60, n = n_in + n_out, rows = n + 6;
    Lcg rng{12345u};
    // positions: uniform on the quarter-pixel grid of a 200 x 200 frame, then the true pairs on top
    std::vector<float> qxy(3 * (size_t)rows, NAN), txy(3 * (size_t)rows, NAN);
    for (int i = 0; i < rows; i++) {
        qxy[3 * i] = grid(rng.unit() * 199), qxy[3 * i + 1] = grid(rng.unit() * 199);
        txy[3 * i] = grid(rng.unit() * 199), txy[3 * i + 1] = grid(rng.unit() * 199);
    }
    std::vector<int> qrow(rows), trow(rows);
    for (int i = 0; i < rows; i++) qrow[i] = trow[i] = i;
    for (int i = rows - 1; i > 0; i--) {
        std::swap(qrow[i], qrow[rng.next() % (uint32_t)(i + 1)]);
        std::swap(trow[i], trow[rng.next() % (uint32_t)(i + 1)]);
    }
    const double f = 180, c = 100, T[3] = {0.6, 0.1, 0.15};
    for (int i = 0; i < n_in;) {
        const double u = rng.unit() * 199, v = rng.unit() * 199, z = 3 + 5 * rng.unit();
        const double X = (u - c) / f * z + T[0], Y = (v - c) / f * z + T[1], Z = z + T[2];
        const double u2 = f * X / Z + c, v2 = f * Y / Z + c;
        if (u2 < 0 || u2 > 199 || v2 < 0 || v2 > 199) continue;
        qxy[3 * qrow[i]] = grid(u), qxy[3 * qrow[i] + 1] = grid(v);
        txy[3 * trow[i]] = grid(u2), txy[3 * trow[i] + 1] = grid(v2);
        i++;
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; i++) order[i] = i;
    for (int i = n - 1; i > 0; i--) std::swap(order[i], order[rng.next() % (uint32_t)(i + 1)]);
    std::vector<sift_cuda::DMatch> list((size_t)n);
    for (int j = 0; j < n; j++) list[j] = sift_cuda::DMatch{qrow[order[j]], trow[order[j]], 0, 100.f + (float)order[j]};
    list[17].trainIdx = rows;  // a record outside its position array: never an inlier, never read through

    const Device dq(qxy.data(), sizeof(float) * qxy.size()), dt(txy.data(), sizeof(float) * txy.size());
    const float* q = static_cast<const float*>(dq.p);
    const float* t = static_cast<const float*>(dt.p);

    sift_cuda::VerifyParams params;
    params.hypotheses = 512;
    params.seed = 3;
    const verify_rule::Result ref =
        verify_rule::ransac(list, qxy.data(), 3, rows, txy.data(), 3, rows, params.hypotheses, params.seed, params.max_error);
    REQUIRE(ref.hypothesis >= 0 && ref.valid > 400 && ref.valid < 512);
    int true_in = 0;
    for (const sift_cuda::DMatch& m : ref.list) true_in += m.distance < 100.f + n_in ? 1 : 0;
    REQUIRE(true_in >= 95 && (int)ref.list.size() - true_in <= 10);

    const sift_cuda::TwoViewGeometry g = sift_cuda::verifyFundamental(list, q, rows, t, rows, params);
    REQUIRE(g.hypothesis == ref.hypothesis);
    REQUIRE(std::memcmp(g.F, ref.F, sizeof g.F) == 0);
    REQUIRE(same_list(g.inliers, ref.list));
    for (const sift_cuda::DMatch& m : g.inliers) REQUIRE(m.trainIdx != rows);

    // the handle form, with the list's length on the device and records behind it that must not count
    {
        std::vector<sift_cuda::DMatch> padded = list;
        for (int j = 0; j < 40; j++) padded.push_back(list[(size_t)j]);
        const int count = n;
        const Device dm(padded.data(), sizeof(sift_cuda::DMatch) * padded.size()), dc(&count, sizeof count);
        sift_cuda::Verifier v((int)padded.size(), 512);
        const sift_cuda::TwoViewGeometry h =
            v.verifyHost(static_cast<const sift_cuda::DMatch*>(dm.p), static_cast<const int*>(dc.p), (int)padded.size(), q,
                         3, rows, t, 3, rows, params);
        REQUIRE(h.hypothesis == ref.hypothesis && std::memcmp(h.F, ref.F, sizeof h.F) == 0 && same_list(h.inliers, ref.list));
        // the device form
        sift_cuda::VerifyResult zero{};
        const Device dres(&zero, sizeof zero);
        v.verifyDevice(static_cast<const sift_cuda::DMatch*>(dm.p), static_cast<const int*>(dc.p), (int)padded.size(), q, 3,
                       rows, t, 3, rows, params, static_cast<sift_cuda::VerifyResult*>(dres.p));
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        sift_cuda::VerifyResult r{};
        REQUIRE(sift_hip_memcpy_d2h(&r, dres.p, sizeof r) == SIFT_HIP_OK);
        REQUIRE(r.hypothesis == ref.hypothesis && r.inliers == (int)ref.list.size() && r.matches == n &&
                r.valid_hypotheses == ref.valid && std::memcmp(r.F, ref.F, sizeof r.F) == 0);
    }

    // fewer than 8 matches: the empty result, not an error
    {
        const std::vector<sift_cuda::DMatch> few(list.begin(), list.begin() + 7);
        const sift_cuda::TwoViewGeometry e = sift_cuda::verifyFundamental(few, q, rows, t, rows, params);
        REQUIRE(e.hypothesis == -1 && e.inliers.empty());
        for (float x : e.F) REQUIRE(x == 0.f);
        const sift_cuda::TwoViewGeometry none = sift_cuda::verifyFundamental({}, q, rows, t, rows, params);
        REQUIRE(none.hypothesis == -1 && none.inliers.empty());
    }

    // what the ABI refuses throws std::invalid_argument
    for (float bad : {0.f, -1.5f, NAN, INFINITY}) {
        sift_cuda::VerifyParams p = params;
        p.max_error = bad;
        bool thrown = false;
        try {
            (void)sift_cuda::verifyFundamental(list, q, rows, t, rows, p);
        } catch (const std::invalid_argument&) {
            thrown = true;
        }
        REQUIRE(thrown);
    }
    {
        bool thrown = false;
        try {
            (void)sift_cuda::verifyFundamental(list, q, rows, t, rows, params, 1, 3);  // a stride below 2
        } catch (const std::invalid_argument&) {
            thrown = true;
        }
        REQUIRE(thrown);
        thrown = false;
        try {
            sift_cuda::Verifier v(0, 64);
        } catch (const std::invalid_argument&) {
            thrown = true;
        }
        REQUIRE(thrown);
    }
    std::printf("verify ok: hypothesis %d, %zu inliers (%d true), %d valid hypotheses\n", ref.hypothesis, ref.list.size(),
                true_in, ref.valid);
    return 0;
}
