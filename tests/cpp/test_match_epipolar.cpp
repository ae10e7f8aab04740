// sift_cuda::matchListEpipolar / matchEpipolar on the GPU
// (tests/test_gpu_match_epipolar_cxx.py): two uploaded sets of integer
// descriptors with positions on a quarter-pixel grid are matched under the
// fundamental matrix of a nearly rectified pair, and both results must equal a
// brute force over the gate done here on the host (this file is compiled with
// -ffp-contract=off: the rule of include/sift_hip.h is float32 without fused
// multiply-adds) -- exact integer distances, candidates by
// r r <= e2 (nq + nr) inside the window, ties to the lower index: matchEpipolar
// is the nearest candidate under matchBruteForce's ratio test (0.8 on squared
// distances), matchListEpipolar the default filter (ratio 0.8 on distances,
// cross check) on the top-2 of both directions, the reverse under F
// transposed.  A bad gate throws std::invalid_argument.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "sift_cuda/Detector.hh"
#include "sift_hip.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

// An integer 0..255 as IEEE binary16 bits.
static uint16_t half_bits(int v) {
    if (v == 0) return 0;
    int e = 0;
    while ((v >> (e + 1)) != 0) e++;
    return (uint16_t)(((e + 15) << 10) | (((unsigned)v << (10 - e)) & 0x3ff));
}

struct Lcg {
    uint32_t s;
    uint32_t next() { return s = s * 1664525u + 1013904223u, s >> 8; }
};

struct Set {
    int n;
    std::vector<int> desc;   // n x 128
    std::vector<float> xy;   // n x 3: x, y and a NaN that must not be read as a coordinate
};

struct Top2 {
    int i1 = -1, i2 = -1;
    float d1 = std::numeric_limits<float>::max(), d2 = std::numeric_limits<float>::max();
};

// The rule, spelled as in include/sift_hip.h.
static bool candidate(const float* F, float max_error, float radius, float qx, float qy, float tx, float ty) {
    const float a = (F[0] * qx + F[1] * qy) + F[2];
    const float b = (F[3] * qx + F[4] * qy) + F[5];
    const float c = (F[6] * qx + F[7] * qy) + F[8];
    const float nq = a * a + b * b;
    const float u = (F[0] * tx + F[3] * ty) + F[6];
    const float v = (F[1] * tx + F[4] * ty) + F[7];
    const float nr = u * u + v * v;
    const float r = (a * tx + b * ty) + c;
    const float e2 = max_error * max_error;
    return r * r <= e2 * (nq + nr) && std::fabs(tx - qx) <= radius && std::fabs(ty - qy) <= radius;
}

static std::vector<Top2> brute_force(const Set& q, const Set& t, const float* F, float max_error, float radius) {
    std::vector<Top2> out((size_t)q.n);
    for (int i = 0; i < q.n; i++) {
        Top2 b;
        for (int j = 0; j < t.n; j++) {
            if (!candidate(F, max_error, radius, q.xy[3 * i], q.xy[3 * i + 1], t.xy[3 * j], t.xy[3 * j + 1])) continue;
            long s = 0;
            for (int k = 0; k < 128; k++) {
                const long d = q.desc[128 * i + k] - t.desc[128 * j + k];
                s += d * d;
            }
            const float d = (float)s;
            if (b.i1 < 0 || d < b.d1) {
                b.i2 = b.i1, b.d2 = b.d1;
                b.i1 = j, b.d1 = d;
            } else if (b.i2 < 0 || d < b.d2) {
                b.i2 = j, b.d2 = d;
            }
        }
        out[(size_t)i] = b;
    }
    return out;
}

template <class T>
static T* upload(const void* src, size_t bytes) {
    void* p = nullptr;
    if (sift_hip_malloc(&p, bytes) != SIFT_HIP_OK || sift_hip_memcpy_h2d(p, src, bytes) != SIFT_HIP_OK) return nullptr;
    return static_cast<T*>(p);
}

int main() {
    const int nq = 150, nt = 290;  // two key groups of train rows, a partial query block
    const float inf = std::numeric_limits<float>::infinity();
    // x_t^T F x_q = 0.02 (tx - qx) - (ty - qy): epipolar lines of slope 0.02
    const float F[9] = {0.f, 0.f, 0.02f, 0.f, 0.f, -1.f, -0.02f, 1.f, 0.f};
    float Ft[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Ft[3 * c + r] = F[3 * r + c];
    const float max_error = 1.f;
    Lcg rng{12345u};
    Set q{nq, std::vector<int>((size_t)nq * 128), std::vector<float>((size_t)nq * 3)};
    Set t{nt, std::vector<int>((size_t)nt * 128), std::vector<float>((size_t)nt * 3)};
    for (Set* s : {&q, &t}) {
        for (int& v : s->desc) v = (int)(rng.next() % 128);
        for (int i = 0; i < s->n; i++) {
            s->xy[3 * (size_t)i] = 0.25f * (float)(rng.next() % 800);  // a 200 x 200 square
            s->xy[3 * (size_t)i + 1] = 0.25f * (float)(rng.next() % 800);
            s->xy[3 * (size_t)i + 2] = std::nanf("");
        }
    }
    // every third query gets a noisy copy among the train rows: on its epipolar line for half of them (25 pixels along
    // it: the match the gate finds), 5 pixels off it for the others (the global best the gate must not return)
    for (int i = 0; i < nq; i += 3) {
        const int j = (7 * i + 3) % nt;
        for (int k = 0; k < 128; k++) {
            const int v = q.desc[128 * i + k] + (int)(rng.next() % 5) - 2;
            t.desc[128 * j + k] = v < 0 ? 0 : v;
        }
        const bool on_line = (i / 3) % 2 == 0;
        t.xy[3 * (size_t)j] = q.xy[3 * (size_t)i] + 25.f;
        t.xy[3 * (size_t)j + 1] = q.xy[3 * (size_t)i + 1] + (on_line ? 0.5f : 5.5f);
    }
    std::vector<uint16_t> qh(q.desc.size()), th(t.desc.size());
    for (size_t i = 0; i < qh.size(); i++) qh[i] = half_bits(q.desc[i]);
    for (size_t i = 0; i < th.size(); i++) th[i] = half_bits(t.desc[i]);

    const std::vector<Top2> fwd = brute_force(q, t, F, max_error, inf), rev = brute_force(t, q, Ft, max_error, inf);
    int none = 0, one = 0, many = 0;
    for (const Top2& b : fwd) (b.i1 < 0 ? none : b.i2 < 0 ? one : many)++;
    REQUIRE(none > 0 && one > 0 && many > 0);

    sift_cuda::Half* dq = upload<sift_cuda::Half>(qh.data(), qh.size() * 2);
    sift_cuda::Half* dt = upload<sift_cuda::Half>(th.data(), th.size() * 2);
    float* dqxy = upload<float>(q.xy.data(), q.xy.size() * 4);
    float* dtxy = upload<float>(t.xy.data(), t.xy.size() * 4);
    REQUIRE(dq && dt && dqxy && dtxy);
    const sift_cuda::DeviceBuffer<sift_cuda::Half> bq(dq, qh.size()), bt(dt, th.size());
    sift_cuda::EpipolarGate gate;  // strides: the default 3; radius: the default, no window
    REQUIRE(gate.query_stride == 3 && gate.train_stride == 3 && gate.radius == inf && gate.max_error == 0.f);
    for (float f : gate.F) REQUIRE(f == 0.f);
    gate.query_xy = dqxy;
    gate.train_xy = dtxy;
    std::memcpy(gate.F, F, sizeof F);
    gate.max_error = max_error;

    // matchEpipolar: the nearest candidate under the ratio test on squared distances
    const std::vector<int> mg = sift_cuda::matchEpipolar(bq, nq, bt, nt, gate);
    REQUIRE((int)mg.size() == nq);
    int matched = 0;
    for (int i = 0; i < nq; i++) {
        const Top2& b = fwd[(size_t)i];
        const int expect = b.i1 < 0 ? -1 : (b.i2 < 0 || b.d1 < 0.8f * b.d2) ? b.i1 : -1;
        REQUIRE(mg[(size_t)i] == expect);
        matched += expect >= 0;
    }
    REQUIRE(matched > 0 && matched < nq);

    // matchListEpipolar: ratio 0.8 on distances and the cross check, on the top-2 of both directions
    std::vector<sift_cuda::DMatch> expect;
    for (int i = 0; i < nq; i++) {
        const Top2& b = fwd[(size_t)i];
        if (b.i1 < 0) continue;
        if (b.i2 >= 0) {
            const float rb = 0.8f * std::sqrt(b.d2);
            if (!(std::sqrt(b.d1) < rb)) continue;
        }
        if (rev[(size_t)b.i1].i1 != i) continue;
        expect.push_back(sift_cuda::DMatch{i, b.i1, 0, std::sqrt(b.d1)});
    }
    REQUIRE(!expect.empty() && (int)expect.size() < nq);
    const std::vector<sift_cuda::DMatch> got = sift_cuda::matchListEpipolar(bq, nq, bt, nt, gate);
    REQUIRE(got.size() == expect.size());
    REQUIRE(std::memcmp(got.data(), expect.data(), sizeof(sift_cuda::DMatch) * got.size()) == 0);

    // the band and a window along the line: the copies 25 pixels away fall outside a radius of 20
    sift_cuda::EpipolarGate windowed = gate;
    windowed.radius = 20.f;
    const std::vector<Top2> fw = brute_force(q, t, F, max_error, 20.f);
    const std::vector<int> mw = sift_cuda::matchEpipolar(bq, nq, bt, nt, windowed);
    for (int i = 0; i < nq; i++) {
        const Top2& b = fw[(size_t)i];
        REQUIRE(mw[(size_t)i] == (b.i1 < 0 ? -1 : (b.i2 < 0 || b.d1 < 0.8f * b.d2) ? b.i1 : -1));
    }
    REQUIRE(mw != mg);

    // F matters: with every row a candidate the copies off the line win
    sift_cuda::EpipolarGate open = gate;
    open.max_error = 1e30f;
    const std::vector<int> mo = sift_cuda::matchEpipolar(bq, nq, bt, nt, open);
    const std::vector<int> mb = sift_cuda::matchBruteForce(bq, nq, bt, nt);
    REQUIRE(mo == mb && mo != mg);

    REQUIRE(sift_cuda::matchListEpipolar(bq, 0, bt, nt, gate).empty());
    REQUIRE(sift_cuda::matchListEpipolar(bq, nq, bt, 0, gate).empty());

    // a bad gate throws, whichever entry point
    int thrown = 0;
    const int kBad = 9;
    for (int k = 0; k < kBad; k++) {
        sift_cuda::EpipolarGate bad = gate;
        if (k == 0) bad.radius = 0.f;
        if (k == 1) bad.max_error = std::nanf("");
        if (k == 2) bad.query_stride = 1;
        if (k == 3) bad.train_xy = nullptr;
        if (k == 4) bad.max_error = 0.f;
        if (k == 5) bad.max_error = inf;
        if (k == 6) bad.F[4] = std::nanf("");
        if (k == 7) bad.F[0] = inf;
        if (k == 8) std::memset(bad.F, 0, sizeof bad.F);
        try {
            (void)sift_cuda::matchListEpipolar(bq, nq, bt, nt, bad);
        } catch (const std::invalid_argument&) {
            thrown++;
        }
        try {
            (void)sift_cuda::matchEpipolar(bq, nq, bt, nt, bad);
        } catch (const std::invalid_argument&) {
            thrown++;
        }
    }
    REQUIRE(thrown == 2 * kBad);
    REQUIRE(sift_cuda::matchEpipolar(bq, nq, bt, nt, gate) == mg);  // the refused calls left the matchers usable

    for (void* p : {(void*)dq, (void*)dt, (void*)dqxy, (void*)dtxy}) sift_hip_free(p);
    std::printf("match epipolar ok: %zu mutual, %d one-way of %d queries (%d without a candidate, %d with one)\n",
                got.size(), matched, nq, none, one);
    return 0;
}
