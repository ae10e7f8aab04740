// sift_cuda::matchListGuidedBatchedDevice / matchListEpipolarBatchedDevice /
// projectHomographyBatchedDevice on the GPU, checked against the C ABI and
// against the bytes the Python test computed with the numpy rule.
//
// argv: batch.bin window.bin epipolar.bin
//   batch.bin    int P, radius (float), max_error (float); per pair int nq, nt;
//                then per pair q (nq x 128 half), t (nt x 128 half),
//                q_xy (nq x 2 float), t_xy (nt x 2 float), F (9 float)
//   window.bin / epipolar.bin   per pair int count, count DMatch records
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <stdexcept>
#include <vector>

#include "sift_cuda/Detector.hh"
#include "sift_cuda/Verify.hh"
#include "sift_hip.h"

#define REQUIRE(c)                                                   \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                \
        }                                                            \
    } while (0)

namespace {

std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Dev {
    void* p = nullptr;
    Dev(const void* src, size_t bytes) {
        if (sift_hip_malloc(&p, bytes ? bytes : 1) != 0) throw std::runtime_error("malloc");
        if (bytes && src && sift_hip_memcpy_h2d(p, src, bytes) != 0) throw std::runtime_error("h2d");
    }
    ~Dev() { (void)sift_hip_free(p); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

template <class T>
std::vector<T> download(const Dev& d, size_t n) {
    std::vector<T> out(n);
    if (n && sift_hip_memcpy_d2h(out.data(), d.p, sizeof(T) * n) != 0) throw std::runtime_error("d2h");
    return out;
}

// Per pair the first counts[p] records of its rows, as the expected file lays them out.
std::vector<char> packed(const std::vector<sift_cuda::DMatch>& rows, const std::vector<int>& counts,
                         const std::vector<int>& nq) {
    std::vector<char> out;
    size_t row0 = 0;
    for (size_t p = 0; p < nq.size(); p++) {
        const char* c = reinterpret_cast<const char*>(&counts[p]);
        out.insert(out.end(), c, c + 4);
        const char* r = reinterpret_cast<const char*>(rows.data() + row0);
        out.insert(out.end(), r, r + sizeof(sift_cuda::DMatch) * (size_t)counts[p]);
        row0 += (size_t)nq[p];
    }
    return out;
}

template <class F>
bool throws_invalid(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    REQUIRE(argc == 4);
    const std::vector<char> in = slurp(argv[1]), want_window = slurp(argv[2]), want_epipolar = slurp(argv[3]);
    const char* at = in.data();
    auto take = [&](void* dst, size_t bytes) {
        std::memcpy(dst, at, bytes);
        at += bytes;
    };
    int P = 0;
    float radius = 0.f, max_error = 0.f;
    take(&P, 4);
    take(&radius, 4);
    take(&max_error, 4);
    REQUIRE(P >= 1 && P <= 8);
    std::vector<int> nq(P), nt(P);
    for (int p = 0; p < P; p++) {
        take(&nq[p], 4);
        take(&nt[p], 4);
    }
    std::vector<Dev*> owned;
    std::vector<sift_cuda::GuidedPair> pairs(P);
    std::vector<float> geometry((size_t)P * 13, std::numeric_limits<float>::quiet_NaN());  // records of 52 bytes
    int rows = 0, cap = 1;
    for (int p = 0; p < P; p++) {
        auto up = [&](size_t bytes) {
            owned.push_back(new Dev(at, bytes));
            at += bytes;
            return owned.back()->p;
        };
        pairs[p].des = static_cast<const sift_cuda::Half*>(up((size_t)nq[p] * 256));
        pairs[p].num_des = nq[p];
        pairs[p].src = static_cast<const sift_cuda::Half*>(up((size_t)nt[p] * 256));
        pairs[p].num_src = nt[p];
        pairs[p].des_xy = static_cast<const float*>(up((size_t)nq[p] * 8));
        pairs[p].src_xy = static_cast<const float*>(up((size_t)nt[p] * 8));
        take(&geometry[(size_t)p * 13], 36);
        rows += nq[p];
        cap = std::max(cap, std::max(nq[p], nt[p]));
    }
    REQUIRE(at == in.data() + in.size());
    const Dev dgeo(geometry.data(), geometry.size() * 4);
    const Dev out(nullptr, sizeof(sift_cuda::DMatch) * (size_t)rows), counts(nullptr, 4 * (size_t)P);
    const Dev out_abi(nullptr, sizeof(sift_cuda::DMatch) * (size_t)rows), counts_abi(nullptr, 4 * (size_t)P);

    sift_cuda::BatchMatcher matcher(cap, cap, 2 * P), second(cap, cap, P);
    std::vector<const uint16_t*> q(P), t(P);
    std::vector<sift_hip_match_positions> pos(P);
    for (int p = 0; p < P; p++) {
        q[p] = reinterpret_cast<const uint16_t*>(pairs[p].des);
        t[p] = reinterpret_cast<const uint16_t*>(pairs[p].src);
        pos[p] = sift_hip_match_positions{pairs[p].des_xy, pairs[p].src_xy};
    }
    sift_hip_match_filter f;
    sift_hip_default_match_filter(&f);

    // the window gate: the C++ surface, the C ABI on another matcher (two passes: max_pairs = P), the numpy rule
    sift_cuda::matchListGuidedBatchedDevice(matcher, pairs, 2, 2, radius, {}, out.as<sift_cuda::DMatch>(), counts.as<int>());
    REQUIRE(sift_hip_match_list_guided_batched(second.handle(), P, q.data(), nq.data(), t.data(), nt.data(), pos.data(), 2, 2,
                                               radius, &f, out_abi.as<sift_hip_dmatch>(), counts_abi.as<int>(),
                                               nullptr) == 0);
    REQUIRE(sift_hip_device_sync() == 0);
    std::vector<char> got = packed(download<sift_cuda::DMatch>(out, rows), download<int>(counts, P), nq);
    REQUIRE(got == packed(download<sift_cuda::DMatch>(out_abi, rows), download<int>(counts_abi, P), nq));
    REQUIRE(got == want_window);

    // the epipolar gate, F read from the device records
    sift_cuda::matchListEpipolarBatchedDevice(matcher, pairs, 2, 2, std::numeric_limits<float>::infinity(), dgeo.p, 52,
                                              max_error, {}, out.as<sift_cuda::DMatch>(), counts.as<int>());
    REQUIRE(sift_hip_match_list_epipolar_batched(second.handle(), P, q.data(), nq.data(), t.data(), nt.data(), pos.data(), 2,
                                                 2, std::numeric_limits<float>::infinity(), dgeo.p, 52, max_error, &f,
                                                 out_abi.as<sift_hip_dmatch>(), counts_abi.as<int>(), nullptr) == 0);
    REQUIRE(sift_hip_device_sync() == 0);
    got = packed(download<sift_cuda::DMatch>(out, rows), download<int>(counts, P), nq);
    REQUIRE(got == packed(download<sift_cuda::DMatch>(out_abi, rows), download<int>(counts_abi, P), nq));
    REQUIRE(got == want_epipolar);

    // the batched projection against the single call per set (the records' nine floats serve as H)
    std::vector<Dev*> proj, proj_one;
    std::vector<sift_cuda::ProjectSet> sets(P);
    for (int p = 0; p < P; p++) {
        proj.push_back(new Dev(nullptr, (size_t)nq[p] * 8));
        proj_one.push_back(new Dev(nullptr, (size_t)nq[p] * 8));
        sets[p] = sift_cuda::ProjectSet{pairs[p].des_xy, nq[p], proj[p]->as<float>()};
        sift_cuda::projectHomographyDevice(dgeo.as<float>() + 13 * p, pairs[p].des_xy, 2, nq[p], proj_one[p]->as<float>());
    }
    sift_cuda::projectHomographyBatchedDevice(dgeo.p, 52, sets, 2);
    REQUIRE(sift_hip_device_sync() == 0);
    for (int p = 0; p < P; p++) {
        const std::vector<uint32_t> a = download<uint32_t>(*proj[p], (size_t)nq[p] * 2);
        REQUIRE(a == download<uint32_t>(*proj_one[p], (size_t)nq[p] * 2));
    }

    // what the ABI refuses throws std::invalid_argument
    auto* o = out.as<sift_cuda::DMatch>();
    int* c = counts.as<int>();
    REQUIRE(throws_invalid([&] { sift_cuda::matchListGuidedBatchedDevice(matcher, pairs, 2, 2, 0.f, {}, o, c); }));
    REQUIRE(throws_invalid([&] { sift_cuda::matchListGuidedBatchedDevice(matcher, pairs, 1, 2, radius, {}, o, c); }));
    REQUIRE(throws_invalid([&] { sift_cuda::matchListGuidedBatchedDevice(matcher, {}, 2, 2, radius, {}, o, c); }));
    REQUIRE(throws_invalid(
        [&] { sift_cuda::matchListEpipolarBatchedDevice(matcher, pairs, 2, 2, radius, nullptr, 52, max_error, {}, o, c); }));
    REQUIRE(throws_invalid(
        [&] { sift_cuda::matchListEpipolarBatchedDevice(matcher, pairs, 2, 2, radius, dgeo.p, 34, max_error, {}, o, c); }));
    REQUIRE(throws_invalid(
        [&] { sift_cuda::matchListEpipolarBatchedDevice(matcher, pairs, 2, 2, radius, dgeo.p, 52, 0.f, {}, o, c); }));
    REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyBatchedDevice(nullptr, 52, sets, 2); }));
    REQUIRE(throws_invalid([&] { sift_cuda::projectHomographyBatchedDevice(dgeo.p, 52, {}, 2); }));

    for (Dev* d : owned) delete d;
    for (Dev* d : proj) delete d;
    for (Dev* d : proj_one) delete d;
    std::printf("guided batched ok: %d pairs\n", P);
    return 0;
}
