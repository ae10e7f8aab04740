// The gated k-NN C++ surface on the GPU (tests/test_gpu_match_knn_gated_cxx.py): sift_cuda::matchKnnGuided /
// matchKnnEpipolar / matchKnnListGuided / matchKnnListEpipolar and the four batched device forms, on arrays the Python
// side wrote into the directory given as argv[1] -- the fp16 rows and positions (stride 3) of two pairs, the gates'
// numbers, and what sift_amd.cv.guided_knn / epipolar_knn / knn_records expect.  Every comparison is byte for byte.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
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

static std::string g_dir;

template <class T>
static std::vector<T> load(const std::string& name) {
    std::ifstream f(g_dir + "/" + name, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing " + name);
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes) f.read(reinterpret_cast<char*>(v.data()), bytes);
    return v;
}

// A host array on the device (freed at exit of the test: the process ends).
template <class T>
static T* upload(const std::vector<T>& v, size_t extra = 0) {
    void* p = nullptr;
    if (sift_hip_malloc(&p, (v.size() + extra) * sizeof(T) + 16) != SIFT_HIP_OK) throw std::runtime_error("malloc");
    if (!v.empty() && sift_hip_memcpy_h2d(p, v.data(), v.size() * sizeof(T)) != SIFT_HIP_OK)
        throw std::runtime_error("h2d");
    return static_cast<T*>(p);
}

template <class T>
static std::vector<T> download(const T* p, size_t n) {
    std::vector<T> v(n);
    if (n && sift_hip_memcpy_d2h(v.data(), p, n * sizeof(T)) != SIFT_HIP_OK) throw std::runtime_error("d2h");
    return v;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// Rows of DMatch -> the flat list in (queryIdx, rank) order.
static std::vector<sift_cuda::DMatch> flat(const std::vector<std::vector<sift_cuda::DMatch>>& rows) {
    std::vector<sift_cuda::DMatch> out;
    for (const auto& r : rows) out.insert(out.end(), r.begin(), r.end());
    return out;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 2);
    g_dir = argv[1];
    using sift_cuda::DMatch;
    using sift_cuda::Half;
    const auto meta = load<float>("meta.bin");  // nq0 nt0 nq1 nt1 k radius max_error cap F[9]
    REQUIRE(meta.size() == 17);
    const int nq[2] = {(int)meta[0], (int)meta[2]}, nt[2] = {(int)meta[1], (int)meta[3]}, k = (int)meta[4];
    const float radius = meta[5], max_error = meta[6], cap = meta[7];
    Half *dq[2], *dt[2];
    float *dqxy[2], *dtxy[2];
    for (int p = 0; p < 2; p++) {
        const std::string s = std::to_string(p);
        dq[p] = reinterpret_cast<Half*>(upload(load<uint16_t>("q" + s + ".bin")));
        dt[p] = reinterpret_cast<Half*>(upload(load<uint16_t>("t" + s + ".bin")));
        dqxy[p] = upload(load<float>("qxy" + s + ".bin"));
        dtxy[p] = upload(load<float>("txy" + s + ".bin"));
    }
    sift_cuda::MatchGate win;
    win.query_xy = dqxy[0], win.train_xy = dtxy[0], win.radius = radius;
    sift_cuda::EpipolarGate band;
    band.query_xy = dqxy[0], band.train_xy = dtxy[0], band.max_error = max_error;
    for (int e = 0; e < 9; e++) band.F[e] = meta[8 + (size_t)e];
    const sift_cuda::DeviceBuffer<Half> q0(dq[0], (size_t)nq[0] * 128), t0(dt[0], (size_t)nt[0] * 128);

    // single pair, synchronous: the rows are the table's records, the lists the capped records
    REQUIRE(same(flat(sift_cuda::matchKnnGuided(q0, nq[0], t0, nt[0], win, k)), load<DMatch>("rows_window0.bin")));
    REQUIRE(same(flat(sift_cuda::matchKnnEpipolar(q0, nq[0], t0, nt[0], band, k)), load<DMatch>("rows_band0.bin")));
    REQUIRE(same(sift_cuda::matchKnnListGuided(q0, nq[0], t0, nt[0], win, k, cap), load<DMatch>("list_window0.bin")));
    REQUIRE(same(sift_cuda::matchKnnListEpipolar(q0, nq[0], t0, nt[0], band, k, cap), load<DMatch>("list_band0.bin")));
    REQUIRE((int)sift_cuda::matchKnnGuided(q0, nq[0], t0, nt[0], win, k).size() == nq[0]);

    // the batched device forms on both pairs
    std::vector<sift_cuda::GuidedPair> pairs(2);
    for (int p = 0; p < 2; p++) pairs[(size_t)p] = sift_cuda::GuidedPair{dq[p], nq[p], dt[p], nt[p], dqxy[p], dtxy[p]};
    const size_t rows = (size_t)nq[0] + nq[1];
    sift_cuda::BatchMatcher bm(std::max(nq[0], nq[1]), std::max(nt[0], nt[1]), 2);
    int* idx = upload(std::vector<int>(rows * k, -7));
    float* d2 = upload(std::vector<float>(rows * k, -7.f));
    DMatch* out = upload(std::vector<DMatch>(rows * k, DMatch{-7, -7, -7, -7.f}));
    int* counts = upload(std::vector<int>(2, -7));
    float* geo = upload(std::vector<float>(meta.begin() + 8, meta.end()), 9);
    REQUIRE(sift_hip_memcpy_h2d(geo + 9, meta.data() + 8, 36) == SIFT_HIP_OK);  // pair 1's record: the same F
    sift_cuda::matchKnnGuidedBatchedDevice(bm, pairs, 3, 3, radius, k, idx, d2);
    REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
    REQUIRE(same(download(idx, rows * k), load<int>("idx_window.bin")) && same(download(d2, rows * k), load<float>("d2_window.bin")));
    sift_cuda::matchKnnEpipolarBatchedDevice(bm, pairs, 3, 3, INFINITY, geo, 36, max_error, k, idx, d2);
    REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
    REQUIRE(same(download(idx, rows * k), load<int>("idx_band.bin")) && same(download(d2, rows * k), load<float>("d2_band.bin")));
    for (int band_gate = 0; band_gate < 2; band_gate++) {
        if (band_gate)
            sift_cuda::matchKnnListEpipolarBatchedDevice(bm, pairs, 3, 3, INFINITY, geo, 36, max_error, k, cap, out, counts);
        else
            sift_cuda::matchKnnListGuidedBatchedDevice(bm, pairs, 3, 3, radius, k, cap, out, counts);
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        const auto n = download(counts, 2);
        const std::string g = band_gate ? "band" : "window";
        const auto e0 = load<DMatch>("list_" + g + "0.bin"), e1 = load<DMatch>("blist_" + g + "1.bin");
        REQUIRE(n[0] == (int)e0.size() && n[1] == (int)e1.size());
        REQUIRE(same(download(out, e0.size()), e0) && same(download(out + (size_t)k * nq[0], e1.size()), e1));
    }

    // what the ABI refuses throws
    int thrown = 0;
    for (int bad : {0, 9})
        try {
            (void)sift_cuda::matchKnnGuided(q0, nq[0], t0, nt[0], win, bad);
        } catch (const std::invalid_argument&) {
            thrown++;
        }
    sift_cuda::MatchGate nogate = win;
    nogate.radius = 0.f;
    try {
        (void)sift_cuda::matchKnnListGuided(q0, nq[0], t0, nt[0], nogate, k);
    } catch (const std::invalid_argument&) {
        thrown++;
    }
    sift_cuda::EpipolarGate zero = band;
    for (float& f : zero.F) f = 0.f;
    try {
        (void)sift_cuda::matchKnnEpipolar(q0, nq[0], t0, nt[0], zero, k);
    } catch (const std::invalid_argument&) {
        thrown++;
    }
    try {
        sift_cuda::matchKnnEpipolarBatchedDevice(bm, pairs, 3, 3, INFINITY, geo, 34, max_error, k, idx, d2);
    } catch (const std::invalid_argument&) {
        thrown++;
    }
    REQUIRE(thrown == 5);
    REQUIRE(sift_cuda::matchKnnListEpipolar(q0, 0, t0, nt[0], band, k).empty());
    std::printf("match knn gated ok: %d x %d and %d x %d, k = %d\n", nq[0], nt[0], nq[1], nt[1], k);
    return 0;
}
