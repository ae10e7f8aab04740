// sift_cuda::Verifier's batched host forms on the GPU
// (tests/test_gpu_verify_batched_cxx.py): the batch the Python test wrote to
// a file -- tests/verify_batched_cases.py's MIXED: per pair a buffer of cap
// records, the number that counts, and two position arrays -- is uploaded and
// verified in one call per model; every pair's model, winning hypothesis and
// inlier records must equal, byte for byte, the expected bytes the Python test
// wrote from the numpy rule (pair p with the seed + p).
//
//   test_verify_batched <batch file> <expected fundamental> <expected homography>
//
// Batch file, little endian: int32 P, K; uint32 seed; float max_error; per pair
// int32 cap, count, nq, nt; the match rows (sum of cap x 16 bytes); per pair its
// query rows (nq x 2 floats), then its train rows (nt x 2 floats).  The file
// holds the fundamental batch; the homography batch follows in the same format.
// Expected file: per pair 9 floats, int32 hypothesis, int32 inliers, then that
// many records.
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

struct Device {
    void* p = nullptr;
    Device(const void* host, size_t bytes) {
        if (sift_hip_malloc(&p, bytes ? bytes : 1) != SIFT_HIP_OK) std::abort();
        if (bytes && sift_hip_memcpy_h2d(p, host, bytes) != SIFT_HIP_OK) std::abort();
    }
    Device(const Device&) = delete;
    ~Device() { (void)sift_hip_free(p); }
};

struct Reader {
    std::FILE* f;
    explicit Reader(const char* path) : f(std::fopen(path, "rb")) {
        if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    }
    ~Reader() { std::fclose(f); }
    template <class T>
    std::vector<T> take(size_t n) {
        std::vector<T> v(n);
        if (n && std::fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short file");
        return v;
    }
    template <class T>
    T one() {
        return take<T>(1)[0];
    }
};

struct Batch {
    int P = 0, K = 0;
    uint32_t seed = 0;
    float max_error = 0;
    std::vector<int> cap, count, nq, nt;
    std::vector<sift_cuda::DMatch> rows;
    std::vector<std::vector<float>> q, t;
    explicit Batch(Reader& r) {
        P = r.one<int32_t>(), K = r.one<int32_t>(), seed = r.one<uint32_t>(), max_error = r.one<float>();
        size_t total = 0;
        for (int p = 0; p < P; p++) {
            cap.push_back(r.one<int32_t>()), count.push_back(r.one<int32_t>());
            nq.push_back(r.one<int32_t>()), nt.push_back(r.one<int32_t>());
            total += (size_t)cap.back();
        }
        rows = r.take<sift_cuda::DMatch>(total);
        for (int p = 0; p < P; p++) {
            q.push_back(r.take<float>(2 * (size_t)nq[p]));
            t.push_back(r.take<float>(2 * (size_t)nt[p]));
        }
    }
};

struct Expected {
    float model[9];
    int hypothesis;
    std::vector<sift_cuda::DMatch> list;
};

static std::vector<Expected> expected(const char* path, int P) {
    Reader r(path);
    std::vector<Expected> out((size_t)P);
    for (Expected& e : out) {
        const std::vector<float> m = r.take<float>(9);
        std::memcpy(e.model, m.data(), sizeof e.model);
        e.hypothesis = r.one<int32_t>();
        e.list = r.take<sift_cuda::DMatch>((size_t)r.one<int32_t>());
    }
    return out;
}

template <class Geometry>
static bool same(const Geometry& g, const float (&model)[9], const Expected& e) {
    return g.hypothesis == e.hypothesis && std::memcmp(model, e.model, sizeof e.model) == 0 &&
           g.inliers.size() == e.list.size() &&
           (e.list.empty() || std::memcmp(g.inliers.data(), e.list.data(), sizeof(sift_cuda::DMatch) * e.list.size()) == 0);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    static_assert(sizeof(sift_cuda::DMatch) == 16, "the record the file holds");
    Reader in(argv[1]);
    int winners[2] = {0, 0};
    for (int model = 0; model < 2; model++) {
        const Batch b(in);
        const std::vector<Expected> want = expected(argv[2 + model], b.P);
        std::vector<Device*> keep;
        std::vector<sift_cuda::VerifyPair> pairs;
        int total = 0;
        for (int p = 0; p < b.P; p++) {
            sift_cuda::VerifyPair pr;
            if (b.cap[p] > 0) {  // an empty pair keeps null positions
                keep.push_back(new Device(b.q[p].data(), sizeof(float) * b.q[p].size()));
                pr.query_xy = static_cast<const float*>(keep.back()->p);
                keep.push_back(new Device(b.t[p].data(), sizeof(float) * b.t[p].size()));
                pr.train_xy = static_cast<const float*>(keep.back()->p);
                pr.nq = b.nq[p], pr.nt = b.nt[p];
            }
            pr.cap = b.cap[p];
            pairs.push_back(pr);
            total += b.cap[p];
        }
        const Device dm(b.rows.data(), sizeof(sift_cuda::DMatch) * b.rows.size());
        const Device dc(b.count.data(), sizeof(int) * b.count.size());
        const sift_cuda::DMatch* rows = static_cast<const sift_cuda::DMatch*>(dm.p);
        const int* counts = static_cast<const int*>(dc.p);
        sift_cuda::VerifyParams params;
        params.hypotheses = b.K, params.seed = b.seed, params.max_error = b.max_error;
        sift_cuda::Verifier v(total, b.K, -1, b.P);
        if (model == 0) {
            const std::vector<sift_cuda::TwoViewGeometry> g = v.verifyBatchedHost(rows, counts, pairs, 2, 2, params);
            REQUIRE((int)g.size() == b.P);
            for (int p = 0; p < b.P; p++) {
                REQUIRE(same(g[(size_t)p], g[(size_t)p].F, want[(size_t)p]));
                winners[model] += g[(size_t)p].hypothesis >= 0;
            }
        } else {
            const std::vector<sift_cuda::PlanarGeometry> g = v.verifyHomographyBatchedHost(rows, counts, pairs, 2, 2, params);
            REQUIRE((int)g.size() == b.P);
            for (int p = 0; p < b.P; p++) {
                REQUIRE(same(g[(size_t)p], g[(size_t)p].H, want[(size_t)p]));
                winners[model] += g[(size_t)p].hypothesis >= 0;
            }
        }
        // the device form: the result records on the device, read back
        {
            std::vector<sift_cuda::VerifyResult> zero((size_t)b.P), got((size_t)b.P);
            std::memset(zero.data(), 0, sizeof(sift_cuda::VerifyResult) * zero.size());
            const Device dres(zero.data(), sizeof(sift_cuda::VerifyResult) * zero.size());
            if (model == 0)
                v.verifyBatchedDevice(rows, counts, pairs, 2, 2, params, static_cast<sift_cuda::VerifyResult*>(dres.p));
            else
                v.verifyHomographyBatchedDevice(rows, counts, pairs, 2, 2, params,
                                                static_cast<sift_cuda::HomographyResult*>(dres.p));
            REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
            REQUIRE(sift_hip_memcpy_d2h(got.data(), dres.p, sizeof(sift_cuda::VerifyResult) * got.size()) == SIFT_HIP_OK);
            for (int p = 0; p < b.P; p++) {
                const sift_cuda::VerifyResult& r = got[(size_t)p];
                const Expected& e = want[(size_t)p];
                REQUIRE(r.hypothesis == e.hypothesis && r.inliers == (int)e.list.size() && r.matches == b.count[p] &&
                        std::memcmp(r.F, e.model, sizeof r.F) == 0);
            }
        }
        // what the ABI refuses throws std::invalid_argument
        bool thrown = false;
        try {
            sift_cuda::Verifier one(total, b.K);  // max_pairs = 1
            (void)one.verifyBatchedHost(rows, counts, pairs, 2, 2, params);
        } catch (const std::invalid_argument&) {
            thrown = true;
        }
        REQUIRE(thrown);
        for (Device* d : keep) delete d;
    }
    REQUIRE(winners[0] >= 5 && winners[1] >= 5);
    std::printf("verify batched ok: %d + %d pairs with a winner\n", winners[0], winners[1]);
    return 0;
}
