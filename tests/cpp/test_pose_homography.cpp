// The plane pose forms of sift_cuda::Verifier and sift_cuda::recoverPoseHomography on the GPU
// (tests/test_gpu_pose_homography_cxx.py writes the inputs and the bytes the Python surface returns; see there for the
// files).
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

template <class T>
static std::vector<T> download(const T* p, size_t n) {
    std::vector<T> v(n);
    if (n) (void)sift_hip_memcpy_d2h(v.data(), p, n * sizeof(T));
    return v;
}

struct Pair {
    int n, nq, nt;
    std::vector<sift_cuda::DMatch> matches;
    std::vector<float> q_xy, t_xy;
    sift_cuda::HomographyResult result;
    std::vector<uint8_t> mask;
    sift_cuda::Camera cq, ct;
};

static Pair read_pair(Reader& in) {
    Pair p;
    p.n = in.get<int>(), p.nq = in.get<int>(), p.nt = in.get<int>();
    p.matches = in.many<sift_cuda::DMatch>((size_t)p.n);
    p.q_xy = in.many<float>(2 * (size_t)p.nq), p.t_xy = in.many<float>(2 * (size_t)p.nt);
    p.result = in.get<sift_cuda::HomographyResult>();
    p.mask = in.many<uint8_t>((size_t)p.n);
    p.cq = in.get<sift_cuda::Camera>(), p.ct = in.get<sift_cuda::Camera>();
    return p;
}

// The bytes the Python surface wrote for a pair: record, candidates, mask, points, count, records.
static bool equals(const sift_cuda::PlanePose& got, Reader& want, int n) {
    const auto pose = want.get<sift_cuda::PlanePoseResult>();
    const auto cands = want.many<sift_cuda::PlaneCandidate>(4);
    if (std::memcmp(got.candidates, cands.data(), 4 * sizeof(sift_cuda::PlaneCandidate)) != 0) return false;
    const auto mask = want.many<uint8_t>((size_t)n);
    const auto points = want.many<float>(3 * (size_t)n);
    const int k = want.get<int>();
    const auto recs = want.many<sift_cuda::DMatch>((size_t)k);
    return std::memcmp(&got.pose, &pose, sizeof pose) == 0 && got.mask == mask && (int)got.inliers.size() == k &&
           got.points.size() == points.size() &&
           (points.empty() || std::memcmp(got.points.data(), points.data(), points.size() * sizeof(float)) == 0) &&
           (k == 0 || std::memcmp(got.inliers.data(), recs.data(), (size_t)k * sizeof(sift_cuda::DMatch)) == 0);
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    const std::vector<char> given = slurp(argv[1]), expected = slurp(argv[2]);
    Reader in{given};
    const int P = in.get<int>();
    std::vector<Pair> pairs;
    for (int p = 0; p < P; p++) pairs.push_back(read_pair(in));
    REQUIRE(in.at == given.size() && P >= 2);

    // Pair by pair: the host form, the all-in-one, and the device form on device memory.
    Reader want{expected};
    for (const Pair& p : pairs) {
        const sift_cuda::DMatch* dm = upload(p.matches);
        const float *dq = upload(p.q_xy), *dt = upload(p.t_xy);
        sift_cuda::Verifier v(p.n, 1);
        const size_t at = want.at;
        REQUIRE(equals(v.recoverPoseHomographyHost(dm, nullptr, p.n, dq, 2, p.nq, dt, 2, p.nt, p.result, p.mask, p.cq, p.ct), want, p.n));
        want.at = at;
        if (p.result.hypothesis >= 0) {  // the all-in-one takes H alone: its record is never the empty one
            REQUIRE(equals(sift_cuda::recoverPoseHomography(p.matches, dq, p.nq, dt, p.nt, p.result.H, p.mask, p.cq, p.ct, {}, 2,
                                                            2),
                           want, p.n));
            want.at = at;
        }
        const auto* dres = upload(std::vector<sift_cuda::HomographyResult>{p.result});
        uint8_t* dmask = upload(p.mask);
        auto* dpose = upload(std::vector<sift_cuda::PlanePoseResult>(1));
        auto* dcands = upload(std::vector<sift_cuda::PlaneCandidate>(4));
        float* dpoints = upload(std::vector<float>(3 * (size_t)p.n));
        auto* dout = upload(std::vector<sift_cuda::DMatch>((size_t)p.n));
        int* dcount = upload(std::vector<int>(1));
        v.recoverPoseHomographyDevice(dm, nullptr, p.n, dq, 2, p.nq, dt, 2, p.nt, dres, dmask, p.cq, p.ct, {}, dpose, dmask,
                                      dpoints, dout, dcount, dcands);  // mask_out is the mask
        REQUIRE(sift_hip_device_sync() == SIFT_HIP_OK);
        sift_cuda::PlanePose got;
        got.pose = download(dpose, 1)[0];
        std::memcpy(got.candidates, download(dcands, 4).data(), sizeof got.candidates);
        got.mask = download(dmask, (size_t)p.n);
        got.points = download(dpoints, 3 * (size_t)p.n);
        got.inliers = download(dout, (size_t)download(dcount, 1)[0]);
        REQUIRE(equals(got, want, p.n));
        for (const void* d : {(const void*)dm, (const void*)dq, (const void*)dt, (const void*)dres, (const void*)dmask,
                              (const void*)dpose, (const void*)dcands, (const void*)dpoints, (const void*)dout, (const void*)dcount})
            (void)sift_hip_free(const_cast<void*>(d));
    }
    REQUIRE(want.at == expected.size());

    // All pairs in one batched call, host form.
    std::vector<sift_cuda::DMatch> all;
    std::vector<uint8_t> mask;
    std::vector<sift_cuda::VerifyPair> table;
    std::vector<sift_cuda::HomographyResult> results;
    std::vector<sift_cuda::Camera> cq, ct;
    std::vector<const float*> held;
    for (const Pair& p : pairs) {
        all.insert(all.end(), p.matches.begin(), p.matches.end());
        mask.insert(mask.end(), p.mask.begin(), p.mask.end());
        const float *dq = upload(p.q_xy), *dt = upload(p.t_xy);
        held.push_back(dq), held.push_back(dt);
        table.push_back({dq, dt, p.nq, p.nt, p.n});
        results.push_back(p.result), cq.push_back(p.cq), ct.push_back(p.ct);
    }
    const sift_cuda::DMatch* dall = upload(all);
    sift_cuda::Verifier vb((int)all.size(), 1, -1, P);
    const auto got = vb.recoverPoseHomographyBatchedHost(dall, nullptr, table, 2, 2, results, mask, cq, ct);
    REQUIRE((int)got.size() == P);
    Reader again{expected};
    for (int p = 0; p < P; p++) REQUIRE(equals(got[(size_t)p], again, pairs[(size_t)p].n));
    for (const float* d : held) (void)sift_hip_free(const_cast<float*>(d));
    (void)sift_hip_free(const_cast<sift_cuda::DMatch*>(dall));
    std::printf("pose homography cxx ok\n");
    return 0;
}
