// sift_cuda::Verifier / verifyFundamental / verifyHomography / verifyAffine / projectHomographyDevice
// (include/sift_cuda/Verify.hh) over the
// C ABI in include/sift_hip.h.  Plain C++ (g++): no HIP headers, no device code.
#include "sift_cuda/Verify.hh"

#include <cstddef>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

#include "sift_hip.h"

namespace sift_cuda {

namespace {

static_assert(sizeof(VerifyResult) == sizeof(sift_hip_verify_result) &&
                  offsetof(VerifyResult, hypothesis) == offsetof(sift_hip_verify_result, hypothesis),
              "sift_cuda::VerifyResult is sift_hip_verify_result");
static_assert(sizeof(HomographyResult) == sizeof(sift_hip_homography_result) &&
                  offsetof(HomographyResult, hypothesis) == offsetof(sift_hip_homography_result, hypothesis),
              "sift_cuda::HomographyResult is sift_hip_homography_result");

static_assert(sizeof(VerifyPair) == sizeof(sift_hip_verify_pair) &&
                  offsetof(VerifyPair, train_xy) == offsetof(sift_hip_verify_pair, train_xy) &&
                  offsetof(VerifyPair, nq) == offsetof(sift_hip_verify_pair, nq) &&
                  offsetof(VerifyPair, nt) == offsetof(sift_hip_verify_pair, nt) &&
                  offsetof(VerifyPair, cap) == offsetof(sift_hip_verify_pair, cap),
              "sift_cuda::VerifyPair is sift_hip_verify_pair");

static_assert(sizeof(PoseResult) == sizeof(sift_hip_pose_result) &&
                  offsetof(PoseResult, counts) == offsetof(sift_hip_pose_result, counts) &&
                  offsetof(PoseResult, candidate) == offsetof(sift_hip_pose_result, candidate),
              "sift_cuda::PoseResult is sift_hip_pose_result");
static_assert(sizeof(PlanePoseResult) == sizeof(sift_hip_plane_pose_result) &&
                  offsetof(PlanePoseResult, candidate) == offsetof(sift_hip_plane_pose_result, candidate) &&
                  offsetof(PlanePoseResult, normal) == offsetof(sift_hip_plane_pose_result, normal) &&
                  offsetof(PlanePoseResult, distance) == offsetof(sift_hip_plane_pose_result, distance),
              "sift_cuda::PlanePoseResult is sift_hip_plane_pose_result");
static_assert(sizeof(PlaneCandidate) == sizeof(sift_hip_plane_candidate) &&
                  offsetof(PlaneCandidate, normal) == offsetof(sift_hip_plane_candidate, normal) &&
                  offsetof(PlaneCandidate, distance) == offsetof(sift_hip_plane_candidate, distance),
              "sift_cuda::PlaneCandidate is sift_hip_plane_candidate");
static_assert(sizeof(Camera) == sizeof(sift_hip_camera) && offsetof(Camera, cx) == offsetof(sift_hip_camera, cx),
              "sift_cuda::Camera is sift_hip_camera");

void check_throw(int rc, const char* what) {
    if (rc == SIFT_HIP_OK) return;
    const std::string msg = std::string(what) + ": " + sift_hip_last_error() + " (status " + std::to_string(rc) + ")";
    if (rc == SIFT_HIP_ERR_INVALID) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}

sift_hip_verify_params toAbi(const VerifyParams& p) { return sift_hip_verify_params{p.hypotheses, p.seed, p.max_error}; }

// A device allocation freed on every path out.
struct DeviceBlock {
    void* p = nullptr;
    explicit DeviceBlock(size_t bytes) { check_throw(sift_hip_malloc(&p, bytes ? bytes : 1), "device allocation"); }
    ~DeviceBlock() { (void)sift_hip_free(p); }
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
};

const sift_hip_verify_pair* toAbi(const std::vector<VerifyPair>& pairs) {
    return reinterpret_cast<const sift_hip_verify_pair*>(pairs.data());
}
sift_hip_dmatch* abi(DMatch* p) { return reinterpret_cast<sift_hip_dmatch*>(p); }
const sift_hip_dmatch* abi(const DMatch* p) { return reinterpret_cast<const sift_hip_dmatch*>(p); }

// The rows of a batch (0 for caps the ABI refuses: the call throws before anything is read).
size_t batchRows(const std::vector<VerifyPair>& pairs) {
    size_t rows = 0;
    for (const VerifyPair& p : pairs)
        if (p.cap < 0 || p.cap > 65536) return 0;
        else rows += (size_t)p.cap;
    return rows;
}

// The host forms' mask: one byte per row, or the ABI's refusal of the rows themselves (nothing is read then).
void check_mask(const std::vector<uint8_t>& mask, size_t rows, const char* what) {
    if (mask.size() != rows) throw std::invalid_argument(std::string(what) + ": mask must hold one byte per row");
}

// The list a call works on as the methods take it -- one pair's, or a batch's -- and the ABI call that spreads it into
// the leading arguments of an entry point.
struct OnePair {
    const DMatch* matches;
    const int* count;
    int cap;
    const float* query_xy;
    int query_stride, nq;
    const float* train_xy;
    int train_stride, nt;
};
struct Batch {
    const DMatch* matches;
    const int* counts;
    const std::vector<VerifyPair>& pairs;
    int query_stride, train_stride;
};
template <class Fn, class... Rest>
int abiCall(Fn fn, sift_hip_verifier* h, const OnePair& l, Rest... rest) {
    return fn(h, abi(l.matches), l.count, l.cap, l.query_xy, l.query_stride, l.nq, l.train_xy, l.train_stride, l.nt, rest...);
}
template <class Fn, class... Rest>
int abiCall(Fn fn, sift_hip_verifier* h, const Batch& l, Rest... rest) {
    return fn(h, abi(l.matches), l.counts, (int)l.pairs.size(), toAbi(l.pairs), l.query_stride, l.train_stride, rest...);
}

// A model: its ABI record, the C++ record and geometry that mirror it, the matrix member they share, its entry points
// by list type, and the names its host methods throw under.
#define SIFT_MODEL(Name, name, Cxx, RECORD, RESULT, GEOMETRY, M)                                         \
    struct Name {                                                                                        \
        using Record = RECORD;                                                                           \
        using Result = RESULT;                                                                           \
        using Geometry = GEOMETRY;                                                                       \
        static constexpr const char* verifyHostName = "Verifier::verify" #Cxx "Host";                    \
        static constexpr const char* refineHostName = "Verifier::refine" #Cxx "Host";                    \
        static const float (&matrix(const Record& r))[9] { return r.M; }                                 \
        static float (&matrix(Geometry& g))[9] { return g.M; }                                           \
        static auto verifyDevice(const OnePair&) { return sift_hip_verify_##name##_device; }             \
        static auto verifyDevice(const Batch&) { return sift_hip_verify_##name##_batched_device; }       \
        static auto verifyHost(const OnePair&) { return sift_hip_verify_##name##_host; }                 \
        static auto verifyHost(const Batch&) { return sift_hip_verify_##name##_batched_host; }           \
        static auto refineDevice(const OnePair&) { return sift_hip_refine_##name##_device; }             \
        static auto refineDevice(const Batch&) { return sift_hip_refine_##name##_batched_device; }       \
        static auto refineHost(const OnePair&) { return sift_hip_refine_##name##_host; }                 \
        static auto refineHost(const Batch&) { return sift_hip_refine_##name##_batched_host; }           \
    };
SIFT_MODEL(Fundamental, fundamental, , sift_hip_verify_result, VerifyResult, TwoViewGeometry, F)
SIFT_MODEL(Planar, homography, Homography, sift_hip_homography_result, HomographyResult, PlanarGeometry, H)
#undef SIFT_MODEL

// The affine models: one set of entry points that carry the model behind the handle.  Bound to it here, they have the
// other models' shape, and the method templates below serve them as they are.
template <int MODEL, class Fn>
auto bound(Fn fn) {
    return [fn](sift_hip_verifier* h, auto... rest) { return fn(h, MODEL, rest...); };
}
template <int MODEL>
struct AffineMap {
    using Record = sift_hip_affine_result;
    using Result = AffineResult;
    using Geometry = PlanarGeometry;
    static constexpr const char* verifyHostName = "Verifier::verifyAffineHost";
    static constexpr const char* refineHostName = "Verifier::refineAffineHost";
    static const float (&matrix(const Record& r))[9] { return r.H; }
    static float (&matrix(Geometry& g))[9] { return g.H; }
    static auto verifyDevice(const OnePair&) { return bound<MODEL>(sift_hip_verify_affine_device); }
    static auto verifyDevice(const Batch&) { return bound<MODEL>(sift_hip_verify_affine_batched_device); }
    static auto verifyHost(const OnePair&) { return bound<MODEL>(sift_hip_verify_affine_host); }
    static auto verifyHost(const Batch&) { return bound<MODEL>(sift_hip_verify_affine_batched_host); }
    static auto refineDevice(const OnePair&) { return bound<MODEL>(sift_hip_refine_affine_device); }
    static auto refineDevice(const Batch&) { return bound<MODEL>(sift_hip_refine_affine_batched_device); }
    static auto refineHost(const OnePair&) { return bound<MODEL>(sift_hip_refine_affine_host); }
    static auto refineHost(const Batch&) { return bound<MODEL>(sift_hip_refine_affine_batched_host); }
};
// f(the model's struct) for the model an affine method was given.
template <class F>
auto byModel(AffineModel model, const char* what, F f) {
    if (model == AffineModel::Similarity) return f(AffineMap<SIFT_HIP_MODEL_SIMILARITY>{});
    if (model != AffineModel::Affine) throw std::invalid_argument(std::string(what) + ": model must be Affine or Similarity");
    return f(AffineMap<SIFT_HIP_MODEL_AFFINE>{});
}

template <class M>
typename M::Record* abi(typename M::Result* r) {
    return reinterpret_cast<typename M::Record*>(r);
}

// The geometry of a record and its inlier records.
template <class M>
typename M::Geometry geometry(const typename M::Record& r, std::vector<DMatch> inliers) {
    typename M::Geometry g;
    for (int i = 0; i < 9; i++) M::matrix(g)[i] = M::matrix(r)[i];
    g.hypothesis = r.hypothesis;
    g.inliers = std::move(inliers);
    return g;
}

// The method shapes, one template each over the model (and, for the device forms, the list).
template <class M, class List>
void verifyDeviceT(sift_hip_verifier* h, const char* what, const List& l, const VerifyParams& params,
                   typename M::Result* result, DMatch* out, int* out_count, uint8_t* mask, void* stream) {
    const sift_hip_verify_params p = toAbi(params);
    check_throw(abiCall(M::verifyDevice(l), h, l, &p, abi<M>(result), abi(out), out_count, mask, stream), what);
}

template <class M>
typename M::Geometry verifyHostT(sift_hip_verifier* h, const char* what, const OnePair& l, const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    typename M::Record r{};
    std::vector<DMatch> list(l.cap > 0 ? (size_t)l.cap : 0);
    check_throw(abiCall(M::verifyHost(l), h, l, &p, &r, abi(list.data()), nullptr), what);
    list.resize((size_t)r.inliers);
    return geometry<M>(r, std::move(list));
}

// One geometry per pair from the host form's outputs: pair p's records are the first r[p].inliers of its rows.
template <class M>
std::vector<typename M::Geometry> verifyBatchedHostT(sift_hip_verifier* h, const char* what, const Batch& l,
                                                     const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    std::vector<typename M::Record> r(l.pairs.size());
    std::vector<DMatch> list(batchRows(l.pairs));
    check_throw(abiCall(M::verifyHost(l), h, l, &p, r.data(), abi(list.data()), nullptr), what);
    std::vector<typename M::Geometry> out(l.pairs.size());
    size_t row0 = 0;
    for (size_t i = 0; i < l.pairs.size(); i++) {
        out[i] = geometry<M>(r[i], {list.begin() + row0, list.begin() + row0 + (size_t)r[i].inliers});
        row0 += (size_t)l.pairs[i].cap;
    }
    return out;
}

template <class M, class List>
void refineDeviceT(sift_hip_verifier* h, const char* what, const List& l, float max_error, int rounds,
                   typename M::Result* result, uint8_t* mask, DMatch* out, int* out_count, int* accepted, void* stream) {
    check_throw(abiCall(M::refineDevice(l), h, l, max_error, rounds, abi<M>(result), mask, abi(out), out_count, accepted,
                        stream),
                what);
}

template <class M>
int refineHostT(sift_hip_verifier* h, const char* what, const OnePair& l, float max_error, int rounds,
                typename M::Result& result, std::vector<uint8_t>& mask, std::vector<DMatch>* inliers) {
    if (l.cap >= 0 && l.cap <= 65536) check_mask(mask, (size_t)l.cap, what);
    std::vector<DMatch> list(inliers && l.cap > 0 && l.cap <= 65536 ? (size_t)l.cap : 0);
    int n = 0, accepted = 0;
    check_throw(abiCall(M::refineHost(l), h, l, max_error, rounds, abi<M>(&result), mask.empty() ? nullptr : mask.data(),
                        inliers ? abi(list.data()) : nullptr, &n, &accepted),
                what);
    if (inliers) {
        list.resize((size_t)n);
        *inliers = std::move(list);
    }
    return accepted;
}

template <class M>
std::vector<int> refineBatchedHostT(sift_hip_verifier* h, const char* what, const Batch& l, float max_error, int rounds,
                                    std::vector<typename M::Result>& results, std::vector<uint8_t>& mask,
                                    std::vector<DMatch>* out, std::vector<int>* out_counts) {
    if (results.size() != l.pairs.size()) throw std::invalid_argument(std::string(what) + ": one result record per pair");
    const size_t rows = batchRows(l.pairs);
    if (rows > 0) check_mask(mask, rows, what);
    std::vector<DMatch> list(out ? rows : 0);
    std::vector<int> n(l.pairs.size()), accepted(l.pairs.size());
    check_throw(abiCall(M::refineHost(l), h, l, max_error, rounds, abi<M>(results.data()),
                        mask.empty() ? nullptr : mask.data(), out ? abi(list.data()) : nullptr, n.data(), accepted.data()),
                what);
    if (out) *out = std::move(list);
    if (out_counts) *out_counts = n;
    return accepted;
}

const sift_hip_camera* abi(const Camera* c) { return reinterpret_cast<const sift_hip_camera*>(c); }
sift_hip_pose_params toAbi(const PoseParams& p) { return sift_hip_pose_params{p.max_depth, p.max_cos_parallax}; }
auto poseDevice(const OnePair&) { return sift_hip_recover_pose_device; }
auto poseDevice(const Batch&) { return sift_hip_recover_pose_batched_device; }
auto poseHost(const OnePair&) { return sift_hip_recover_pose_host; }
auto poseHost(const Batch&) { return sift_hip_recover_pose_batched_host; }

// The pose calls' host form over either list: `rows` rows of mask, points and records, `P` records.
template <class List>
std::vector<RelativePose> recoverPoseHostT(sift_hip_verifier* h, const char* what, const List& l, size_t rows,
                                           const std::vector<size_t>& caps, const sift_hip_verify_result* results,
                                           const std::vector<uint8_t>& mask, const Camera* cq, const Camera* ct,
                                           const PoseParams& params) {
    const sift_hip_pose_params p = toAbi(params);
    const size_t P = caps.size();
    std::vector<sift_hip_pose_result> poses(P ? P : 1);
    std::vector<uint8_t> front(rows);
    std::vector<float> points(3 * rows, std::numeric_limits<float>::quiet_NaN());
    std::vector<DMatch> list(rows);
    std::vector<int> n(P ? P : 1);
    check_throw(abiCall(poseHost(l), h, l, results, mask.empty() ? nullptr : mask.data(), abi(cq), abi(ct), &p,
                        poses.data(), front.data(), points.data(), abi(list.data()), n.data()),
                what);
    std::vector<RelativePose> out(P);
    size_t row0 = 0;
    for (size_t i = 0; i < P; i++) {
        static_assert(sizeof(PoseResult) == sizeof(sift_hip_pose_result), "copied as bytes");
        std::memcpy(&out[i].pose, &poses[i], sizeof(PoseResult));
        out[i].mask.assign(front.begin() + row0, front.begin() + row0 + caps[i]);
        out[i].points.assign(points.begin() + 3 * row0, points.begin() + 3 * (row0 + caps[i]));
        out[i].inliers.assign(list.begin() + row0, list.begin() + row0 + (size_t)n[i]);
        row0 += caps[i];
    }
    return out;
}

auto planePoseDevice(const OnePair&) { return sift_hip_recover_pose_homography_device; }
auto planePoseDevice(const Batch&) { return sift_hip_recover_pose_homography_batched_device; }
auto planePoseHost(const OnePair&) { return sift_hip_recover_pose_homography_host; }
auto planePoseHost(const Batch&) { return sift_hip_recover_pose_homography_batched_host; }

// The plane pose calls' host form over either list, as recoverPoseHostT.
template <class List>
std::vector<PlanePose> recoverPlanePoseHostT(sift_hip_verifier* h, const char* what, const List& l, size_t rows,
                                             const std::vector<size_t>& caps, const sift_hip_homography_result* results,
                                             const std::vector<uint8_t>& mask, const Camera* cq, const Camera* ct,
                                             const PoseParams& params) {
    const sift_hip_pose_params p = toAbi(params);
    const size_t P = caps.size();
    std::vector<sift_hip_plane_pose_result> poses(P ? P : 1);
    std::vector<sift_hip_plane_candidate> cands(4 * (P ? P : 1));
    std::vector<uint8_t> front(rows);
    std::vector<float> points(3 * rows, std::numeric_limits<float>::quiet_NaN());
    std::vector<DMatch> list(rows);
    std::vector<int> n(P ? P : 1);
    check_throw(abiCall(planePoseHost(l), h, l, results, mask.empty() ? nullptr : mask.data(), abi(cq), abi(ct), &p,
                        poses.data(), front.data(), points.data(), abi(list.data()), n.data(), cands.data()),
                what);
    std::vector<PlanePose> out(P);
    size_t row0 = 0;
    for (size_t i = 0; i < P; i++) {
        std::memcpy(&out[i].pose, &poses[i], sizeof(PlanePoseResult));
        std::memcpy(out[i].candidates, &cands[4 * i], 4 * sizeof(PlaneCandidate));
        out[i].mask.assign(front.begin() + row0, front.begin() + row0 + caps[i]);
        out[i].points.assign(points.begin() + 3 * row0, points.begin() + 3 * (row0 + caps[i]));
        out[i].inliers.assign(list.begin() + row0, list.begin() + row0 + (size_t)n[i]);
        row0 += caps[i];
    }
    return out;
}

// The convenience call on a host list: a verifier sized to it (the argument rules come first, they need no device
// memory), the list uploaded, the host form, and with refit > 0 that many refit rounds on its record and mask.
template <class M>
typename M::Geometry verifyT(const char* what, const std::vector<DMatch>& matches, const OnePair& positions,
                             const VerifyParams& params, int refit) {
    const int n = (int)matches.size();
    Verifier v(n > 0 ? n : 1, params.hypotheses > 0 && params.hypotheses <= 4096 ? params.hypotheses : 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), what);
    OnePair l = positions;
    l.matches = static_cast<const DMatch*>(d.p), l.count = nullptr, l.cap = n;
    if (refit == 0) return verifyHostT<M>(v.handle(), M::verifyHostName, l, params);
    const sift_hip_verify_params p = toAbi(params);
    typename M::Result r{};
    std::vector<uint8_t> mask(matches.size());
    check_throw(abiCall(M::verifyHost(l), v.handle(), l, &p, abi<M>(&r), nullptr, mask.empty() ? nullptr : mask.data()),
                what);
    std::vector<DMatch> inliers;
    refineHostT<M>(v.handle(), M::refineHostName, l, params.max_error, refit, r, mask, &inliers);
    return geometry<M>(*abi<M>(&r), std::move(inliers));
}

}  // namespace

Verifier::Verifier(int max_matches, int max_hypotheses, int device, int max_pairs) {
    check_throw(sift_hip_verifier_create_batched(device, max_matches, max_hypotheses, max_pairs, &m_handle),
                "Verifier::Verifier");
}

Verifier::Verifier(int max_matches, int max_hypotheses, int device) {
    check_throw(sift_hip_verifier_create(device, max_matches, max_hypotheses, &m_handle), "Verifier::Verifier");
}

Verifier::~Verifier() { (void)sift_hip_verifier_destroy(m_handle); }

// The methods: each names its model, its list and itself.
#define ONE_PAIR_ARGS                                                                                                  \
    const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,                \
        const float* train_xy, int train_stride, int nt
#define ONE_PAIR OnePair{matches, count, cap, query_xy, query_stride, nq, train_xy, train_stride, nt}
#define BATCH_ARGS \
    const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs, int query_stride, int train_stride
#define BATCH Batch{matches, counts, pairs, query_stride, train_stride}

#define SIFT_VERIFIER_METHODS(Model, Cxx)                                                                              \
    void Verifier::verify##Cxx##Device(ONE_PAIR_ARGS, const VerifyParams& params, Model::Result* result, DMatch* out,  \
                                       int* out_count, uint8_t* mask, void* stream) {                                  \
        verifyDeviceT<Model>(m_handle, "Verifier::verify" #Cxx "Device", ONE_PAIR, params, result, out, out_count,     \
                             mask, stream);                                                                            \
    }                                                                                                                  \
    void Verifier::verify##Cxx##BatchedDevice(BATCH_ARGS, const VerifyParams& params, Model::Result* results,          \
                                              DMatch* out, int* out_counts, uint8_t* mask, void* stream) {             \
        verifyDeviceT<Model>(m_handle, "Verifier::verify" #Cxx "BatchedDevice", BATCH, params, results, out,           \
                             out_counts, mask, stream);                                                                \
    }                                                                                                                  \
    Model::Geometry Verifier::verify##Cxx##Host(ONE_PAIR_ARGS, const VerifyParams& params) {                           \
        return verifyHostT<Model>(m_handle, Model::verifyHostName, ONE_PAIR, params);                                  \
    }                                                                                                                  \
    std::vector<Model::Geometry> Verifier::verify##Cxx##BatchedHost(BATCH_ARGS, const VerifyParams& params) {          \
        return verifyBatchedHostT<Model>(m_handle, "Verifier::verify" #Cxx "BatchedHost", BATCH, params);              \
    }                                                                                                                  \
    void Verifier::refine##Cxx##Device(ONE_PAIR_ARGS, float max_error, int rounds, Model::Result* result,              \
                                       uint8_t* mask, DMatch* out, int* out_count, int* accepted, void* stream) {      \
        refineDeviceT<Model>(m_handle, "Verifier::refine" #Cxx "Device", ONE_PAIR, max_error, rounds, result, mask,    \
                             out, out_count, accepted, stream);                                                        \
    }                                                                                                                  \
    void Verifier::refine##Cxx##BatchedDevice(BATCH_ARGS, float max_error, int rounds, Model::Result* results,         \
                                              uint8_t* mask, DMatch* out, int* out_counts, int* accepted,              \
                                              void* stream) {                                                          \
        refineDeviceT<Model>(m_handle, "Verifier::refine" #Cxx "BatchedDevice", BATCH, max_error, rounds, results,     \
                             mask, out, out_counts, accepted, stream);                                                 \
    }                                                                                                                  \
    int Verifier::refine##Cxx##Host(ONE_PAIR_ARGS, float max_error, int rounds, Model::Result& result,                 \
                                    std::vector<uint8_t>& mask, std::vector<DMatch>* inliers) {                        \
        return refineHostT<Model>(m_handle, Model::refineHostName, ONE_PAIR, max_error, rounds, result, mask, inliers); \
    }                                                                                                                  \
    std::vector<int> Verifier::refine##Cxx##BatchedHost(BATCH_ARGS, float max_error, int rounds,                       \
                                                        std::vector<Model::Result>& results,                           \
                                                        std::vector<uint8_t>& mask, std::vector<DMatch>* out,          \
                                                        std::vector<int>* out_counts) {                                \
        return refineBatchedHostT<Model>(m_handle, "Verifier::refine" #Cxx "BatchedHost", BATCH, max_error, rounds,    \
                                         results, mask, out, out_counts);                                              \
    }
SIFT_VERIFIER_METHODS(Fundamental, )
SIFT_VERIFIER_METHODS(Planar, Homography)
#undef SIFT_VERIFIER_METHODS

// The affine methods: the same shapes, the model chosen at run time.
void Verifier::verifyAffineDevice(ONE_PAIR_ARGS, AffineModel model, const VerifyParams& params, AffineResult* result,
                                  DMatch* out, int* out_count, uint8_t* mask, void* stream) {
    const char* what = "Verifier::verifyAffineDevice";
    byModel(model, what, [&](auto m) {
        verifyDeviceT<decltype(m)>(m_handle, what, ONE_PAIR, params, result, out, out_count, mask, stream);
    });
}
void Verifier::verifyAffineBatchedDevice(BATCH_ARGS, AffineModel model, const VerifyParams& params, AffineResult* results,
                                         DMatch* out, int* out_counts, uint8_t* mask, void* stream) {
    const char* what = "Verifier::verifyAffineBatchedDevice";
    byModel(model, what, [&](auto m) {
        verifyDeviceT<decltype(m)>(m_handle, what, BATCH, params, results, out, out_counts, mask, stream);
    });
}
PlanarGeometry Verifier::verifyAffineHost(ONE_PAIR_ARGS, AffineModel model, const VerifyParams& params) {
    const char* what = "Verifier::verifyAffineHost";
    return byModel(model, what, [&](auto m) { return verifyHostT<decltype(m)>(m_handle, what, ONE_PAIR, params); });
}
std::vector<PlanarGeometry> Verifier::verifyAffineBatchedHost(BATCH_ARGS, AffineModel model, const VerifyParams& params) {
    const char* what = "Verifier::verifyAffineBatchedHost";
    return byModel(model, what, [&](auto m) { return verifyBatchedHostT<decltype(m)>(m_handle, what, BATCH, params); });
}
void Verifier::refineAffineDevice(ONE_PAIR_ARGS, AffineModel model, float max_error, int rounds, AffineResult* result,
                                  uint8_t* mask, DMatch* out, int* out_count, int* accepted, void* stream) {
    const char* what = "Verifier::refineAffineDevice";
    byModel(model, what, [&](auto m) {
        refineDeviceT<decltype(m)>(m_handle, what, ONE_PAIR, max_error, rounds, result, mask, out, out_count, accepted,
                                   stream);
    });
}
void Verifier::refineAffineBatchedDevice(BATCH_ARGS, AffineModel model, float max_error, int rounds, AffineResult* results,
                                         uint8_t* mask, DMatch* out, int* out_counts, int* accepted, void* stream) {
    const char* what = "Verifier::refineAffineBatchedDevice";
    byModel(model, what, [&](auto m) {
        refineDeviceT<decltype(m)>(m_handle, what, BATCH, max_error, rounds, results, mask, out, out_counts, accepted,
                                   stream);
    });
}
int Verifier::refineAffineHost(ONE_PAIR_ARGS, AffineModel model, float max_error, int rounds, AffineResult& result,
                               std::vector<uint8_t>& mask, std::vector<DMatch>* inliers) {
    const char* what = "Verifier::refineAffineHost";
    return byModel(model, what, [&](auto m) {
        return refineHostT<decltype(m)>(m_handle, what, ONE_PAIR, max_error, rounds, result, mask, inliers);
    });
}
std::vector<int> Verifier::refineAffineBatchedHost(BATCH_ARGS, AffineModel model, float max_error, int rounds,
                                                   std::vector<AffineResult>& results, std::vector<uint8_t>& mask,
                                                   std::vector<DMatch>* out, std::vector<int>* out_counts) {
    const char* what = "Verifier::refineAffineBatchedHost";
    return byModel(model, what, [&](auto m) {
        return refineBatchedHostT<decltype(m)>(m_handle, what, BATCH, max_error, rounds, results, mask, out, out_counts);
    });
}

// The essential methods: the fundamental model's record and geometry, the cameras in front of the params.
void Verifier::reserveEssential(int max_samples) {
    check_throw(sift_hip_verifier_reserve_essential(m_handle, max_samples), "Verifier::reserveEssential");
}

void Verifier::verifyEssentialDevice(ONE_PAIR_ARGS, const Camera& cam_query, const Camera& cam_train,
                                     const VerifyParams& params, VerifyResult* result, DMatch* out, int* out_count,
                                     uint8_t* mask, void* stream) {
    const sift_hip_verify_params p = toAbi(params);
    check_throw(abiCall(sift_hip_verify_essential_device, m_handle, ONE_PAIR, abi(&cam_query), abi(&cam_train), &p,
                        abi<Fundamental>(result), abi(out), out_count, mask, stream),
                "Verifier::verifyEssentialDevice");
}

void Verifier::verifyEssentialBatchedDevice(BATCH_ARGS, const std::vector<Camera>& cams_query,
                                            const std::vector<Camera>& cams_train, const VerifyParams& params,
                                            VerifyResult* results, DMatch* out, int* out_counts, uint8_t* mask,
                                            void* stream) {
    if (cams_query.size() != pairs.size() || cams_train.size() != pairs.size())
        throw std::invalid_argument("Verifier::verifyEssentialBatchedDevice: one camera per pair and side");
    const sift_hip_verify_params p = toAbi(params);
    check_throw(abiCall(sift_hip_verify_essential_batched_device, m_handle, BATCH, abi(cams_query.data()),
                        abi(cams_train.data()), &p, abi<Fundamental>(results), abi(out), out_counts, mask, stream),
                "Verifier::verifyEssentialBatchedDevice");
}

TwoViewGeometry Verifier::verifyEssentialHost(ONE_PAIR_ARGS, const Camera& cam_query, const Camera& cam_train,
                                              const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    sift_hip_verify_result r{};
    std::vector<DMatch> list(cap > 0 ? (size_t)cap : 0);
    check_throw(abiCall(sift_hip_verify_essential_host, m_handle, ONE_PAIR, abi(&cam_query), abi(&cam_train), &p, &r,
                        abi(list.data()), nullptr),
                "Verifier::verifyEssentialHost");
    list.resize((size_t)r.inliers);
    return geometry<Fundamental>(r, std::move(list));
}

std::vector<TwoViewGeometry> Verifier::verifyEssentialBatchedHost(BATCH_ARGS, const std::vector<Camera>& cams_query,
                                                                  const std::vector<Camera>& cams_train,
                                                                  const VerifyParams& params) {
    const char* what = "Verifier::verifyEssentialBatchedHost";
    if (cams_query.size() != pairs.size() || cams_train.size() != pairs.size())
        throw std::invalid_argument(std::string(what) + ": one camera per pair and side");
    const sift_hip_verify_params p = toAbi(params);
    std::vector<sift_hip_verify_result> r(pairs.size());
    std::vector<DMatch> list(batchRows(pairs));
    check_throw(abiCall(sift_hip_verify_essential_batched_host, m_handle, BATCH, abi(cams_query.data()),
                        abi(cams_train.data()), &p, r.data(), abi(list.data()), nullptr),
                what);
    std::vector<TwoViewGeometry> out(pairs.size());
    size_t row0 = 0;
    for (size_t i = 0; i < pairs.size(); i++) {
        out[i] = geometry<Fundamental>(r[i], {list.begin() + row0, list.begin() + row0 + (size_t)r[i].inliers});
        row0 += (size_t)pairs[i].cap;
    }
    return out;
}

void Verifier::recoverPoseDevice(ONE_PAIR_ARGS, const VerifyResult* result, const uint8_t* mask, const Camera& cam_query,
                                 const Camera& cam_train, const PoseParams& params, PoseResult* pose, uint8_t* mask_out,
                                 float* points, DMatch* out, int* out_count, void* stream) {
    const sift_hip_pose_params p = toAbi(params);
    const OnePair l = ONE_PAIR;
    check_throw(abiCall(poseDevice(l), m_handle, l, reinterpret_cast<const sift_hip_verify_result*>(result), mask,
                        abi(&cam_query), abi(&cam_train), &p, reinterpret_cast<sift_hip_pose_result*>(pose), mask_out,
                        points, abi(out), out_count, stream),
                "Verifier::recoverPoseDevice");
}

void Verifier::recoverPoseBatchedDevice(BATCH_ARGS, const VerifyResult* results, const uint8_t* mask,
                                        const std::vector<Camera>& cams_query, const std::vector<Camera>& cams_train,
                                        const PoseParams& params, PoseResult* poses, uint8_t* mask_out, float* points,
                                        DMatch* out, int* out_counts, void* stream) {
    if (cams_query.size() != pairs.size() || cams_train.size() != pairs.size())
        throw std::invalid_argument("Verifier::recoverPoseBatchedDevice: one camera per pair and side");
    const sift_hip_pose_params p = toAbi(params);
    const Batch l = BATCH;
    check_throw(abiCall(poseDevice(l), m_handle, l, reinterpret_cast<const sift_hip_verify_result*>(results), mask,
                        abi(cams_query.data()), abi(cams_train.data()), &p, reinterpret_cast<sift_hip_pose_result*>(poses),
                        mask_out, points, abi(out), out_counts, stream),
                "Verifier::recoverPoseBatchedDevice");
}

RelativePose Verifier::recoverPoseHost(ONE_PAIR_ARGS, const VerifyResult& result, const std::vector<uint8_t>& mask,
                                       const Camera& cam_query, const Camera& cam_train, const PoseParams& params) {
    const char* what = "Verifier::recoverPoseHost";
    const bool sized = cap >= 0 && cap <= 65536;
    if (sized) check_mask(mask, (size_t)cap, what);
    const size_t rows = sized ? (size_t)cap : 0;
    return recoverPoseHostT(m_handle, what, ONE_PAIR, rows, {rows},
                            reinterpret_cast<const sift_hip_verify_result*>(&result), mask, &cam_query, &cam_train,
                            params)[0];
}

std::vector<RelativePose> Verifier::recoverPoseBatchedHost(BATCH_ARGS, const std::vector<VerifyResult>& results,
                                                           const std::vector<uint8_t>& mask,
                                                           const std::vector<Camera>& cams_query,
                                                           const std::vector<Camera>& cams_train,
                                                           const PoseParams& params) {
    const char* what = "Verifier::recoverPoseBatchedHost";
    if (results.size() != pairs.size()) throw std::invalid_argument(std::string(what) + ": one result record per pair");
    if (cams_query.size() != pairs.size() || cams_train.size() != pairs.size())
        throw std::invalid_argument(std::string(what) + ": one camera per pair and side");
    const size_t rows = batchRows(pairs);
    if (rows > 0) check_mask(mask, rows, what);
    std::vector<size_t> caps;
    for (const VerifyPair& p : pairs) caps.push_back(rows > 0 && p.cap > 0 ? (size_t)p.cap : 0);
    return recoverPoseHostT(m_handle, what, BATCH, rows, caps,
                            reinterpret_cast<const sift_hip_verify_result*>(results.data()), mask, cams_query.data(),
                            cams_train.data(), params);
}

void Verifier::recoverPoseHomographyDevice(ONE_PAIR_ARGS, const HomographyResult* result, const uint8_t* mask,
                                           const Camera& cam_query, const Camera& cam_train, const PoseParams& params,
                                           PlanePoseResult* pose, uint8_t* mask_out, float* points, DMatch* out,
                                           int* out_count, PlaneCandidate* candidates, void* stream) {
    const sift_hip_pose_params p = toAbi(params);
    const OnePair l = ONE_PAIR;
    check_throw(abiCall(planePoseDevice(l), m_handle, l, reinterpret_cast<const sift_hip_homography_result*>(result), mask,
                        abi(&cam_query), abi(&cam_train), &p, reinterpret_cast<sift_hip_plane_pose_result*>(pose),
                        mask_out, points, abi(out), out_count, reinterpret_cast<sift_hip_plane_candidate*>(candidates),
                        stream),
                "Verifier::recoverPoseHomographyDevice");
}

void Verifier::recoverPoseHomographyBatchedDevice(BATCH_ARGS, const HomographyResult* results, const uint8_t* mask,
                                                  const std::vector<Camera>& cams_query,
                                                  const std::vector<Camera>& cams_train, const PoseParams& params,
                                                  PlanePoseResult* poses, uint8_t* mask_out, float* points, DMatch* out,
                                                  int* out_counts, PlaneCandidate* candidates, void* stream) {
    if (cams_query.size() != pairs.size() || cams_train.size() != pairs.size())
        throw std::invalid_argument("Verifier::recoverPoseHomographyBatchedDevice: one camera per pair and side");
    const sift_hip_pose_params p = toAbi(params);
    const Batch l = BATCH;
    check_throw(abiCall(planePoseDevice(l), m_handle, l, reinterpret_cast<const sift_hip_homography_result*>(results),
                        mask, abi(cams_query.data()), abi(cams_train.data()), &p,
                        reinterpret_cast<sift_hip_plane_pose_result*>(poses), mask_out, points, abi(out), out_counts,
                        reinterpret_cast<sift_hip_plane_candidate*>(candidates), stream),
                "Verifier::recoverPoseHomographyBatchedDevice");
}

PlanePose Verifier::recoverPoseHomographyHost(ONE_PAIR_ARGS, const HomographyResult& result,
                                              const std::vector<uint8_t>& mask, const Camera& cam_query,
                                              const Camera& cam_train, const PoseParams& params) {
    const char* what = "Verifier::recoverPoseHomographyHost";
    const bool sized = cap >= 0 && cap <= 65536;
    if (sized) check_mask(mask, (size_t)cap, what);
    const size_t rows = sized ? (size_t)cap : 0;
    return recoverPlanePoseHostT(m_handle, what, ONE_PAIR, rows, {rows},
                                 reinterpret_cast<const sift_hip_homography_result*>(&result), mask, &cam_query,
                                 &cam_train, params)[0];
}

std::vector<PlanePose> Verifier::recoverPoseHomographyBatchedHost(BATCH_ARGS, const std::vector<HomographyResult>& results,
                                                                  const std::vector<uint8_t>& mask,
                                                                  const std::vector<Camera>& cams_query,
                                                                  const std::vector<Camera>& cams_train,
                                                                  const PoseParams& params) {
    const char* what = "Verifier::recoverPoseHomographyBatchedHost";
    if (results.size() != pairs.size()) throw std::invalid_argument(std::string(what) + ": one result record per pair");
    if (cams_query.size() != pairs.size() || cams_train.size() != pairs.size())
        throw std::invalid_argument(std::string(what) + ": one camera per pair and side");
    const size_t rows = batchRows(pairs);
    if (rows > 0) check_mask(mask, rows, what);
    std::vector<size_t> caps;
    for (const VerifyPair& p : pairs) caps.push_back(rows > 0 && p.cap > 0 ? (size_t)p.cap : 0);
    return recoverPlanePoseHostT(m_handle, what, BATCH, rows, caps,
                                 reinterpret_cast<const sift_hip_homography_result*>(results.data()), mask,
                                 cams_query.data(), cams_train.data(), params);
}
#undef BATCH
#undef BATCH_ARGS
#undef ONE_PAIR
#undef ONE_PAIR_ARGS

TwoViewGeometry verifyFundamental(const std::vector<DMatch>& matches, const float* query_xy, int nq,
                                  const float* train_xy, int nt, const VerifyParams& params, int query_stride,
                                  int train_stride, int refit) {
    return verifyT<Fundamental>("verifyFundamental", matches,
                                OnePair{nullptr, nullptr, 0, query_xy, query_stride, nq, train_xy, train_stride, nt}, params,
                                refit);
}

TwoViewGeometry verifyFundamental(const std::vector<DMatch>& matches, const float* query_xy, int nq,
                                  const float* train_xy, int nt, const VerifyParams& params, int query_stride,
                                  int train_stride) {
    return verifyFundamental(matches, query_xy, nq, train_xy, nt, params, query_stride, train_stride, 0);
}

PlanarGeometry verifyHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const VerifyParams& params, int query_stride, int train_stride, int refit) {
    return verifyT<Planar>("verifyHomography", matches,
                           OnePair{nullptr, nullptr, 0, query_xy, query_stride, nq, train_xy, train_stride, nt}, params,
                           refit);
}

PlanarGeometry verifyHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const VerifyParams& params, int query_stride, int train_stride) {
    return verifyHomography(matches, query_xy, nq, train_xy, nt, params, query_stride, train_stride, 0);
}

RelativePose recoverPose(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy, int nt,
                         const float (&F)[9], const std::vector<uint8_t>& mask, const Camera& cam_query,
                         const Camera& cam_train, const PoseParams& params, int query_stride, int train_stride) {
    const int n = (int)matches.size();
    if (!mask.empty() && mask.size() != matches.size())
        throw std::invalid_argument("recoverPose: mask must hold one byte per match, or none");
    Verifier v(n > 0 ? n : 1, 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), "recoverPose");
    VerifyResult r{};
    for (int i = 0; i < 9; i++) r.F[i] = F[i];
    r.matches = n;
    return v.recoverPoseHost(static_cast<const DMatch*>(d.p), nullptr, n, query_xy, query_stride, nq, train_xy, train_stride,
                             nt, r, mask.empty() ? std::vector<uint8_t>(matches.size(), 1) : mask, cam_query, cam_train,
                             params);
}

TwoViewGeometry verifyEssential(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const Camera& cam_query, const Camera& cam_train, const VerifyParams& params,
                                int query_stride, int train_stride, int refit) {
    const char* what = "verifyEssential";
    const int n = (int)matches.size();
    Verifier v(n > 0 ? n : 1, 1);
    v.reserveEssential(params.hypotheses);  // refuses a sample count outside 1..4096
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), what);
    const DMatch* dm = static_cast<const DMatch*>(d.p);
    if (refit == 0)
        return v.verifyEssentialHost(dm, nullptr, n, query_xy, query_stride, nq, train_xy, train_stride, nt, cam_query,
                                     cam_train, params);
    const sift_hip_verify_params p = toAbi(params);
    VerifyResult r{};
    std::vector<uint8_t> mask(matches.size());
    const OnePair l{dm, nullptr, n, query_xy, query_stride, nq, train_xy, train_stride, nt};
    check_throw(abiCall(sift_hip_verify_essential_host, v.handle(), l, abi(&cam_query), abi(&cam_train), &p,
                        abi<Fundamental>(&r), nullptr, mask.empty() ? nullptr : mask.data()),
                what);
    std::vector<DMatch> inliers;
    refineHostT<Fundamental>(v.handle(), Fundamental::refineHostName, l, params.max_error, refit, r, mask, &inliers);
    return geometry<Fundamental>(*abi<Fundamental>(&r), std::move(inliers));
}

PlanarGeometry verifyAffine(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                            int nt, AffineModel model, const VerifyParams& params, int query_stride, int train_stride,
                            int refit) {
    return byModel(model, "verifyAffine", [&](auto m) {
        return verifyT<decltype(m)>("verifyAffine", matches,
                                    OnePair{nullptr, nullptr, 0, query_xy, query_stride, nq, train_xy, train_stride, nt},
                                    params, refit);
    });
}

PlanePose recoverPoseHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const float (&H)[9], const std::vector<uint8_t>& mask, const Camera& cam_query,
                                const Camera& cam_train, const PoseParams& params, int query_stride, int train_stride) {
    const int n = (int)matches.size();
    if (!mask.empty() && mask.size() != matches.size())
        throw std::invalid_argument("recoverPoseHomography: mask must hold one byte per match, or none");
    Verifier v(n > 0 ? n : 1, 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0)
        check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), "recoverPoseHomography");
    HomographyResult r{};
    for (int i = 0; i < 9; i++) r.H[i] = H[i];
    r.matches = n;
    return v.recoverPoseHomographyHost(static_cast<const DMatch*>(d.p), nullptr, n, query_xy, query_stride, nq, train_xy,
                                       train_stride, nt, r, mask.empty() ? std::vector<uint8_t>(matches.size(), 1) : mask,
                                       cam_query, cam_train, params);
}

void projectHomographyDevice(const float* H, const float* xy, int stride, int n, float* out_xy, int out_stride,
                             void* stream) {
    check_throw(sift_hip_project_homography_device(H, xy, stride, n, out_xy, out_stride, stream),
                "projectHomographyDevice");
}

static_assert(sizeof(ProjectSet) == sizeof(sift_hip_project_set) &&
                  offsetof(ProjectSet, n) == offsetof(sift_hip_project_set, n) &&
                  offsetof(ProjectSet, out_xy) == offsetof(sift_hip_project_set, out_xy),
              "sift_cuda::ProjectSet is sift_hip_project_set");

void projectHomographyBatchedDevice(const void* geometry, int geometry_stride_bytes, const std::vector<ProjectSet>& sets,
                                    int stride, int out_stride, void* stream) {
    check_throw(sift_hip_project_homography_batched_device(geometry, geometry_stride_bytes, (int)sets.size(),
                                                           reinterpret_cast<const sift_hip_project_set*>(sets.data()),
                                                           stride, out_stride, stream),
                "projectHomographyBatchedDevice");
}

}  // namespace sift_cuda
