// sift_cuda::Verifier / verifyFundamental / verifyHomography / projectHomographyDevice
// (include/sift_cuda/Verify.hh) over the
// C ABI in include/sift_hip.h.  Plain C++ (g++): no HIP headers, no device code.
#include "sift_cuda/Verify.hh"

#include <cstddef>
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

// The rows of a batch (0 for caps the ABI refuses: the call throws before anything is read).
size_t batchRows(const std::vector<VerifyPair>& pairs) {
    size_t rows = 0;
    for (const VerifyPair& p : pairs)
        if (p.cap < 0 || p.cap > 65536) return 0;
        else rows += (size_t)p.cap;
    return rows;
}

// One geometry per pair from the host forms' outputs: pair p's records are the first r[p].inliers of its rows.
template <class Geometry, class Record>
std::vector<Geometry> geometries(const std::vector<VerifyPair>& pairs, const std::vector<Record>& r,
                                 const std::vector<DMatch>& list, float (Geometry::*model)[9],
                                 float (Record::*from)[9]) {
    std::vector<Geometry> out(pairs.size());
    size_t row0 = 0;
    for (size_t p = 0; p < pairs.size(); p++) {
        for (int i = 0; i < 9; i++) (out[p].*model)[i] = (r[p].*from)[i];
        out[p].hypothesis = r[p].hypothesis;
        out[p].inliers.assign(list.begin() + row0, list.begin() + row0 + (size_t)r[p].inliers);
        row0 += (size_t)pairs[p].cap;
    }
    return out;
}

}  // namespace

Verifier::Verifier(int max_matches, int max_hypotheses, int device, int max_pairs) {
    check_throw(sift_hip_verifier_create_batched(device, max_matches, max_hypotheses, max_pairs, &m_handle),
                "Verifier::Verifier");
}

void Verifier::verifyBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                   int query_stride, int train_stride, const VerifyParams& params, VerifyResult* results,
                                   DMatch* out, int* out_counts, uint8_t* mask, void* stream) {
    const sift_hip_verify_params p = toAbi(params);
    check_throw(sift_hip_verify_fundamental_batched_device(
                    m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), counts, (int)pairs.size(), toAbi(pairs),
                    query_stride, train_stride, &p, reinterpret_cast<sift_hip_verify_result*>(results),
                    reinterpret_cast<sift_hip_dmatch*>(out), out_counts, mask, stream),
                "Verifier::verifyBatchedDevice");
}

void Verifier::verifyHomographyBatchedDevice(const DMatch* matches, const int* counts,
                                             const std::vector<VerifyPair>& pairs, int query_stride, int train_stride,
                                             const VerifyParams& params, HomographyResult* results, DMatch* out,
                                             int* out_counts, uint8_t* mask, void* stream) {
    const sift_hip_verify_params p = toAbi(params);
    check_throw(sift_hip_verify_homography_batched_device(
                    m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), counts, (int)pairs.size(), toAbi(pairs),
                    query_stride, train_stride, &p, reinterpret_cast<sift_hip_homography_result*>(results),
                    reinterpret_cast<sift_hip_dmatch*>(out), out_counts, mask, stream),
                "Verifier::verifyHomographyBatchedDevice");
}

std::vector<TwoViewGeometry> Verifier::verifyBatchedHost(const DMatch* matches, const int* counts,
                                                         const std::vector<VerifyPair>& pairs, int query_stride,
                                                         int train_stride, const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    std::vector<sift_hip_verify_result> r(pairs.size());
    std::vector<DMatch> list(batchRows(pairs));
    check_throw(sift_hip_verify_fundamental_batched_host(
                    m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), counts, (int)pairs.size(), toAbi(pairs),
                    query_stride, train_stride, &p, r.data(), reinterpret_cast<sift_hip_dmatch*>(list.data()), nullptr),
                "Verifier::verifyBatchedHost");
    return geometries<TwoViewGeometry>(pairs, r, list, &TwoViewGeometry::F, &sift_hip_verify_result::F);
}

std::vector<PlanarGeometry> Verifier::verifyHomographyBatchedHost(const DMatch* matches, const int* counts,
                                                                  const std::vector<VerifyPair>& pairs, int query_stride,
                                                                  int train_stride, const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    std::vector<sift_hip_homography_result> r(pairs.size());
    std::vector<DMatch> list(batchRows(pairs));
    check_throw(sift_hip_verify_homography_batched_host(
                    m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), counts, (int)pairs.size(), toAbi(pairs),
                    query_stride, train_stride, &p, r.data(), reinterpret_cast<sift_hip_dmatch*>(list.data()), nullptr),
                "Verifier::verifyHomographyBatchedHost");
    return geometries<PlanarGeometry>(pairs, r, list, &PlanarGeometry::H, &sift_hip_homography_result::H);
}

Verifier::Verifier(int max_matches, int max_hypotheses, int device) {
    check_throw(sift_hip_verifier_create(device, max_matches, max_hypotheses, &m_handle), "Verifier::Verifier");
}

Verifier::~Verifier() { (void)sift_hip_verifier_destroy(m_handle); }

void Verifier::verifyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                            int nq, const float* train_xy, int train_stride, int nt, const VerifyParams& params,
                            VerifyResult* result, DMatch* out, int* out_count, uint8_t* mask, void* stream) {
    const sift_hip_verify_params p = toAbi(params);
    check_throw(sift_hip_verify_fundamental_device(
                    m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), count, cap, query_xy, query_stride, nq,
                    train_xy, train_stride, nt, &p, reinterpret_cast<sift_hip_verify_result*>(result),
                    reinterpret_cast<sift_hip_dmatch*>(out), out_count, mask, stream),
                "Verifier::verifyDevice");
}

TwoViewGeometry Verifier::verifyHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                     int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                     const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    sift_hip_verify_result r{};
    std::vector<DMatch> list(cap > 0 ? (size_t)cap : 0);
    check_throw(sift_hip_verify_fundamental_host(m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), count, cap,
                                                 query_xy, query_stride, nq, train_xy, train_stride, nt, &p, &r,
                                                 reinterpret_cast<sift_hip_dmatch*>(list.data()), nullptr),
                "Verifier::verifyHost");
    TwoViewGeometry g;
    for (int i = 0; i < 9; i++) g.F[i] = r.F[i];
    g.hypothesis = r.hypothesis;
    list.resize((size_t)r.inliers);
    g.inliers = std::move(list);
    return g;
}

void Verifier::verifyHomographyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                      int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                      const VerifyParams& params, HomographyResult* result, DMatch* out, int* out_count,
                                      uint8_t* mask, void* stream) {
    const sift_hip_verify_params p = toAbi(params);
    check_throw(sift_hip_verify_homography_device(
                    m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), count, cap, query_xy, query_stride, nq,
                    train_xy, train_stride, nt, &p, reinterpret_cast<sift_hip_homography_result*>(result),
                    reinterpret_cast<sift_hip_dmatch*>(out), out_count, mask, stream),
                "Verifier::verifyHomographyDevice");
}

PlanarGeometry Verifier::verifyHomographyHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                              int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                              const VerifyParams& params) {
    const sift_hip_verify_params p = toAbi(params);
    sift_hip_homography_result r{};
    std::vector<DMatch> list(cap > 0 ? (size_t)cap : 0);
    check_throw(sift_hip_verify_homography_host(m_handle, reinterpret_cast<const sift_hip_dmatch*>(matches), count, cap,
                                                query_xy, query_stride, nq, train_xy, train_stride, nt, &p, &r,
                                                reinterpret_cast<sift_hip_dmatch*>(list.data()), nullptr),
                "Verifier::verifyHomographyHost");
    PlanarGeometry g;
    for (int i = 0; i < 9; i++) g.H[i] = r.H[i];
    g.hypothesis = r.hypothesis;
    list.resize((size_t)r.inliers);
    g.inliers = std::move(list);
    return g;
}

TwoViewGeometry verifyFundamental(const std::vector<DMatch>& matches, const float* query_xy, int nq,
                                  const float* train_xy, int nt, const VerifyParams& params, int query_stride,
                                  int train_stride) {
    const int n = (int)matches.size();
    // The argument rules first (they need no device memory): a verifier sized to this call.
    Verifier v(n > 0 ? n : 1, params.hypotheses > 0 && params.hypotheses <= 4096 ? params.hypotheses : 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), "verifyFundamental");
    return v.verifyHost(static_cast<const DMatch*>(d.p), nullptr, n, query_xy, query_stride, nq, train_xy, train_stride,
                        nt, params);
}

PlanarGeometry verifyHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const VerifyParams& params, int query_stride, int train_stride) {
    const int n = (int)matches.size();
    Verifier v(n > 0 ? n : 1, params.hypotheses > 0 && params.hypotheses <= 4096 ? params.hypotheses : 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), "verifyHomography");
    return v.verifyHomographyHost(static_cast<const DMatch*>(d.p), nullptr, n, query_xy, query_stride, nq, train_xy,
                                  train_stride, nt, params);
}

// --- The refit (sift_hip_refine_*).

namespace {

sift_hip_dmatch* abi(DMatch* p) { return reinterpret_cast<sift_hip_dmatch*>(p); }
const sift_hip_dmatch* abi(const DMatch* p) { return reinterpret_cast<const sift_hip_dmatch*>(p); }

// The host forms' mask: one byte per row, or the ABI's refusal of the rows themselves (nothing is read then).
void check_mask(const std::vector<uint8_t>& mask, size_t rows, const char* what) {
    if (mask.size() != rows) throw std::invalid_argument(std::string(what) + ": mask must hold one byte per row");
}

}  // namespace

void Verifier::refineDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                            int nq, const float* train_xy, int train_stride, int nt, float max_error, int rounds,
                            VerifyResult* result, uint8_t* mask, DMatch* out, int* out_count, int* accepted,
                            void* stream) {
    check_throw(sift_hip_refine_fundamental_device(m_handle, abi(matches), count, cap, query_xy, query_stride, nq, train_xy,
                                                   train_stride, nt, max_error, rounds,
                                                   reinterpret_cast<sift_hip_verify_result*>(result), mask, abi(out),
                                                   out_count, accepted, stream),
                "Verifier::refineDevice");
}

void Verifier::refineHomographyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                      int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                      float max_error, int rounds, HomographyResult* result, uint8_t* mask, DMatch* out,
                                      int* out_count, int* accepted, void* stream) {
    check_throw(sift_hip_refine_homography_device(m_handle, abi(matches), count, cap, query_xy, query_stride, nq, train_xy,
                                                  train_stride, nt, max_error, rounds,
                                                  reinterpret_cast<sift_hip_homography_result*>(result), mask, abi(out),
                                                  out_count, accepted, stream),
                "Verifier::refineHomographyDevice");
}

int Verifier::refineHost(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,
                         const float* train_xy, int train_stride, int nt, float max_error, int rounds,
                         VerifyResult& result, std::vector<uint8_t>& mask, std::vector<DMatch>* inliers) {
    if (cap >= 0 && cap <= 65536) check_mask(mask, (size_t)cap, "Verifier::refineHost");
    std::vector<DMatch> list(inliers && cap > 0 && cap <= 65536 ? (size_t)cap : 0);
    int n = 0, accepted = 0;
    check_throw(sift_hip_refine_fundamental_host(m_handle, abi(matches), count, cap, query_xy, query_stride, nq, train_xy,
                                                 train_stride, nt, max_error, rounds,
                                                 reinterpret_cast<sift_hip_verify_result*>(&result),
                                                 mask.empty() ? nullptr : mask.data(),
                                                 inliers ? abi(list.data()) : nullptr, &n, &accepted),
                "Verifier::refineHost");
    if (inliers) {
        list.resize((size_t)n);
        *inliers = std::move(list);
    }
    return accepted;
}

int Verifier::refineHomographyHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                   int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                   float max_error, int rounds, HomographyResult& result, std::vector<uint8_t>& mask,
                                   std::vector<DMatch>* inliers) {
    if (cap >= 0 && cap <= 65536) check_mask(mask, (size_t)cap, "Verifier::refineHomographyHost");
    std::vector<DMatch> list(inliers && cap > 0 && cap <= 65536 ? (size_t)cap : 0);
    int n = 0, accepted = 0;
    check_throw(sift_hip_refine_homography_host(m_handle, abi(matches), count, cap, query_xy, query_stride, nq, train_xy,
                                                train_stride, nt, max_error, rounds,
                                                reinterpret_cast<sift_hip_homography_result*>(&result),
                                                mask.empty() ? nullptr : mask.data(),
                                                inliers ? abi(list.data()) : nullptr, &n, &accepted),
                "Verifier::refineHomographyHost");
    if (inliers) {
        list.resize((size_t)n);
        *inliers = std::move(list);
    }
    return accepted;
}

void Verifier::refineBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                   int query_stride, int train_stride, float max_error, int rounds, VerifyResult* results,
                                   uint8_t* mask, DMatch* out, int* out_counts, int* accepted, void* stream) {
    check_throw(sift_hip_refine_fundamental_batched_device(m_handle, abi(matches), counts, (int)pairs.size(), toAbi(pairs),
                                                           query_stride, train_stride, max_error, rounds,
                                                           reinterpret_cast<sift_hip_verify_result*>(results), mask,
                                                           abi(out), out_counts, accepted, stream),
                "Verifier::refineBatchedDevice");
}

void Verifier::refineHomographyBatchedDevice(const DMatch* matches, const int* counts,
                                             const std::vector<VerifyPair>& pairs, int query_stride, int train_stride,
                                             float max_error, int rounds, HomographyResult* results, uint8_t* mask,
                                             DMatch* out, int* out_counts, int* accepted, void* stream) {
    check_throw(sift_hip_refine_homography_batched_device(m_handle, abi(matches), counts, (int)pairs.size(), toAbi(pairs),
                                                          query_stride, train_stride, max_error, rounds,
                                                          reinterpret_cast<sift_hip_homography_result*>(results), mask,
                                                          abi(out), out_counts, accepted, stream),
                "Verifier::refineHomographyBatchedDevice");
}

std::vector<int> Verifier::refineBatchedHost(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                             int query_stride, int train_stride, float max_error, int rounds,
                                             std::vector<VerifyResult>& results, std::vector<uint8_t>& mask,
                                             std::vector<DMatch>* out, std::vector<int>* out_counts) {
    if (results.size() != pairs.size())
        throw std::invalid_argument("Verifier::refineBatchedHost: one result record per pair");
    const size_t rows = batchRows(pairs);
    if (rows > 0) check_mask(mask, rows, "Verifier::refineBatchedHost");
    std::vector<DMatch> list(out ? rows : 0);
    std::vector<int> n(pairs.size()), accepted(pairs.size());
    check_throw(sift_hip_refine_fundamental_batched_host(
                    m_handle, abi(matches), counts, (int)pairs.size(), toAbi(pairs), query_stride, train_stride, max_error,
                    rounds, reinterpret_cast<sift_hip_verify_result*>(results.data()), mask.empty() ? nullptr : mask.data(),
                    out ? abi(list.data()) : nullptr, n.data(), accepted.data()),
                "Verifier::refineBatchedHost");
    if (out) *out = std::move(list);
    if (out_counts) *out_counts = n;
    return accepted;
}

std::vector<int> Verifier::refineHomographyBatchedHost(const DMatch* matches, const int* counts,
                                                       const std::vector<VerifyPair>& pairs, int query_stride,
                                                       int train_stride, float max_error, int rounds,
                                                       std::vector<HomographyResult>& results, std::vector<uint8_t>& mask,
                                                       std::vector<DMatch>* out, std::vector<int>* out_counts) {
    if (results.size() != pairs.size())
        throw std::invalid_argument("Verifier::refineHomographyBatchedHost: one result record per pair");
    const size_t rows = batchRows(pairs);
    if (rows > 0) check_mask(mask, rows, "Verifier::refineHomographyBatchedHost");
    std::vector<DMatch> list(out ? rows : 0);
    std::vector<int> n(pairs.size()), accepted(pairs.size());
    check_throw(sift_hip_refine_homography_batched_host(
                    m_handle, abi(matches), counts, (int)pairs.size(), toAbi(pairs), query_stride, train_stride, max_error,
                    rounds, reinterpret_cast<sift_hip_homography_result*>(results.data()),
                    mask.empty() ? nullptr : mask.data(), out ? abi(list.data()) : nullptr, n.data(), accepted.data()),
                "Verifier::refineHomographyBatchedHost");
    if (out) *out = std::move(list);
    if (out_counts) *out_counts = n;
    return accepted;
}

TwoViewGeometry verifyFundamental(const std::vector<DMatch>& matches, const float* query_xy, int nq,
                                  const float* train_xy, int nt, const VerifyParams& params, int query_stride,
                                  int train_stride, int refit) {
    if (refit == 0) return verifyFundamental(matches, query_xy, nq, train_xy, nt, params, query_stride, train_stride);
    const int n = (int)matches.size();
    Verifier v(n > 0 ? n : 1, params.hypotheses > 0 && params.hypotheses <= 4096 ? params.hypotheses : 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), "verifyFundamental");
    const sift_hip_verify_params p = toAbi(params);
    VerifyResult r{};
    std::vector<uint8_t> mask(matches.size());
    check_throw(sift_hip_verify_fundamental_host(v.handle(), abi(static_cast<const DMatch*>(d.p)), nullptr, n, query_xy,
                                                 query_stride, nq, train_xy, train_stride, nt, &p,
                                                 reinterpret_cast<sift_hip_verify_result*>(&r), nullptr,
                                                 mask.empty() ? nullptr : mask.data()),
                "verifyFundamental");
    TwoViewGeometry g;
    v.refineHost(static_cast<const DMatch*>(d.p), nullptr, n, query_xy, query_stride, nq, train_xy, train_stride, nt,
                 params.max_error, refit, r, mask, &g.inliers);
    for (int i = 0; i < 9; i++) g.F[i] = r.F[i];
    g.hypothesis = r.hypothesis;
    return g;
}

PlanarGeometry verifyHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const VerifyParams& params, int query_stride, int train_stride, int refit) {
    if (refit == 0) return verifyHomography(matches, query_xy, nq, train_xy, nt, params, query_stride, train_stride);
    const int n = (int)matches.size();
    Verifier v(n > 0 ? n : 1, params.hypotheses > 0 && params.hypotheses <= 4096 ? params.hypotheses : 1);
    DeviceBlock d(sizeof(DMatch) * matches.size());
    if (n > 0) check_throw(sift_hip_memcpy_h2d(d.p, matches.data(), sizeof(DMatch) * matches.size()), "verifyHomography");
    const sift_hip_verify_params p = toAbi(params);
    HomographyResult r{};
    std::vector<uint8_t> mask(matches.size());
    check_throw(sift_hip_verify_homography_host(v.handle(), abi(static_cast<const DMatch*>(d.p)), nullptr, n, query_xy,
                                                query_stride, nq, train_xy, train_stride, nt, &p,
                                                reinterpret_cast<sift_hip_homography_result*>(&r), nullptr,
                                                mask.empty() ? nullptr : mask.data()),
                "verifyHomography");
    PlanarGeometry g;
    v.refineHomographyHost(static_cast<const DMatch*>(d.p), nullptr, n, query_xy, query_stride, nq, train_xy, train_stride,
                           nt, params.max_error, refit, r, mask, &g.inliers);
    for (int i = 0; i < 9; i++) g.H[i] = r.H[i];
    g.hypothesis = r.hypothesis;
    return g;
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
