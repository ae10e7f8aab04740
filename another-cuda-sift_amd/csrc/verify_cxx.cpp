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

}  // namespace

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

void projectHomographyDevice(const float* H, const float* xy, int stride, int n, float* out_xy, int out_stride,
                             void* stream) {
    check_throw(sift_hip_project_homography_device(H, xy, stride, n, out_xy, out_stride, stream),
                "projectHomographyDevice");
}

}  // namespace sift_cuda
