// sift_cuda::BatchMatcher / matchListGuidedBatchedDevice / matchListEpipolarBatchedDevice
// (include/sift_cuda/Detector.hh) over the C ABI in include/sift_hip.h.  Plain
// C++ (g++): no HIP headers, no device code.
#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "sift_cuda/Detector.hh"
#include "sift_hip.h"

namespace sift_cuda {

namespace {

void check_throw(int rc, const char* what) {
    if (rc == SIFT_HIP_OK) return;
    const std::string msg = std::string(what) + ": " + sift_hip_last_error() + " (status " + std::to_string(rc) + ")";
    if (rc == SIFT_HIP_ERR_INVALID) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}

// The pairs as the ABI takes them: four arrays and the position records.
struct AbiPairs {
    std::vector<const uint16_t*> q, t;
    std::vector<int> nq, nt;
    std::vector<sift_hip_match_positions> pos;
    explicit AbiPairs(const std::vector<GuidedPair>& pairs) {
        for (const GuidedPair& p : pairs) {
            q.push_back(reinterpret_cast<const uint16_t*>(p.des));
            t.push_back(reinterpret_cast<const uint16_t*>(p.src));
            nq.push_back(p.num_des);
            nt.push_back(p.num_src);
            pos.push_back(sift_hip_match_positions{p.des_xy, p.src_xy});
        }
    }
};

sift_hip_match_filter toAbi(const MatchFilter& f) {
    return sift_hip_match_filter{f.ratio, f.ratio_on_squared, f.ratio_both_ways, f.max_distance, f.cross_check};
}

}  // namespace

BatchMatcher::BatchMatcher(int max_query, int max_train, int max_pairs, int device) {
    check_throw(sift_hip_matcher_create(device, max_query, max_train, max_pairs, &m_handle), "BatchMatcher::BatchMatcher");
}

BatchMatcher::~BatchMatcher() { (void)sift_hip_matcher_destroy(m_handle); }

void matchListGuidedBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                  int src_stride, float radius, const MatchFilter& filter, DMatch* out, int* counts,
                                  void* stream) {
    const AbiPairs a(pairs);
    const sift_hip_match_filter f = toAbi(filter);
    check_throw(sift_hip_match_list_guided_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(),
                                                   a.t.data(), a.nt.data(), a.pos.data(), des_stride, src_stride, radius,
                                                   &f, reinterpret_cast<sift_hip_dmatch*>(out), counts, stream),
                "matchListGuidedBatchedDevice");
}

void matchListEpipolarBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                    int src_stride, float radius, const void* geometry, int geometry_stride_bytes,
                                    float max_error, const MatchFilter& filter, DMatch* out, int* counts, void* stream) {
    const AbiPairs a(pairs);
    const sift_hip_match_filter f = toAbi(filter);
    check_throw(sift_hip_match_list_epipolar_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(),
                                                     a.t.data(), a.nt.data(), a.pos.data(), des_stride, src_stride,
                                                     radius, geometry, geometry_stride_bytes, max_error, &f,
                                                     reinterpret_cast<sift_hip_dmatch*>(out), counts, stream),
                "matchListEpipolarBatchedDevice");
}

// --- k nearest neighbours (sift_hip_match_knn_*) ---------------------------------
namespace {

struct MatcherDeleter {
    void operator()(sift_hip_matcher* m) const { sift_hip_matcher_destroy(m); }
};

// The thread-local matcher of matchKnn / matchKnnList, grown to hold the call.
sift_hip_matcher* knn_matcher(int num_des, int num_src, const char* what) {
    thread_local std::unique_ptr<sift_hip_matcher, MatcherDeleter> matcher;
    thread_local int capQ = 0, capT = 0;
    if (!matcher || num_des > capQ || num_src > capT) {
        capQ = std::max(std::max(num_des, 1), capQ);
        capT = std::max(std::max(num_src, 1), capT);
        sift_hip_matcher_t m = nullptr;
        check_throw(sift_hip_matcher_create(-1, capQ, capT, 1, &m), what);
        matcher.reset(m);
    }
    return matcher.get();
}

}  // namespace

std::vector<std::vector<DMatch>> matchKnn(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                          int num_src, int k) {
    if (k < 1 || k > SIFT_HIP_KNN_MAX) throw std::invalid_argument("matchKnn: k outside 1..SIFT_HIP_KNN_MAX");
    std::vector<std::vector<DMatch>> out((size_t)std::max(num_des, 0));
    if (num_des <= 0 || num_src <= 0) return out;
    std::vector<int> idx((size_t)num_des * k);
    std::vector<float> d2((size_t)num_des * k);
    check_throw(sift_hip_match_knn_host(knn_matcher(num_des, num_src, "matchKnn"),
                                        reinterpret_cast<const uint16_t*>(des.data()), num_des,
                                        reinterpret_cast<const uint16_t*>(src.data()), num_src, k, idx.data(), d2.data()),
                "matchKnn");
    for (int i = 0; i < num_des; i++)
        for (int j = 0; j < k && idx[(size_t)i * k + j] >= 0; j++)
            out[(size_t)i].push_back(DMatch{i, idx[(size_t)i * k + j], 0, std::sqrt(d2[(size_t)i * k + j])});
    return out;
}

std::vector<DMatch> matchKnnList(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src, int num_src,
                                 int k, float max_distance) {
    if (k < 1 || k > SIFT_HIP_KNN_MAX) throw std::invalid_argument("matchKnnList: k outside 1..SIFT_HIP_KNN_MAX");
    std::vector<DMatch> out;
    if (num_des <= 0 || num_src <= 0) return out;
    out.resize((size_t)num_des * k);
    int count = 0;
    check_throw(sift_hip_match_knn_list_host(knn_matcher(num_des, num_src, "matchKnnList"),
                                             reinterpret_cast<const uint16_t*>(des.data()), num_des,
                                             reinterpret_cast<const uint16_t*>(src.data()), num_src, k, max_distance,
                                             reinterpret_cast<sift_hip_dmatch*>(out.data()), (int)out.size(), &count),
                "matchKnnList");
    out.resize((size_t)count);
    return out;
}

void matchKnnBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int k, int* idx, float* d2,
                           void* stream) {
    const AbiPairs a(pairs);
    check_throw(sift_hip_match_knn_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(), a.t.data(),
                                           a.nt.data(), k, idx, d2, stream),
                "matchKnnBatchedDevice");
}

void matchKnnListBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int k, float max_distance,
                               DMatch* out, int* counts, void* stream) {
    const AbiPairs a(pairs);
    check_throw(sift_hip_match_knn_list_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(), a.t.data(),
                                                a.nt.data(), k, max_distance, reinterpret_cast<sift_hip_dmatch*>(out),
                                                counts, stream),
                "matchKnnListBatchedDevice");
}

// --- k nearest neighbours inside a gate (sift_hip_match_knn_guided_* / *_epipolar_*) ---------
namespace {

sift_hip_match_gate abi(const MatchGate& g) {
    return sift_hip_match_gate{g.query_xy, g.query_stride, g.train_xy, g.train_stride, g.radius};
}
sift_hip_match_epipolar_gate abi(const EpipolarGate& g) {
    sift_hip_match_epipolar_gate a{g.query_xy, g.query_stride, g.train_xy, g.train_stride, g.radius, {}, g.max_error};
    std::copy(g.F, g.F + 9, a.F);
    return a;
}

// The bodies for either gate: `call` is the C ABI's host entry point for the gate's type.  The ABI judges k and the
// gate before it looks at the matcher, so a bad argument throws whatever the sets are.
template <class AbiGate, class Call>
std::vector<std::vector<DMatch>> knn_gated(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                           int num_src, const AbiGate& gate, int k, Call call, const char* what) {
    if (k < 1 || k > SIFT_HIP_KNN_MAX) throw std::invalid_argument(std::string(what) + ": k outside 1..SIFT_HIP_KNN_MAX");
    std::vector<std::vector<DMatch>> out((size_t)std::max(num_des, 0));
    std::vector<int> idx((size_t)std::max(num_des, 0) * k, -1);
    std::vector<float> d2((size_t)std::max(num_des, 0) * k);
    check_throw(call(knn_matcher(num_des, num_src, what), reinterpret_cast<const uint16_t*>(des.data()), num_des,
                     reinterpret_cast<const uint16_t*>(src.data()), num_src, &gate, k, idx.data(), d2.data()),
                what);
    for (int i = 0; i < num_des; i++)
        for (int j = 0; j < k && idx[(size_t)i * k + j] >= 0; j++)
            out[(size_t)i].push_back(DMatch{i, idx[(size_t)i * k + j], 0, std::sqrt(d2[(size_t)i * k + j])});
    return out;
}

template <class AbiGate, class Call>
std::vector<DMatch> knn_gated_list(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                   int num_src, const AbiGate& gate, int k, float max_distance, Call call,
                                   const char* what) {
    if (k < 1 || k > SIFT_HIP_KNN_MAX) throw std::invalid_argument(std::string(what) + ": k outside 1..SIFT_HIP_KNN_MAX");
    std::vector<DMatch> out((size_t)std::max(num_des, 0) * k);
    int count = 0;
    check_throw(call(knn_matcher(num_des, num_src, what), reinterpret_cast<const uint16_t*>(des.data()), num_des,
                     reinterpret_cast<const uint16_t*>(src.data()), num_src, &gate, k, max_distance,
                     reinterpret_cast<sift_hip_dmatch*>(out.data()), (int)out.size(), &count),
                what);
    out.resize((size_t)count);
    return out;
}

}  // namespace

std::vector<std::vector<DMatch>> matchKnnGuided(const DeviceBuffer<Half>& des, int num_des,
                                                const DeviceBuffer<Half>& src, int num_src, const MatchGate& gate,
                                                int k) {
    return knn_gated(des, num_des, src, num_src, abi(gate), k, sift_hip_match_knn_guided_host, "matchKnnGuided");
}

std::vector<std::vector<DMatch>> matchKnnEpipolar(const DeviceBuffer<Half>& des, int num_des,
                                                  const DeviceBuffer<Half>& src, int num_src, const EpipolarGate& gate,
                                                  int k) {
    return knn_gated(des, num_des, src, num_src, abi(gate), k, sift_hip_match_knn_epipolar_host, "matchKnnEpipolar");
}

std::vector<DMatch> matchKnnListGuided(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                       int num_src, const MatchGate& gate, int k, float max_distance) {
    return knn_gated_list(des, num_des, src, num_src, abi(gate), k, max_distance, sift_hip_match_knn_list_guided_host,
                          "matchKnnListGuided");
}

std::vector<DMatch> matchKnnListEpipolar(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                         int num_src, const EpipolarGate& gate, int k, float max_distance) {
    return knn_gated_list(des, num_des, src, num_src, abi(gate), k, max_distance, sift_hip_match_knn_list_epipolar_host,
                          "matchKnnListEpipolar");
}

void matchKnnGuidedBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                 int src_stride, float radius, int k, int* idx, float* d2, void* stream) {
    const AbiPairs a(pairs);
    check_throw(sift_hip_match_knn_guided_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(),
                                                  a.t.data(), a.nt.data(), a.pos.data(), des_stride, src_stride, radius,
                                                  k, idx, d2, stream),
                "matchKnnGuidedBatchedDevice");
}

void matchKnnEpipolarBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                   int src_stride, float radius, const void* geometry, int geometry_stride_bytes,
                                   float max_error, int k, int* idx, float* d2, void* stream) {
    const AbiPairs a(pairs);
    check_throw(sift_hip_match_knn_epipolar_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(),
                                                    a.t.data(), a.nt.data(), a.pos.data(), des_stride, src_stride, radius,
                                                    geometry, geometry_stride_bytes, max_error, k, idx, d2, stream),
                "matchKnnEpipolarBatchedDevice");
}

void matchKnnListGuidedBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                     int src_stride, float radius, int k, float max_distance, DMatch* out, int* counts,
                                     void* stream) {
    const AbiPairs a(pairs);
    check_throw(sift_hip_match_knn_list_guided_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(),
                                                       a.t.data(), a.nt.data(), a.pos.data(), des_stride, src_stride,
                                                       radius, k, max_distance,
                                                       reinterpret_cast<sift_hip_dmatch*>(out), counts, stream),
                "matchKnnListGuidedBatchedDevice");
}

void matchKnnListEpipolarBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                       int src_stride, float radius, const void* geometry, int geometry_stride_bytes,
                                       float max_error, int k, float max_distance, DMatch* out, int* counts,
                                       void* stream) {
    const AbiPairs a(pairs);
    check_throw(sift_hip_match_knn_list_epipolar_batched(matcher.handle(), (int)pairs.size(), a.q.data(), a.nq.data(),
                                                         a.t.data(), a.nt.data(), a.pos.data(), des_stride, src_stride,
                                                         radius, geometry, geometry_stride_bytes, max_error, k,
                                                         max_distance, reinterpret_cast<sift_hip_dmatch*>(out), counts,
                                                         stream),
                "matchKnnListEpipolarBatchedDevice");
}

}  // namespace sift_cuda
