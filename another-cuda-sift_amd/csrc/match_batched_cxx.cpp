// sift_cuda::BatchMatcher / matchListGuidedBatchedDevice / matchListEpipolarBatchedDevice
// (include/sift_cuda/Detector.hh) over the C ABI in include/sift_hip.h.  Plain
// C++ (g++): no HIP headers, no device code.
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

}  // namespace sift_cuda
