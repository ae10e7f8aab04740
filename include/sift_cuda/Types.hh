// Host-side element types of the drop-in surface.  The reference exposes CUDA's
// float3 / float4 / half (Detector.hh:54-60); these PODs have the same layout
// and member names so caller code like `kpts[i].x` or `(float)desc[k]` compiles
// unchanged, without pulling HIP headers into the caller.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

namespace sift_cuda {

struct Float3 {
    float x, y, z;
};
struct Float4 {
    float x, y, z, w;
};

// IEEE binary16 storage; SIFT descriptor values are integers 0..255, exact here.
struct Half {
    uint16_t bits{0};
    operator float() const {
        const uint32_t s = (bits & 0x8000u) << 16, e = (bits >> 10) & 0x1f, m = bits & 0x3ffu;
        uint32_t f;
        if (e == 0) {
            if (m == 0) {
                f = s;
            } else {  // subnormal
                int sh = 0;
                uint32_t mm = m;
                while (!(mm & 0x400u)) { mm <<= 1; sh++; }
                f = s | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13);
            }
        } else if (e == 31) {
            f = s | 0x7f800000u | (m << 13);
        } else {
            f = s | ((e + 112) << 23) | (m << 13);
        }
        float out;
        std::memcpy(&out, &f, 4);
        return out;
    }
};
static_assert(sizeof(Float3) == 12 && sizeof(Float4) == 16 && sizeof(Half) == 2, "layout");

// A caller-supplied keypoint for Detector::compute: cv::KeyPoint minus
// class_id, layout-identical to sift_hip_keypoint (include/sift_hip.h).
// x, y, size in input-image pixels, angle in degrees (0..360), octave in
// OpenCV's packed form (octave & 255 | layer << 8 | xi << 16).
struct KeyPoint {
    float x, y, size, angle, response;
    int octave;
};
static_assert(sizeof(KeyPoint) == 24 && offsetof(KeyPoint, octave) == 20, "layout of sift_hip_keypoint");

// One match of matchList: cv::DMatch's fields in its order, layout-identical to
// sift_hip_dmatch.  distance is the L2 distance (not squared).
struct DMatch {
    int queryIdx, trainIdx, imgIdx;
    float distance;
};
static_assert(sizeof(DMatch) == 16 && offsetof(DMatch, distance) == 12, "layout of sift_hip_dmatch");

// The keep rule of matchList (sift_hip_match_filter, include/sift_hip.h; the
// defaults are sift_hip_default_match_filter's).
struct MatchFilter {
    float ratio = 0.8f;            // Lowe's ratio; <= 0: no ratio test
    int ratio_on_squared = 0;      // the ratio applies to squared distances (matchBruteForce's convention)
    int ratio_both_ways = 0;       // the reverse top-2 of the matched row passes the ratio test too
    float max_distance = 0.f;      // cap on the L2 distance; <= 0: none
    int cross_check = 1;           // mutual nearest neighbours only (cv::BFMatcher's crossCheck)
};
static_assert(sizeof(MatchFilter) == 20, "layout of sift_hip_match_filter");

// The search window of matchListGuided / matchGuided (sift_hip_match_gate,
// include/sift_hip.h): device rows of floats with x, y first for both sets --
// row i of the query set at query_xy[i * query_stride + {0, 1}] -- and the
// window's half-size: a train row is a candidate of a query when both
// coordinates differ by at most radius pixels.
struct MatchGate {
    const float* query_xy = nullptr;
    int query_stride = 3;          // floats per row, >= 2; 3: a Detector's device_kpts as it is
    const float* train_xy = nullptr;
    int train_stride = 3;
    float radius = 0.f;            // pixels, > 0; infinity: no gate
};

// The gate of matchListEpipolar / matchEpipolar (sift_hip_match_epipolar_gate,
// include/sift_hip.h): the positions as MatchGate's, the fundamental matrix of
// the pair and the width of the band round a query's epipolar line.  A train
// row is a candidate of a query when its Sampson distance under F is at most
// max_error pixels and it lies in the query's window (radius; infinity: none).
struct EpipolarGate {
    const float* query_xy = nullptr;
    int query_stride = 3;
    const float* train_xy = nullptr;
    int train_stride = 3;
    float radius = std::numeric_limits<float>::infinity();
    float F[9] = {};               // row-major, x_train^T F x_query = 0 (cv::findFundamentalMat(query, train))
    float max_error = 0.f;         // pixels, > 0 and finite
};

// Non-owning view of a device array owned by a Detector (stands in for the
// reference's thrust::device_vector members, Detector.hh:54-57; data()/size()
// as there).  data() is read-only: the detector derives data from what it
// writes (the matcher's int8 sidecar of the descriptor rows), so a caller that
// writes takes mutable_data(), which tells the detector (for descriptor
// buffers, sift_hip_descriptors_written: matches then convert those rows).
template <class T>
class DeviceBuffer {
public:
    using WriteHook = void (*)(const void*);
    DeviceBuffer() = default;
    DeviceBuffer(T* p, size_t n, WriteHook on_write = nullptr) : ptr_(p), n_(n), on_write_(on_write) {}
    const T* data() const { return ptr_; }
    T* mutable_data() const {
        if (on_write_ && ptr_) on_write_(ptr_);
        return ptr_;
    }
    size_t size() const { return n_; }

private:
    T* ptr_{nullptr};
    size_t n_{0};
    WriteHook on_write_{nullptr};
};

}  // namespace sift_cuda
