// Drop-in for /root/reference/sift_cuda/interface/Detector.hh:24-96.
// Same class name, constructor, public methods and public result members;
// device members are non-owning DeviceBuffer views, host members std::vector.
// No HIP/CUDA header is included: everything goes through include/sift_hip.h.
#pragma once
#include <string>
#include <vector>

#include "sift_cuda/CudaSiftConfig.hh"
#include "sift_cuda/HostImage.hh"
#include "sift_cuda/Types.hh"

struct sift_hip_detector;
struct sift_hip_matcher;

namespace sift_cuda {

class Detector {
public:
    explicit Detector(const CudaSiftConfig& config);
    // Extra: bound to an explicit device instead of the calling thread's
    // current one (one Detector per GPU, each driven by its own host thread:
    // sift_cuda/MultiDetector.hh).
    Detector(const CudaSiftConfig& config, int device);
    ~Detector();
    Detector(const Detector&) = delete;
    Detector& operator=(const Detector&) = delete;

    // Detector.cu:17-39: allocate, capture the pipeline graph, warm up.
    // Returns false when the image size is unset (as the reference does).
    bool gpuWarmUpAndAllocate();

    // Detector.cu:133-233: synchronous; results valid until the next call.
    void detectAndCompute(const Imagef& image);
    // Extra: 8-bit frame (Image8U, HostImage.hh:187); converted on the GPU,
    // results identical to the Imagef holding the same values.
    void detectAndCompute(const Image8U& image);
    // Extra: pipelined input (sift_hip_submit / sift_hip_wait).  submit()
    // stages and uploads the frame while earlier frames compute and returns a
    // ticket; wait(ticket) makes that frame's results (and its predecessor's
    // descriptors as prev_descriptor) current.  Frames in flight compute
    // concurrently on up to setLanes() compute lanes (default 2), at most two
    // per lane past the last waited one.
    long long submit(const Imagef& image);
    long long submit(const Image8U& image);
    // Extra: the same for a frame already in device memory (fp32 or 8-bit,
    // row stride in bytes), read after `hip_stream` reaches the call; the
    // buffer must stay unchanged until wait(ticket).
    long long submitDevice(const void* device_image, size_t row_stride_bytes, bool u8 = false,
                           void* hip_stream = nullptr);
    void wait(long long ticket);
    // Extra: compute lanes for frames in flight (sift_hip_set_lanes, 1..4);
    // before gpuWarmUpAndAllocate.  1 = every frame on one stream in order.
    void setLanes(int lanes);
    // Extra: submitDevice frames run in launch groups of `frames`
    // (sift_hip_set_micro_batch, 1..16); before gpuWarmUpAndAllocate.
    void setMicroBatch(int frames);
    // Extra: automatic launch groups of up to `frames` once every lane is
    // busy (sift_hip_set_auto_micro_batch; default 8, 0 = off); before
    // gpuWarmUpAndAllocate.
    void setAutoMicroBatch(int frames);
    // Extra: image already in device memory (fp32, row stride in bytes).
    void detectAndComputeDevice(const float* device_image, size_t row_stride_bytes, void* hip_stream = nullptr);

    // Extra: cv::SIFT::detectAndCompute(image, mask, ...) -- a detection mask
    // (Image8U of the frame's size; sift_hip_detect_masked).  A keypoint is
    // dropped when mask[(int)(y + 0.5f)][(int)(x + 0.5f)] == 0 (OpenCV's
    // KeyPointsFilter::runByPixelsMask; any non-zero byte keeps it), after
    // retainBest(numFeatures) as in OpenCV: total_size, the device buffers,
    // prev_descriptor of the next frame and the host results hold the kept rows
    // only, in the unmasked order.  Synchronous.  A mask of the wrong size
    // throws std::invalid_argument (nothing runs).  No submit / submitDevice
    // variants take a mask, and compute() takes none (OpenCV ignores the mask
    // for provided keypoints).
    void detectAndCompute(const Imagef& image, const Image8U& mask);
    void detectAndCompute(const Image8U& image, const Image8U& mask);
    // Extra: the same for a device image (fp32 or 8-bit) and a device mask
    // (col_width x row_width bytes, row stride in bytes, 0 = packed), read in
    // place after `hip_stream` reaches the call; returns when the results are
    // ready.  A null mask is the unmasked call.
    void detectAndComputeDevice(const void* device_image, size_t row_stride_bytes, bool u8, const uint8_t* device_mask,
                                size_t mask_stride_bytes, void* hip_stream = nullptr);

    // Extra: descriptors for the caller's own keypoints (cv::Feature2D::compute;
    // sift_hip_compute / sift_hip_compute_u8): the frame's pyramid is built and
    // the keypoints described in the caller's order -- total_size =
    // keypoints.size(), device_kpts / device_features hold the input,
    // prev_descriptor the previous frame's rows.  Synchronous.  Throws
    // std::invalid_argument when a keypoint is invalid or there are more than
    // the result capacity (nothing runs), std::runtime_error on any other error.
    void compute(const Imagef& image, const std::vector<KeyPoint>& keypoints);
    void compute(const Image8U& image, const std::vector<KeyPoint>& keypoints);
    // Extra: the same for a device image (fp32 or 8-bit, row stride in bytes)
    // and n device keypoints, read after `hip_stream` reaches the call;
    // returns when the results are ready.  Device keypoints are validated on
    // the GPU: an invalid one gets an all-zero row and sets overflow flag 16
    // (reported on stderr like a capacity overflow).
    void computeDevice(const void* device_image, size_t row_stride_bytes, bool u8, const KeyPoint* device_keypoints,
                       int n, void* hip_stream = nullptr);

    // Detector.cu:606-634: copies total_size results (+ descriptors) to host.
    void copyToHost(bool descriptor);
    // Extra: the same rows without the copy into final_kpts / final_features /
    // descriptors -- views of the detector's pinned host results of the
    // current frame (sift_hip_results_host), valid while that frame is the
    // current or the previous one.
    struct HostResults {
        const Float3* kpts = nullptr;
        const Float4* features = nullptr;
        const Half* descriptors = nullptr;  // 128 per keypoint; null unless requested
        int count = 0;
    };
    HostResults hostResults(bool descriptor);

    // Detector.hh:48-51 debug snapshot switch: every following detectAndCompute
    // writes its stage dumps into `path` (sift_hip_set_datagen: meta.json,
    // input, every Gaussian plane, candidates, keypoints, descriptors);
    // tests/stage_check.py replays them.  An empty path switches it off.
    void setDataGen(const std::string& path);
    // Extra: OpenCV's sequential float descriptor histogram (bit-identical
    // descriptors; sift_hip_set_descriptor_mode(SIFT_HIP_DESC_EXACT)).  Call
    // before gpuWarmUpAndAllocate; the default is the fixed-point histogram.
    void setExactDescriptors(bool exact);
    // Extra: RootSIFT rows (sift_hip_set_descriptor_norm(SIFT_HIP_NORM_ROOT): the
    // square root of the L1-normalised row at OpenCV's scale, computed in the
    // descriptor kernel; the rule is spelled out in include/sift_hip.h).  Every
    // row the detector writes follows it; keypoints are unchanged.  Call before
    // gpuWarmUpAndAllocate: afterwards, or with setDataGen active, it throws
    // std::runtime_error.  Independent of setExactDescriptors.
    void setRootSift(bool root);
    bool rootSift() const;
    // tool/perf.cu:43-100 (HostInterface.hh:11-69 run<Stage>): one stage --
    // "pyramid", "extrema", "refine", "orientation", "order", "descriptor" --
    // alone on a setDataGen dump's recorded input; its outputs go to out_dir
    // in the dump's formats (sift_hip_replay_stage).  Discards the current results.
    void replayStage(const std::string& dump_dir, const std::string& stage, const std::string& out_dir);

    int numOctaves() const { return m_nOctaves; }
    sift_hip_detector* handle() const { return m_handle; }

    // Results (Detector.hh:53-62).
    DeviceBuffer<Float3> device_kpts;      // {x, y, layer}
    DeviceBuffer<Float4> device_features;  // {octave (packed, as float), size, response, angle}
    DeviceBuffer<Half> device_descriptor;  // 128 per keypoint, values 0..255
    DeviceBuffer<Half> prev_descriptor;    // previous frame's descriptors
    std::vector<Float3> final_kpts{};
    std::vector<Float4> final_features{};
    std::vector<Half> descriptors{};
    int max_kpts = 5000;
    int total_size{0};

private:
    void refreshViews();
    void warnOverflow();
    CudaSiftConfig m_config{};
    sift_hip_detector* m_handle{nullptr};
    bool m_initialized{false};
    int m_nOctaves{0};
    int m_overflowWarned{0};  // overflow flags already reported on stderr
    std::string m_debug_path;
};

// Match.cuh:9-14: for each of the num_des rows of `des`, the index of its
// nearest row of `src` if it passes Lowe's test on squared distances
// (d1^2 < 0.8 d2^2, the reference's Match.cu:172 convention), else -1.
std::vector<int> matchBruteForce(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                 int num_src);

// Extra: the RootSIFT rule for n rows of 128 values the detector did not write
// with setRootSift (a database's rows, a kept frame, another extractor's):
// device rows on `stream` (not synchronised; out == in transforms in place), or
// host rows through the device, synchronously (sift_hip_rootsift_device / _host).
// A detector's own buffer is passed as mutable_data(), so that later matches
// convert the written rows.  Rows of the two norms must not be matched against
// each other.  What the ABI refuses throws std::invalid_argument.
void rootSiftDevice(const Half* in, int n, Half* out, void* stream = nullptr);
void rootSiftHost(const Half* in, int n, Half* out);

// Extra: the usable match list in one device operation (sift_hip_match_list_host)
// -- top-2 search in both directions, the filter (ratio test, distance cap,
// cross check = cv::BFMatcher(NORM_L2, crossCheck = true)) and compaction on the
// GPU: the kept (queryIdx, trainIdx, distance) records in ascending queryIdx,
// imgIdx 0.  The rule is spelled out in include/sift_hip.h.  Synchronous; a
// thread-local matcher as matchBruteForce's, sized so both directions fit.
// OpencvUtils::cvtMatchToDMatch turns the result into std::vector<cv::DMatch>.
std::vector<DMatch> matchList(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src, int num_src,
                              const MatchFilter& filter = {});

// Extra: matchList inside a search window (sift_hip_match_list_guided_host) --
// row t of src is a candidate of row i of des when both coordinates of their
// positions differ by at most gate.radius pixels, and the top-2 search of both
// directions, the ratio test and the cross check see candidates only
// (ORB-SLAM's search by projection, COLMAP's guided match).  The tracker loop:
//     gate.query_xy = the previous frame's positions (a device copy of its
//                     device_kpts) or the caller's predictions,
//     gate.train_xy = reinterpret_cast<const float*>(det.device_kpts.data()),
//     both strides 3, gate.radius = the search radius in pixels;
//     matchListGuided(det.prev_descriptor, n0, det.device_descriptor, n1, gate).
// Synchronous; the thread-local matcher is sized as matchList's.  A bad gate
// (null positions, a stride below 2, a radius that is not > 0) throws
// std::invalid_argument.
std::vector<DMatch> matchListGuided(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                    int num_src, const MatchGate& gate, const MatchFilter& filter = {});

// Extra: matchBruteForce inside the same window, with its ratio convention
// (0.8 on squared distances): the nearest candidate of each des row if it
// passes the test against the second-nearest candidate, else -1; a row with one
// candidate matches it.
std::vector<int> matchGuided(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src, int num_src,
                             const MatchGate& gate);

// Extra: matchListGuided / matchGuided under a fundamental matrix
// (sift_hip_match_list_epipolar_host, sift_hip_match_epipolar_device): row t of
// src is a candidate of row i of des when it lies within gate.max_error pixels
// (Sampson distance) of i's epipolar line under gate.F, and inside the window
// gate.radius when that is finite -- COLMAP's guided match, ORB-SLAM's
// SearchForTriangulation.  F from the relative pose of two keyframes, a stereo
// rig, or a RANSAC pass over matchList's output; the rule is spelled out in
// include/sift_hip.h.  A bad gate (as above, or a max_error that is not > 0 and
// finite, a non-finite or all-zero F) throws std::invalid_argument.
std::vector<DMatch> matchListEpipolar(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                      int num_src, const EpipolarGate& gate, const MatchFilter& filter = {});
std::vector<int> matchEpipolar(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src, int num_src,
                               const EpipolarGate& gate);

// Extra: the guided match lists of P pairs in one pass, over raw device
// pointers and enqueued on a stream (sift_hip_match_list_guided_batched /
// sift_hip_match_list_epipolar_batched), so that the chain batched match ->
// Verifier::verify*BatchedDevice -> (projectHomographyBatchedDevice ->) guided
// rematch never returns to the host.  A BatchMatcher owns the scratch of its
// calls (sift_hip_matcher_create); calls on one must be ordered.  With a filter
// that needs the reverse direction max_query and max_train both bound both sets,
// and max_pairs >= 2 P puts both directions into one pass.
class BatchMatcher {
public:
    BatchMatcher(int max_query, int max_train, int max_pairs, int device = -1);
    ~BatchMatcher();
    BatchMatcher(const BatchMatcher&) = delete;
    BatchMatcher& operator=(const BatchMatcher&) = delete;
    sift_hip_matcher* handle() const { return m_handle; }

private:
    sift_hip_matcher* m_handle = nullptr;
};

// One pair of a batched guided call: its fp16 descriptor rows and position rows, all device memory.
struct GuidedPair {
    const Half* des = nullptr;
    int num_des = 0;
    const Half* src = nullptr;
    int num_src = 0;
    const float* des_xy = nullptr;
    const float* src_xy = nullptr;
};

// Pair p's records (imgIdx = p) start at row sum_{r<p} num_des[r] of `out`, its
// count is counts[p] (device ints); both are what matchListGuided /
// matchListEpipolar give on the pair.  The strides, the radius and max_error are
// the call's.  geometry: device memory, pair p's nine floats at geometry +
// p * geometry_stride_bytes (sizeof(VerifyResult) for verifyBatchedDevice's
// results as they lie); a record with a non-finite entry or all zero gives its
// pair an empty list.  What the ABI refuses throws std::invalid_argument.
void matchListGuidedBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                  int src_stride, float radius, const MatchFilter& filter, DMatch* out, int* counts,
                                  void* stream = nullptr);
void matchListEpipolarBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                    int src_stride, float radius, const void* geometry, int geometry_stride_bytes,
                                    float max_error, const MatchFilter& filter, DMatch* out, int* counts,
                                    void* stream = nullptr);

// Extra: cv::BFMatcher::knnMatch(des, src, k), 1 <= k <= SIFT_HIP_KNN_MAX (8),
// on the device without a distance matrix (sift_hip_match_knn_host): for each
// of the num_des rows its min(k, num_src) nearest rows of src in ascending
// (distance, trainIdx) order -- a tie at any rank goes to the lower index --
// with real L2 distances, imgIdx 0.  OpencvUtils::cvtMatchToDMatch converts each
// row.  Synchronous; a thread-local matcher as matchBruteForce's.  A k outside
// the range throws std::invalid_argument.
std::vector<std::vector<DMatch>> matchKnn(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                          int num_src, int k);

// Extra: cv::BFMatcher::radiusMatch capped at k per query as one flat list
// (sift_hip_match_knn_list_host): the neighbours of matchKnn within
// max_distance (<= 0: no cap) in (queryIdx, rank) order -- the candidates a
// verifier chooses among where the ratio test would discard a repeated
// structure's right match.  Verifier::verify* take the list as it is.
std::vector<DMatch> matchKnnList(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src, int num_src,
                                 int k, float max_distance = 0.f);

// The device forms, enqueued on a stream (sift_hip_match_knn_batched /
// sift_hip_match_knn_list_batched; the positions of a GuidedPair are not read).
// idx / d2: device, k entries per des row, pair p from row sum_{r<p} num_des[r]
// (-1 / FLT_MAX where src has fewer rows; d2 squared).  out: device, pair p's
// records (imgIdx = p) from row k * sum_{r<p} num_des[r], counts[p] of them.
// The first k-NN call on a BatchMatcher allocates (not under stream capture).
void matchKnnBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int k, int* idx, float* d2,
                           void* stream = nullptr);
void matchKnnListBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int k, float max_distance,
                               DMatch* out, int* counts, void* stream = nullptr);

// Extra: matchKnn / matchKnnList inside a gate -- cv::DescriptorMatcher::
// knnMatch(des, src, k, mask) with the window of MatchGate or the epipolar band
// of EpipolarGate as the mask (sift_hip_match_knn_guided_host and its kin; the
// rule is in include/sift_hip.h, "Gated k nearest neighbours"): for each des row
// its min(k, candidates) nearest candidates in ascending (distance, trainIdx)
// order.  After a first verify pass the rematch under its F keeps every twin
// inside the band for a second pass to choose from.  Synchronous; the
// thread-local matcher of matchKnn.  A k outside 1..8 or a bad gate throws
// std::invalid_argument.
std::vector<std::vector<DMatch>> matchKnnGuided(const DeviceBuffer<Half>& des, int num_des,
                                                const DeviceBuffer<Half>& src, int num_src, const MatchGate& gate,
                                                int k);
std::vector<std::vector<DMatch>> matchKnnEpipolar(const DeviceBuffer<Half>& des, int num_des,
                                                  const DeviceBuffer<Half>& src, int num_src, const EpipolarGate& gate,
                                                  int k);
std::vector<DMatch> matchKnnListGuided(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                       int num_src, const MatchGate& gate, int k, float max_distance = 0.f);
std::vector<DMatch> matchKnnListEpipolar(const DeviceBuffer<Half>& des, int num_des, const DeviceBuffer<Half>& src,
                                         int num_src, const EpipolarGate& gate, int k, float max_distance = 0.f);

// The device forms, enqueued on a stream (sift_hip_match_knn_guided_batched and
// its kin): outputs laid out as matchKnnBatchedDevice's / matchKnnListBatchedDevice's,
// strides, radius, geometry and max_error as matchListEpipolarBatchedDevice's.
// A pair whose geometry record is not usable gets -1 / FLT_MAX entries and an
// empty list.
void matchKnnGuidedBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                 int src_stride, float radius, int k, int* idx, float* d2, void* stream = nullptr);
void matchKnnEpipolarBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                   int src_stride, float radius, const void* geometry, int geometry_stride_bytes,
                                   float max_error, int k, int* idx, float* d2, void* stream = nullptr);
void matchKnnListGuidedBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                     int src_stride, float radius, int k, float max_distance, DMatch* out, int* counts,
                                     void* stream = nullptr);
void matchKnnListEpipolarBatchedDevice(BatchMatcher& matcher, const std::vector<GuidedPair>& pairs, int des_stride,
                                       int src_stride, float radius, const void* geometry, int geometry_stride_bytes,
                                       float max_error, int k, float max_distance, DMatch* out, int* counts,
                                       void* stream = nullptr);

}  // namespace sift_cuda
