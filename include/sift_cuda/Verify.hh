// sift_cuda::Verifier / verifyFundamental / verifyHomography / verifyAffine: two-view
// verification of a match list (a fixed-budget RANSAC for the fundamental matrix,
// the homography, the affine map or the similarity on the device) and projectHomographyDevice, over
// sift_hip_verify_* and sift_hip_project_homography_device of
// include/sift_hip.h, where the rules are written out.
// Plain C++: no HIP headers.
#pragma once

#include <cstdint>
#include <vector>

#include "sift_cuda/Types.hh"

struct sift_hip_verifier;

namespace sift_cuda {

// sift_hip_verify_params with sift_hip_default_verify_params' defaults.
struct VerifyParams {
    int hypotheses = 1024;
    unsigned seed = 0;
    float max_error = 1.5f;  // pixels, > 0 and finite: Sampson distance (homography: transfer error)
};

// The winning hypothesis: F row-major with x_train^T F x_query = 0 (zero when
// hypothesis = -1: fewer than 8 matches or no solvable sample) and its inlier
// records, the input's, in input order.
struct TwoViewGeometry {
    float F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int hypothesis = -1;
    std::vector<DMatch> inliers;
};

// sift_hip_verify_result (device form: the record the kernels write).
struct VerifyResult {
    float F[9];
    int inliers, hypothesis, matches, valid_hypotheses;
};

// The homography's winning hypothesis: H row-major with x_train ~ H x_query,
// unit Frobenius norm (zero when hypothesis = -1: fewer than 4 matches or no
// valid sample), and its inlier records, the input's, in input order.
struct PlanarGeometry {
    float H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int hypothesis = -1;
    std::vector<DMatch> inliers;
};

// sift_hip_homography_result (device form: the record the kernels write; H is
// its first field, so its device address is what projectHomographyDevice takes).
struct HomographyResult {
    float H[9];
    int inliers, hypothesis, matches, valid_hypotheses;
};

// The affine models (sift_hip_verify_affine_*): the 6-degree-of-freedom affine map from 3-point samples
// (cv::estimateAffine2D) or the 4-degree-of-freedom similarity from 2-point samples (cv::estimateAffinePartial2D).
// Their record is the homography's, H = {a, b, tx, c, d, ty, 0, 0, 1}: projectHomographyDevice takes it as it lies.
enum class AffineModel { Affine = 0, Similarity = 1 };
using AffineResult = HomographyResult;

// sift_hip_verify_pair: one pair of a batched call -- its device position rows (nq / nt rows) and cap, its number of
// rows in the call's matches, out and mask arrays, where its rows start at the sum of the caps before it.
struct VerifyPair {
    const float* query_xy = nullptr;
    const float* train_xy = nullptr;
    int nq = 0, nt = 0;
    int cap = 0;
};

// sift_hip_camera: a skew-free pinhole camera.
struct Camera {
    float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f;
};

// sift_hip_pose_params with sift_hip_default_pose_params' defaults.
struct PoseParams {
    float max_depth = 50.f;             // > 0, +inf allowed: the far bound on both depths, in baselines
    float max_cos_parallax = 0.99998f;  // in [-1, 1]: a record in front has parallax below this cosine
};

// sift_hip_pose_result (device form: the record the kernels write): X_train = R X_query + t, R row-major, |t| = 1;
// candidate = -1 is the empty result (R and t zero).
struct PoseResult {
    float R[9];
    float t[3];
    int in_front, with_parallax;
    int counts[4];
    int candidate, fit;
};

// What the host forms return beside the record: the in-front mask (one byte per row), the points in the query camera's
// frame (3 floats per row; NaN where the record is not in front, and in the rows past the list's count) and the
// in-front records in input order.
struct RelativePose {
    PoseResult pose{};
    std::vector<uint8_t> mask;
    std::vector<float> points;
    std::vector<DMatch> inliers;
};

// sift_hip_plane_pose_result (device form): a PoseResult as it lies, then the winner's plane n^T X_query = distance
// (|normal| = 1, distance in baselines); candidate = -1 is the empty result (all zero).  Two equal top entries in
// counts: the plane has two valid poses and the first is reported (include/sift_hip.h, "Relative pose from a verified
// homography").
struct PlanePoseResult {
    float R[9];
    float t[3];
    int in_front, with_parallax;
    int counts[4];
    int candidate, fit;
    float normal[3];
    float distance;
};

// sift_hip_plane_candidate: one of the four (R, t, n, distance) of a homography's decomposition.
struct PlaneCandidate {
    float R[9];
    float t[3];
    float normal[3];
    float distance;
};

// What the plane pose host forms return: RelativePose's members with the plane pose record, and the four candidates
// (all zero when H has no decomposition).
struct PlanePose {
    PlanePoseResult pose{};
    PlaneCandidate candidates[4] = {};
    std::vector<uint8_t> mask;
    std::vector<float> points;
    std::vector<DMatch> inliers;
};

// A verifier owns the scratch of its calls; calls on one verifier must be
// ordered.  What the ABI refuses (sift_hip_verify_fundamental_device) throws
// std::invalid_argument; a failed allocation or HIP call std::runtime_error.
class Verifier {
public:
    Verifier(int max_matches, int max_hypotheses = 1024, int device = -1);
    // For the batched calls below (sift_hip_verifier_create_batched): up to max_pairs (1..64) pairs per call, whose
    // caps sum to at most max_matches (1..64 x 65536).
    Verifier(int max_matches, int max_hypotheses, int device, int max_pairs);
    ~Verifier();
    Verifier(const Verifier&) = delete;
    Verifier& operator=(const Verifier&) = delete;

    // Enqueued on `stream` (a hipStream_t, nullptr: the default stream), not synchronised; every pointer is device
    // memory.  count may be nullptr (n = cap); out, out_count and mask may be nullptr.
    void verifyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,
                      const float* train_xy, int train_stride, int nt, const VerifyParams& params, VerifyResult* result,
                      DMatch* out = nullptr, int* out_count = nullptr, uint8_t* mask = nullptr, void* stream = nullptr);
    // Synchronous; matches, count and the positions on the device, the result on the host.
    TwoViewGeometry verifyHost(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                               int nq, const float* train_xy, int train_stride, int nt, const VerifyParams& params = {});

    // The same two calls for the homography (sift_hip_verify_homography_device / _host).
    void verifyHomographyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                                int nq, const float* train_xy, int train_stride, int nt, const VerifyParams& params,
                                HomographyResult* result, DMatch* out = nullptr, int* out_count = nullptr,
                                uint8_t* mask = nullptr, void* stream = nullptr);
    PlanarGeometry verifyHomographyHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                        int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                        const VerifyParams& params = {});

    // All pairs of a batch in one pass (sift_hip_verify_fundamental_batched_device / _homography_batched_device):
    // pair p's result, out rows, out_count and mask are those of the single call on its list with the seed
    // params.seed + p.  counts (pairs.size() device ints, nullptr: every pair counts its cap), results (pairs.size()
    // device records); out, out_counts and mask may be nullptr.  Enqueued on `stream`, not synchronised.
    void verifyBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                             int query_stride, int train_stride, const VerifyParams& params, VerifyResult* results,
                             DMatch* out = nullptr, int* out_counts = nullptr, uint8_t* mask = nullptr,
                             void* stream = nullptr);
    void verifyHomographyBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                       int query_stride, int train_stride, const VerifyParams& params,
                                       HomographyResult* results, DMatch* out = nullptr, int* out_counts = nullptr,
                                       uint8_t* mask = nullptr, void* stream = nullptr);
    // Synchronous; one geometry per pair, in the pairs' order.
    std::vector<TwoViewGeometry> verifyBatchedHost(const DMatch* matches, const int* counts,
                                                   const std::vector<VerifyPair>& pairs, int query_stride,
                                                   int train_stride, const VerifyParams& params = {});
    std::vector<PlanarGeometry> verifyHomographyBatchedHost(const DMatch* matches, const int* counts,
                                                            const std::vector<VerifyPair>& pairs, int query_stride,
                                                            int train_stride, const VerifyParams& params = {});

    // The refit of a verified model on its inliers (sift_hip_refine_*; the rule: include/sift_hip.h, "Refit of the
    // verified model"): `rounds` (1..8) rounds of least-squares fit -> rescore -> accept on the list, count and
    // positions of the verify call that wrote *result and mask, both updated in place (device memory).  out,
    // out_count and accepted (the number of accepted rounds) may be nullptr.  Enqueued on `stream`, not synchronised.
    void refineDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,
                      const float* train_xy, int train_stride, int nt, float max_error, int rounds, VerifyResult* result,
                      uint8_t* mask, DMatch* out = nullptr, int* out_count = nullptr, int* accepted = nullptr,
                      void* stream = nullptr);
    void refineHomographyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                                int nq, const float* train_xy, int train_stride, int nt, float max_error, int rounds,
                                HomographyResult* result, uint8_t* mask, DMatch* out = nullptr, int* out_count = nullptr,
                                int* accepted = nullptr, void* stream = nullptr);
    // Synchronous; the list and positions on the device, `result` and `mask` (cap bytes) on the host, both updated in
    // place; inliers (nullable) receives the records of the updated mask.  Returns the number of accepted rounds.
    int refineHost(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,
                   const float* train_xy, int train_stride, int nt, float max_error, int rounds, VerifyResult& result,
                   std::vector<uint8_t>& mask, std::vector<DMatch>* inliers = nullptr);
    int refineHomographyHost(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                             int nq, const float* train_xy, int train_stride, int nt, float max_error, int rounds,
                             HomographyResult& result, std::vector<uint8_t>& mask, std::vector<DMatch>* inliers = nullptr);
    // All pairs of a batch (sift_hip_refine_*_batched_*): results, out_counts and accepted hold pairs.size() entries,
    // mask and out the caps' sum rows; pair p's bytes are the single call's.
    void refineBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                             int query_stride, int train_stride, float max_error, int rounds, VerifyResult* results,
                             uint8_t* mask, DMatch* out = nullptr, int* out_counts = nullptr, int* accepted = nullptr,
                             void* stream = nullptr);
    void refineHomographyBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                       int query_stride, int train_stride, float max_error, int rounds,
                                       HomographyResult* results, uint8_t* mask, DMatch* out = nullptr,
                                       int* out_counts = nullptr, int* accepted = nullptr, void* stream = nullptr);
    // Synchronous; results (one per pair) and mask (the caps' sum bytes) on the host, updated in place; out (nullable)
    // is resized to the caps' sum rows and out_counts (nullable) to one count per pair.  Returns the accepted rounds
    // per pair.
    std::vector<int> refineBatchedHost(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                       int query_stride, int train_stride, float max_error, int rounds,
                                       std::vector<VerifyResult>& results, std::vector<uint8_t>& mask,
                                       std::vector<DMatch>* out = nullptr, std::vector<int>* out_counts = nullptr);
    std::vector<int> refineHomographyBatchedHost(const DMatch* matches, const int* counts,
                                                 const std::vector<VerifyPair>& pairs, int query_stride, int train_stride,
                                                 float max_error, int rounds, std::vector<HomographyResult>& results,
                                                 std::vector<uint8_t>& mask, std::vector<DMatch>* out = nullptr,
                                                 std::vector<int>* out_counts = nullptr);

    // The affine map and the similarity (sift_hip_verify_affine_* / sift_hip_refine_affine_*; the rule:
    // include/sift_hip.h, "Affine and similarity verification"): the homography's verify and refine calls argument for
    // argument, with the model behind the list.  The geometry's H holds the 2 x 3 matrix over the row 0 0 1.
    void verifyAffineDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                            int nq, const float* train_xy, int train_stride, int nt, AffineModel model,
                            const VerifyParams& params, AffineResult* result, DMatch* out = nullptr,
                            int* out_count = nullptr, uint8_t* mask = nullptr, void* stream = nullptr);
    PlanarGeometry verifyAffineHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                    int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                    AffineModel model, const VerifyParams& params = {});
    void verifyAffineBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                   int query_stride, int train_stride, AffineModel model, const VerifyParams& params,
                                   AffineResult* results, DMatch* out = nullptr, int* out_counts = nullptr,
                                   uint8_t* mask = nullptr, void* stream = nullptr);
    std::vector<PlanarGeometry> verifyAffineBatchedHost(const DMatch* matches, const int* counts,
                                                        const std::vector<VerifyPair>& pairs, int query_stride,
                                                        int train_stride, AffineModel model,
                                                        const VerifyParams& params = {});
    void refineAffineDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                            int nq, const float* train_xy, int train_stride, int nt, AffineModel model, float max_error,
                            int rounds, AffineResult* result, uint8_t* mask, DMatch* out = nullptr,
                            int* out_count = nullptr, int* accepted = nullptr, void* stream = nullptr);
    int refineAffineHost(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,
                         const float* train_xy, int train_stride, int nt, AffineModel model, float max_error, int rounds,
                         AffineResult& result, std::vector<uint8_t>& mask, std::vector<DMatch>* inliers = nullptr);
    void refineAffineBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                   int query_stride, int train_stride, AffineModel model, float max_error, int rounds,
                                   AffineResult* results, uint8_t* mask, DMatch* out = nullptr, int* out_counts = nullptr,
                                   int* accepted = nullptr, void* stream = nullptr);
    std::vector<int> refineAffineBatchedHost(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                             int query_stride, int train_stride, AffineModel model, float max_error,
                                             int rounds, std::vector<AffineResult>& results, std::vector<uint8_t>& mask,
                                             std::vector<DMatch>* out = nullptr, std::vector<int>* out_counts = nullptr);

    // The essential matrix (sift_hip_verify_essential_*; the rule: include/sift_hip.h, "Essential-matrix
    // verification"): the fundamental verify calls argument for argument with the two cameras behind the list.
    // params.hypotheses counts 5-point samples; each owns ten model slots, and the record's hypothesis is the winning
    // slot 10 k + r.  The record's F is the winner's pixel-space matrix, so recoverPose*, refine* and the epipolar
    // matchers take it as it lies.  reserveEssential(max_samples), 1..4096, allocates the calls' scratch once (not
    // capturable); a call without it, or with more samples than it, throws.
    void reserveEssential(int max_samples);
    void verifyEssentialDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                               int nq, const float* train_xy, int train_stride, int nt, const Camera& cam_query,
                               const Camera& cam_train, const VerifyParams& params, VerifyResult* result,
                               DMatch* out = nullptr, int* out_count = nullptr, uint8_t* mask = nullptr,
                               void* stream = nullptr);
    TwoViewGeometry verifyEssentialHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                        int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                        const Camera& cam_query, const Camera& cam_train, const VerifyParams& params = {});
    void verifyEssentialBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                      int query_stride, int train_stride, const std::vector<Camera>& cams_query,
                                      const std::vector<Camera>& cams_train, const VerifyParams& params,
                                      VerifyResult* results, DMatch* out = nullptr, int* out_counts = nullptr,
                                      uint8_t* mask = nullptr, void* stream = nullptr);
    std::vector<TwoViewGeometry> verifyEssentialBatchedHost(const DMatch* matches, const int* counts,
                                                            const std::vector<VerifyPair>& pairs, int query_stride,
                                                            int train_stride, const std::vector<Camera>& cams_query,
                                                            const std::vector<Camera>& cams_train,
                                                            const VerifyParams& params = {});

    // The relative pose from a verified fundamental matrix (sift_hip_recover_pose_*; the rule: include/sift_hip.h,
    // "Relative pose from a verified fundamental matrix"): cv::recoverPose on the list, count and positions of the
    // verify call that wrote *result and mask (device memory, read only).  pose: a device record; mask_out (cap bytes,
    // may be mask itself), points (cap x 3 floats), out and out_count may be nullptr.  Enqueued on `stream`, not
    // synchronised, capturable.
    void recoverPoseDevice(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride, int nq,
                           const float* train_xy, int train_stride, int nt, const VerifyResult* result, const uint8_t* mask,
                           const Camera& cam_query, const Camera& cam_train, const PoseParams& params, PoseResult* pose,
                           uint8_t* mask_out = nullptr, float* points = nullptr, DMatch* out = nullptr,
                           int* out_count = nullptr, void* stream = nullptr);
    // Synchronous; the list and positions on the device, `result` and `mask` (cap bytes) on the host.
    RelativePose recoverPoseHost(const DMatch* matches, const int* count, int cap, const float* query_xy, int query_stride,
                                 int nq, const float* train_xy, int train_stride, int nt, const VerifyResult& result,
                                 const std::vector<uint8_t>& mask, const Camera& cam_query, const Camera& cam_train,
                                 const PoseParams& params = {});
    // All pairs of a batch: results and poses hold pairs.size() records, cams_query and cams_train pairs.size() cameras,
    // mask, mask_out and out the caps' sum rows, points three floats per row; pair p's bytes are the single call's.
    void recoverPoseBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                  int query_stride, int train_stride, const VerifyResult* results, const uint8_t* mask,
                                  const std::vector<Camera>& cams_query, const std::vector<Camera>& cams_train,
                                  const PoseParams& params, PoseResult* poses, uint8_t* mask_out = nullptr,
                                  float* points = nullptr, DMatch* out = nullptr, int* out_counts = nullptr,
                                  void* stream = nullptr);
    // Synchronous; one RelativePose per pair, in the pairs' order.
    std::vector<RelativePose> recoverPoseBatchedHost(const DMatch* matches, const int* counts,
                                                     const std::vector<VerifyPair>& pairs, int query_stride,
                                                     int train_stride, const std::vector<VerifyResult>& results,
                                                     const std::vector<uint8_t>& mask,
                                                     const std::vector<Camera>& cams_query,
                                                     const std::vector<Camera>& cams_train, const PoseParams& params = {});

    // The relative pose from a verified homography (sift_hip_recover_pose_homography_*; the rule: include/sift_hip.h,
    // "Relative pose from a verified homography"): argument for argument the four calls above on what the homography
    // verify and refine calls wrote, with the plane pose record and the trailing candidates (4 device records per
    // pair, nullable).
    void recoverPoseHomographyDevice(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                     int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                     const HomographyResult* result, const uint8_t* mask, const Camera& cam_query,
                                     const Camera& cam_train, const PoseParams& params, PlanePoseResult* pose,
                                     uint8_t* mask_out = nullptr, float* points = nullptr, DMatch* out = nullptr,
                                     int* out_count = nullptr, PlaneCandidate* candidates = nullptr,
                                     void* stream = nullptr);
    PlanePose recoverPoseHomographyHost(const DMatch* matches, const int* count, int cap, const float* query_xy,
                                        int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                                        const HomographyResult& result, const std::vector<uint8_t>& mask,
                                        const Camera& cam_query, const Camera& cam_train, const PoseParams& params = {});
    void recoverPoseHomographyBatchedDevice(const DMatch* matches, const int* counts, const std::vector<VerifyPair>& pairs,
                                            int query_stride, int train_stride, const HomographyResult* results,
                                            const uint8_t* mask, const std::vector<Camera>& cams_query,
                                            const std::vector<Camera>& cams_train, const PoseParams& params,
                                            PlanePoseResult* poses, uint8_t* mask_out = nullptr, float* points = nullptr,
                                            DMatch* out = nullptr, int* out_counts = nullptr,
                                            PlaneCandidate* candidates = nullptr, void* stream = nullptr);
    std::vector<PlanePose> recoverPoseHomographyBatchedHost(const DMatch* matches, const int* counts,
                                                            const std::vector<VerifyPair>& pairs, int query_stride,
                                                            int train_stride, const std::vector<HomographyResult>& results,
                                                            const std::vector<uint8_t>& mask,
                                                            const std::vector<Camera>& cams_query,
                                                            const std::vector<Camera>& cams_train,
                                                            const PoseParams& params = {});

    sift_hip_verifier* handle() const { return m_handle; }

private:
    sift_hip_verifier* m_handle = nullptr;
};

// One shot: uploads the list and verifies it.  query_xy / train_xy: device position rows (x, y first; nq / nt rows of
// query_stride / train_stride floats -- a Detector's device_kpts.data() with stride 3).
TwoViewGeometry verifyFundamental(const std::vector<DMatch>& matches, const float* query_xy, int nq,
                                  const float* train_xy, int nt, const VerifyParams& params = {}, int query_stride = 3,
                                  int train_stride = 3);

// The same one shot for the homography.
PlanarGeometry verifyHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const VerifyParams& params = {}, int query_stride = 3, int train_stride = 3);

// The one shots followed by `refit` refit rounds on the device (Verifier::refineHost): the geometry is then the
// least-squares model of its inliers (F of rank 2) whenever that model counts at least as many.  refit = 0: the calls
// above, byte for byte.
TwoViewGeometry verifyFundamental(const std::vector<DMatch>& matches, const float* query_xy, int nq,
                                  const float* train_xy, int nt, const VerifyParams& params, int query_stride,
                                  int train_stride, int refit);
PlanarGeometry verifyHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const VerifyParams& params, int query_stride, int train_stride, int refit);

// The one shot for the affine map or the similarity, with `refit` refit rounds (0: the minimal-sample winner): the
// matrix in H, over the row 0 0 1.
PlanarGeometry verifyAffine(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                            int nt, AffineModel model, const VerifyParams& params = {}, int query_stride = 3,
                            int train_stride = 3, int refit = 0);

// The one shot for the essential matrix (cv::findEssentialMat): the geometry's F is the pixel-space matrix of the
// winning slot, E = Kt^T F Kq.  `refit` rounds of Verifier::refineHost follow -- the 8-point least-squares F, not an
// essential refit; skip it on near-planar scenes.
TwoViewGeometry verifyEssential(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const Camera& cam_query, const Camera& cam_train, const VerifyParams& params = {},
                                int query_stride = 3, int train_stride = 3, int refit = 0);

// The all-in-one beside verifyFundamental: uploads the list and recovers the pose of a verified F (9 floats, row-major,
// x_train^T F x_query = 0) over the records `mask` marks (empty: every record).
RelativePose recoverPose(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy, int nt,
                         const float (&F)[9], const std::vector<uint8_t>& mask, const Camera& cam_query,
                         const Camera& cam_train, const PoseParams& params = {}, int query_stride = 3,
                         int train_stride = 3);

// The all-in-one beside verifyHomography: uploads the list and recovers the pose and the plane of a verified H (9
// floats, row-major, x_train ~ H x_query, signed as verifyHomography signs it) over the records `mask` marks (empty:
// every record).
PlanePose recoverPoseHomography(const std::vector<DMatch>& matches, const float* query_xy, int nq, const float* train_xy,
                                int nt, const float (&H)[9], const std::vector<uint8_t>& mask, const Camera& cam_query,
                                const Camera& cam_train, const PoseParams& params = {}, int query_stride = 3,
                                int train_stride = 3);

// Enqueued on `stream`, not synchronised (sift_hip_project_homography_device): row i of out_xy = row i of xy carried
// over by H, NaN where it lands behind the camera.  H: 9 floats of device memory (a HomographyResult's address); xy /
// out_xy: n device rows of stride / out_stride floats, x and y first; out_xy may be xy with equal strides.
void projectHomographyDevice(const float* H, const float* xy, int stride, int n, float* out_xy, int out_stride = 2,
                             void* stream = nullptr);

// sift_hip_project_set: one set of a batched projection.
struct ProjectSet {
    const float* xy = nullptr;
    int n = 0;
    float* out_xy = nullptr;
};

// All sets in one launch (sift_hip_project_homography_batched_device): set p goes through the 9 device floats at
// geometry + p * geometry_stride_bytes -- sizeof(HomographyResult) for verifyHomographyBatchedDevice's results as they
// lie -- and gives what projectHomographyDevice gives on it.  Enqueued on `stream`, not synchronised.
void projectHomographyBatchedDevice(const void* geometry, int geometry_stride_bytes, const std::vector<ProjectSet>& sets,
                                    int stride, int out_stride = 2, void* stream = nullptr);

}  // namespace sift_cuda
