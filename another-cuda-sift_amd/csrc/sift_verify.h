// Two-view verifier launch interface (verify.hip) used by verify_api.hip's C
// ABI (sift_hip_verify_*, sift_hip_project_homography_device; the rules are in
// include/sift_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sift_match.h"

namespace sift_amd {

constexpr int kVerifyMaxMatches = 65536;
constexpr int kVerifyMaxHypotheses = 4096;

// The match list as the kernels take it: `cap` records, of which
// n = min(max(*count, 0), cap) count (count == nullptr: n = cap), and the
// position rows the records index (row i of a set at xy[i * stride + {0, 1}],
// rows [0, nq) / [0, nt) exist).
struct VerifyInput {
    const MatchRecord* matches;
    const int* count;
    int cap;
    const float* qxy;
    const float* txy;
    int qstride, tstride;
    int nq, nt;
};

// A batch of lists as the batched kernels take it, by value (as MatchBatch is):
// pair p's `cap` rows of matches, out, mask and of the gathered points start at
// row0 = sum of the caps before it; its n comes from counts[p] (counts ==
// nullptr: n = cap); its positions are its own, the strides the call's.
constexpr int kVerifyMaxPairs = kMaxMatchPairs;
struct VerifyBatchPair {
    const float* qxy;
    const float* txy;
    int row0, cap;
    int nq, nt;
};
struct VerifyBatch {
    VerifyBatchPair pair[kVerifyMaxPairs];
    const MatchRecord* matches;
    const int* counts;
    int qstride, tstride;
    int P;
    int rows, max_cap;  // the sum and the largest of the caps
};

// sift_hip_verify_result's layout.
struct VerifyResult {
    float F[9];
    int inliers, hypothesis, matches, valid_hypotheses;
};
static_assert(sizeof(VerifyResult) == 52, "sift_hip_verify_result layout");

// The launchers are templates over the list, instantiated for VerifyInput and VerifyBatch (verify.hip, refit.hip).  A
// batch runs the same step for all its P pairs in one launch, pair p = blockIdx.y on its own slices -- points, mask
// and out rows at row0[p]; samples at m K p (m = 8 / 4), models at 9 K p, valid flags and counts at K p; its result,
// candidate, out_count and accepted at p -- with the seed `seed + p` (wrapping).  A workgroup serves one pair.
inline int list_pairs(const VerifyInput&) { return 1; }
inline int list_pairs(const VerifyBatch& b) { return b.P; }
inline int list_extent(const VerifyInput& in) { return in.cap; }  // the rows the gather's grid covers
inline int list_extent(const VerifyBatch& b) { return b.max_cap; }

// k_verify_gather: match j -> pts[j] = (qx, qy, tx, ty), NaN x 4 for a record
// with an index outside its position array; j in [n, cap) is not written.
template <class List>
void launch_verify_gather(const List& list, float4* pts, hipStream_t s);

// The model a verify call fits: it selects the hypothesis kernel and the
// predicate the score and select kernels are instantiated with.
// Affine (6 degrees of freedom, 3-point samples) and Similarity (4, 2-point samples) store their 2 x 3 matrix as
// the 3 x 3 {m0 .. m5, 0, 0, 1} in the homography's record and share one predicate (AffinePass).
// Essential (essential.hip): 5-point samples under two cameras, ten model slots per sample, each a pixel-space
// fundamental matrix -- the score and the select then run over 10 K slots with the fundamental matrix's predicate.
enum class VerifyModel { Fundamental = 1, Homography = 2, Affine = 3, Similarity = 4, Essential = 5 };
constexpr bool is_affine(VerifyModel m) { return m == VerifyModel::Affine || m == VerifyModel::Similarity; }
// The matches a hypothesis of the model draws: the stride of its rows in the samples scratch.
constexpr int sample_size(VerifyModel m) {
    return m == VerifyModel::Fundamental  ? 8
           : m == VerifyModel::Homography ? 4
           : m == VerifyModel::Affine     ? 3
           : m == VerifyModel::Essential  ? 5
                                          : 2;
}
// The model slots a sample owns: the rows of the model, valid and count scratch per sample.
constexpr int kEssentialSlots = 10;
constexpr int model_slots(VerifyModel m) { return m == VerifyModel::Essential ? kEssentialSlots : 1; }

// k_verify_hypotheses / k_verify_hypotheses_h / k_verify_hypotheses_a: hypothesis k in [0, K) draws its
// m matches (m = 8 for the fundamental matrix, 4 for the homography, 3 for the affine map, 2 for the similarity;
// samples[m k ..], -1 when n < m) and solves them: F[9 k ..] and valid[k] (an
// invalid hypothesis has F all zero).  e2 = max_error^2 serves the homography's
// own-sample rule; the other kernels do not read it.
template <class List>
void launch_verify_hypotheses(VerifyModel model, const List& list, const float4* pts, int K, unsigned seed, float e2,
                              int* samples, float* F, int* valid, hipStream_t s);

// k_verify_score: counts[k] = the matches j < n that pass the model's predicate
// (Sampson distance / forward transfer error / affine transfer error) under F[9 k ..] with
// e2 = max_error^2; 0 where valid (nullable) says the hypothesis is invalid.
template <class List>
void launch_verify_score(VerifyModel model, const List& list, const float4* pts, const float* F, const int* valid, int K,
                         float e2, int* counts, hipStream_t s);

// k_verify_select: the winner (most inliers among the valid, ties to the lowest
// k) into *result (sift_hip_homography_result has the same layout), its inlier
// mask (cap bytes, nullable), the inlier records in input order (out, nullable)
// and their number (out_count, nullable).  A batch: P results and out_counts, batch.rows rows of out and mask.
template <class List>
void launch_verify_select(VerifyModel model, const List& list, const float4* pts, const float* F, const int* valid,
                          const int* counts, int K, float e2, VerifyResult* result, MatchRecord* out, int* out_count,
                          uint8_t* mask, hipStream_t s);

// k_verify_hypotheses_e (essential.hip): sample k in [0, K) draws 5 matches (samples[5 k ..], -1 when n < 5), turns
// them into calibrated rays under the pair's two cameras and solves the 5-point problem: up to ten real roots, root r
// in ascending order in slot 10 k + r as the pixel-space F = Kt^-T E Kq^-1 of unit norm (F[9 (10 k + r) ..]) with
// valid[10 k + r]; every other slot is zero and invalid.  A batch: pair p's samples at 5 K p, its slots at 10 K p,
// and its cameras go through cam_scratch (2 kVerifyMaxPairs records, device; a single call does not touch it).
struct PoseCameras;
struct PoseCamera;
template <class List>
void launch_verify_hypotheses_e(const List& list, const float4* pts, int K, unsigned seed, const PoseCameras& cams,
                                PoseCamera* cam_scratch, int* samples, float* F, int* valid, hipStream_t s);

// The refit of a verified model on its inliers (refit.hip; sift_hip_refine_*, the rule is in include/sift_hip.h).
// One round is two launches, both with one workgroup per pair:
// k_refit_fit: the least-squares model of the records j < n with mask[j] != 0 and finite gathered points, under the
//   current record *result, into the verifier's scratch record *cand (valid = 0: no refit, the model all zero).
// k_refit_accept: the candidate rescored over the n records with the model's predicate; when it is valid and counts
//   at least result->inliers records, result's model and inliers and mask[0, n) become the candidate's.  out
//   (nullable) then receives the records of the mask as it stands, in input order, and out_count (nullable) their
//   number; *accepted (nullable) is set to (first_round ? 0 : *accepted) + 1 on an accepted round.
struct RefitCandidate {
    float m[9];
    int valid;
};
template <class List>
void launch_refit_fit(VerifyModel model, const List& list, const float4* pts, const uint8_t* mask,
                      const VerifyResult* result, RefitCandidate* cand, hipStream_t s);
template <class List>
void launch_refit_accept(VerifyModel model, const List& list, const float4* pts, const RefitCandidate* cand, float e2,
                         VerifyResult* result, uint8_t* mask, MatchRecord* out, int* out_count, int* accepted,
                         bool first_round, hipStream_t s);

// The relative pose from a verified fundamental matrix (pose.hip; sift_hip_recover_pose_*, the rule is in
// include/sift_hip.h).  Two launches on the gathered list:
// k_pose_decompose: one wave per pair.  E = Kt^T F Kq of the pair's record under its two cameras, the eigenvectors of
//   E^T E by the refit's Jacobi routine, and the two rotations and the translation of the four candidates into the
//   verifier's scratch record cand[p] (usable = 0: an empty or unusable record, or an E of rank <= 1).
// k_pose_select: one workgroup per pair.  The fit records' depths under the four candidates, their counts, the winner
//   into pose[p]; then mask_out (cap bytes, may be the mask itself), the points (3 floats per row j < n) and the
//   in-front records in input order (out, out_count), each nullable.
struct PoseResult {  // sift_hip_pose_result's layout
    float R[9], t[3];
    int in_front, with_parallax, counts[4], candidate, fit;
};
static_assert(sizeof(PoseResult) == 80, "sift_hip_pose_result layout");
struct PoseCamera {
    float fx, fy, cx, cy;
};
struct PoseCameras {  // by value, as VerifyBatch is: pair p's query and train camera
    PoseCamera q[kVerifyMaxPairs], t[kVerifyMaxPairs];
};
struct PoseCandidates {  // k_pose_select reads the 29 leading doubles as an array
    double R[2][9];  // R1, R2 row-major; the candidates are (R1, t), (R2, t), (R1, -t), (R2, -t)
    double t[3];
    double kq[4], kt[4];  // the cameras' fx, fy, cx, cy
    int usable, pad;
};
static_assert(offsetof(PoseCandidates, usable) == 29 * sizeof(double), "k_pose_select's view of the record");
void launch_pose_decompose(const PoseCameras& cams, int P, const VerifyResult* result, PoseCandidates* cand,
                           hipStream_t s);
template <class List>
void launch_pose_select(const List& list, const float4* pts, const uint8_t* mask, const PoseCandidates* cand,
                        float max_depth, float max_cos_parallax, PoseResult* pose, uint8_t* mask_out, float* points,
                        MatchRecord* out, int* out_count, hipStream_t s);

// The relative pose from a verified homography (pose_homography.hip; sift_hip_recover_pose_homography_*, the rule is
// in include/sift_hip.h).  The same two launches on the gathered list:
// k_plane_decompose: one wave per pair.  A = Kt^-1 H Kq of the pair's record under its two cameras, the eigenvectors of
//   A^T A by the refit's Jacobi routine, and the two (R, t, N, distance) of the four candidates into the verifier's
//   scratch record cand[p] (usable = 0: an empty or unusable record, or an A without a decomposition); the four
//   candidates rounded to float32 into candidates[4 p ..] when that is not null (all zero when usable = 0).
// k_plane_select: one workgroup per pair.  k_pose_select with a translation per rotation and w > 0 under H in the fit
//   test; the winner's plane follows its pose in pose[p].
struct PlanePoseResult {  // sift_hip_plane_pose_result's layout: a PoseResult, then the plane
    PoseResult pose;
    float normal[3], distance;
};
static_assert(sizeof(PlanePoseResult) == 96, "sift_hip_plane_pose_result layout");
struct PlaneCandidate {  // sift_hip_plane_candidate's layout
    float R[9], t[3], normal[3], distance;
};
static_assert(sizeof(PlaneCandidate) == 64, "sift_hip_plane_candidate layout");
struct PlaneCandidates {  // k_plane_select reads the 43 leading doubles as an array
    double R[2][9];  // R+, R- row-major; the candidates are (R+, t+, N+), (R-, t-, N-), (R+, -t+, -N+), (R-, -t-, -N-)
    double t[2][3];
    double kq[4], kt[4];  // the cameras' fx, fy, cx, cy
    double h3[3];         // the third row of H as the record holds it: w = (h3[0] qx + h3[1] qy) + h3[2]
    double N[2][3];
    double distance[2];
    int usable, pad;
};
static_assert(offsetof(PlaneCandidates, usable) == 43 * sizeof(double), "k_plane_select's view of the record");
void launch_plane_decompose(const PoseCameras& cams, int P, const VerifyResult* result, PlaneCandidates* cand,
                            PlaneCandidate* candidates, hipStream_t s);
template <class List>
void launch_plane_select(const List& list, const float4* pts, const uint8_t* mask, const PlaneCandidates* cand,
                         float max_depth, float max_cos_parallax, PlanePoseResult* pose, uint8_t* mask_out, float* points,
                         MatchRecord* out, int* out_count, hipStream_t s);

// k_project_homography: out[i * out_stride + {0, 1}] = row i of xy (n rows of
// `stride` floats) through the device matrix H, NaN x 2 where w is not > 0.
void launch_project_homography(const float* H, const float* xy, int stride, int n, float* out, int out_stride,
                               hipStream_t s);

// k_project_homography_batch: the same for P sets in one launch, pair p =
// blockIdx.y with the matrix at geometry + p * geometry_stride bytes (device)
// and its own rows; the strides are the call's.  By value, as VerifyBatch is.
struct ProjectPair {
    const float* xy;
    float* out;
    int n;
};
struct ProjectBatch {
    ProjectPair pair[kVerifyMaxPairs];
    int P, max_n;
};
void launch_project_homography_batched(const void* geometry, int geometry_stride, const ProjectBatch& batch, int stride,
                                       int out_stride, hipStream_t s);

}  // namespace sift_amd
