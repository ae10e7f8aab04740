// Verifier handle (sift_hip_verifier_*, sift_hip_verify_*, sift_hip_score_*) and
// sift_hip_project_homography_device of libsift_hip.so; the kernels are verify.hip.  The handle owns every scratch
// array from creation on, so a device call only launches kernels (capturable).  A handle from
// sift_hip_verifier_create_batched holds the scratch of up to maxP pairs per call (sift_hip_verify_*_batched_*): maxM
// then bounds a call's rows over all its pairs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

#include "detector_state.h"
#include "sift_verify.h"

struct sift_hip_verifier {
    int device = 0;
    int maxM = 0, maxK = 0, maxP = 0;
    float4* dPts = nullptr;      // the gathered matches (qx, qy, tx, ty), maxM rows
    int* dSamples = nullptr;     // 8 per hypothesis (the homography uses 4, the affine map 3, the similarity 2), maxP x
                                 // maxK hypotheses as are dF .. dCounts
    float* dF = nullptr;         // 9 per hypothesis (F, H, or the affine matrix over 0 0 1)
    int* dValid = nullptr;
    int* dCounts = nullptr;
    // the outputs of sift_hip_verify_fundamental_host / _homography_host and their batched forms
    VerifyResult* dResult = nullptr;  // maxP records
    MatchRecord* dOut = nullptr;
    uint8_t* dMask = nullptr;
    RefitCandidate* dCand = nullptr;  // the refit's candidate model per pair (sift_hip_refine_*), maxP records
    int* dRefineInts = nullptr;       // sift_hip_refine_*_host: maxP out counts, then maxP accepted rounds
    PoseCandidates* dPoseCand = nullptr;  // the pose calls' candidates per pair (sift_hip_recover_pose_*), maxP records
    PoseResult* dPose = nullptr;          // sift_hip_recover_pose_*_host: maxP pose records and maxM x 3 point floats
    float* dPoints = nullptr;
    PlaneCandidates* dPlaneCand = nullptr;  // the plane pose calls' candidates per pair (sift_hip_recover_pose_homography_*)
    PlanePoseResult* dPlanePose = nullptr;  // their host forms: maxP pose records and 4 x maxP candidates
    PlaneCandidate* dPlaneOut = nullptr;
    // The essential calls' hypothesis scratch (sift_hip_verifier_reserve_essential): maxP x essK samples of 5 indices
    // and ten model slots each.  essK = 0: not reserved.
    int essK = 0;
    int* dEssSamples = nullptr;
    float* dEssF = nullptr;
    int* dEssValid = nullptr;
    int* dEssCounts = nullptr;
    PoseCamera* dEssCams = nullptr;  // a batch's cameras on their way to the hypothesis kernel
    int lastK = 0;               // hypotheses of the last verify call (sift_hip_verify_*hypotheses_host)
    int lastModel = 0;           // its VerifyModel, 0: none
    bool lastBatch = false;      // it was a batched call (the getters read one pair's scratch layout)
    ~sift_hip_verifier() {
        (void)hipSetDevice(device);
        for (void* p : {(void*)dPts, (void*)dSamples, (void*)dF, (void*)dValid, (void*)dCounts, (void*)dResult,
                        (void*)dOut, (void*)dMask, (void*)dCand, (void*)dRefineInts, (void*)dPoseCand, (void*)dPose,
                        (void*)dPoints, (void*)dPlaneCand, (void*)dPlanePose, (void*)dPlaneOut, (void*)dEssSamples,
                        (void*)dEssF, (void*)dEssValid, (void*)dEssCounts, (void*)dEssCams})
            if (p) (void)hipFree(p);
    }
};

static_assert(sizeof(sift_hip_verify_result) == sizeof(VerifyResult), "the result record is written by the kernel");
static_assert(sizeof(sift_hip_homography_result) == sizeof(VerifyResult) &&
                  offsetof(sift_hip_homography_result, inliers) == offsetof(VerifyResult, inliers),
              "both models' result records share the kernel's layout");
static_assert(sizeof(sift_hip_affine_result) == sizeof(VerifyResult), "the affine models reuse the homography's record");
static_assert(sizeof(sift_hip_pose_result) == sizeof(PoseResult) &&
                  offsetof(sift_hip_pose_result, candidate) == offsetof(PoseResult, candidate),
              "the pose record is written by the kernel");
static_assert(sizeof(sift_hip_plane_pose_result) == sizeof(PlanePoseResult) &&
                  offsetof(sift_hip_plane_pose_result, normal) == offsetof(PlanePoseResult, normal) &&
                  sizeof(sift_hip_plane_candidate) == sizeof(PlaneCandidate),
              "the plane pose record and the candidates are written by the kernels");
static_assert(sizeof(sift_hip_camera) == sizeof(PoseCamera), "the cameras go to the kernel as they are");

namespace {

constexpr int kRefineMaxRounds = 8;

// One call of the verifier as every entry point hands it down: the operation, the list(s) and the outputs.  A
// single-pair entry point describes its list as a one-pair table (row0 = 0) and sets `single`: the same rules and the
// same host path then serve it, and only the launches differ -- they take the 72-byte VerifyInput, not the batch table.
enum class Op { Verify, Score, Refine, Pose };
struct Call {
    Op op;
    VerifyModel model;
    bool host;    // the synchronous form: result, out, mask, out_counts and accepted are host memory
    bool single;  // came in through a single-pair entry point
    const sift_hip_dmatch* matches;
    const int* counts;
    int P;
    const sift_hip_verify_pair* pairs;
    int qstride, tstride;
    const sift_hip_verify_params* params;  // verify: the caller's; score and refine: the entry point's (K, -, max_error)
    void* result;                          // P records of either model (they share a layout)
    sift_hip_dmatch* out;
    int* out_counts;
    uint8_t* mask;
    int rounds;  // refine
    int* accepted;
    const float* models;  // score: the K models to count under, and their counts
    int* scores;
    const sift_hip_camera* cams_q;  // pose: P cameras per side (host memory), the thresholds, the P pose records and
    const sift_hip_camera* cams_t;  // the optional mask and points; `result` and `mask` are the inputs.  An essential
                                    // verify call carries the cameras too.
    const sift_hip_pose_params* pose_params;
    void* pose;
    uint8_t* mask_out;
    float* points;
    void* candidates;  // plane pose: 4 P candidates, nullable
    void* stream;
};

Call make_call(Op op, VerifyModel model, bool host, const sift_hip_dmatch* matches, int qstride, int tstride) {
    Call c{};
    c.op = op, c.model = model, c.host = host;
    c.matches = matches, c.qstride = qstride, c.tstride = tstride;
    return c;
}

// The argument rules of every call, each stated once, in the order include/sift_hip.h documents: what can be judged
// without the handle first (nothing is dereferenced), then the handle's limits.  Nothing is launched or written on a
// refusal.  On success `b` is the pair table the kernels take.
int check(const sift_hip_verifier* v, const Call& c, VerifyBatch& b) {
    const auto refuse = [](const std::string& msg) { return fail(SIFT_HIP_ERR_INVALID, msg); };
    const bool refine = c.op == Op::Refine, pose = c.op == Op::Pose;
    const bool essential = c.op == Op::Verify && c.model == VerifyModel::Essential;
    if (!v) return refuse("null verifier");
    if ((int)c.model == 0) return refuse("verify: model must be SIFT_HIP_MODEL_AFFINE or SIFT_HIP_MODEL_SIMILARITY");
    if (!c.pairs) return refuse("verify: null pairs");
    if (c.op == Op::Score) {
        if (!c.models || !c.scores)
            return refuse(c.model == VerifyModel::Homography ? "verify: null H or counts"
                          : is_affine(c.model)               ? "verify: null A or counts"
                                                             : "verify: null F or counts");
    } else if (!pose && (!c.params || !c.result)) {
        return refuse(refine && c.single ? "refine: null result" : "verify: null params or result");
    }
    if (c.P < 1 || c.P > kVerifyMaxPairs) return refuse("verify: pairs outside 1.." + std::to_string(kVerifyMaxPairs));
    if (c.qstride < 2 || c.tstride < 2) return refuse("verify: a position stride below 2 floats");
    int rows = 0, max_cap = 0;  // P x 65536 fits
    for (int p = 0; p < c.P; p++) {
        const sift_hip_verify_pair& e = c.pairs[p];
        const auto at = [&] { return c.single ? std::string() : " (pair " + std::to_string(p) + ")"; };
        if (e.cap < 0 || e.cap > kVerifyMaxMatches)
            return refuse("verify: cap must lie in 0.." + std::to_string(kVerifyMaxMatches) + at());
        if (e.nq < 0 || e.nt < 0) return refuse("verify: a negative position row count" + at());
        if (e.cap > 0 && (!e.query_xy || !e.train_xy)) return refuse("verify: null position pointer" + at());
        b.pair[p] = VerifyBatchPair{e.query_xy, e.train_xy, rows, e.cap, e.nq, e.nt};
        rows += e.cap;
        max_cap = std::max(max_cap, e.cap);
    }
    if (rows > 0 && !c.matches) return refuse("verify: null matches");
    if (pose || essential) {  // the cameras' rules, the pose calls' and the essential calls' alike
        const std::string who = pose ? "pose" : "verify";
        if (!c.cams_q || !c.cams_t) return refuse(who + ": null camera pointer");
        for (int p = 0; p < c.P; p++)
            for (const sift_hip_camera* k : {c.cams_q + p, c.cams_t + p}) {
                const auto at = [&] { return c.single ? std::string() : " (pair " + std::to_string(p) + ")"; };
                if (!(k->fx > 0.f) || !(k->fy > 0.f) || !std::isfinite(k->fx) || !std::isfinite(k->fy))
                    return refuse(who + ": fx and fy must be > 0 and finite" + at());
                if (!std::isfinite(k->cx) || !std::isfinite(k->cy))
                    return refuse(who + ": cx and cy must be finite" + at());
            }
    }
    if (pose) {  // the pose calls' own rules stand where max_error stands for the others
        if (!c.pose_params || !c.result || !c.pose) return refuse("pose: null params or result");
        if (!(c.pose_params->max_depth > 0.f)) return refuse("pose: max_depth must be > 0");
        if (!(c.pose_params->max_cos_parallax >= -1.f && c.pose_params->max_cos_parallax <= 1.f))
            return refuse("pose: max_cos_parallax must lie in [-1, 1]");
        if (rows > 0 && !c.mask) return refuse("pose: null mask (the mask is the fit set)");
    } else if (!(c.params->max_error > 0.f) || !std::isfinite(c.params->max_error)) {
        return refuse("verify: max_error must be > 0 and finite");
    }
    const uintptr_t ob = (uintptr_t)c.out, mb = (uintptr_t)c.matches, bytes = sizeof(sift_hip_dmatch) * (size_t)rows;
    if (!c.host && c.out && rows > 0 && ob < mb + bytes && mb < ob + bytes) return refuse("verify: out aliases matches");
    if (refine && rows > 0 && !c.mask) return refuse("refine: null mask (the mask is the fit set)");
    if (refine && (c.rounds < 1 || c.rounds > kRefineMaxRounds))
        return refuse("refine: rounds must lie in 1.." + std::to_string(kRefineMaxRounds));
    const int K = pose ? 1 : c.params->hypotheses;  // a pose call draws nothing
    if (K < 1 || K > kVerifyMaxHypotheses || (!essential && K > v->maxK))
        return refuse("verify: hypotheses outside 1..max_hypotheses");
    if (c.P > v->maxP) return refuse("verify: more pairs than the verifier's max_pairs");
    if (rows > v->maxM)
        return refuse(c.single ? "verify: cap exceeds the verifier's max_matches"
                               : "verify: the caps' sum exceeds the verifier's max_matches");
    // An essential call draws its samples into the scratch of sift_hip_verifier_reserve_essential: a matter of the
    // handle's state, judged when the arguments themselves are in order.
    if (essential && v->essK == 0)
        return fail(SIFT_HIP_ERR_STATE, "verify: no essential scratch (sift_hip_verifier_reserve_essential)");
    if (essential && K > v->essK) return fail(SIFT_HIP_ERR_STATE, "verify: hypotheses above the essential reservation");
    if (!c.single) std::fill(b.pair + c.P, b.pair + kVerifyMaxPairs, VerifyBatchPair{});  // the table goes by value
    b.matches = reinterpret_cast<const MatchRecord*>(c.matches);
    b.counts = c.counts;
    b.qstride = c.qstride, b.tstride = c.tstride;
    b.P = c.P, b.rows = rows, b.max_cap = max_cap;
    return SIFT_HIP_OK;
}

// Where a call's launches write: the caller's device memory, or for a host form the handle's own.
struct Outputs {
    VerifyResult* result;
    MatchRecord* out;
    int* out_counts;
    uint8_t* mask;
    int* accepted;
    hipStream_t stream;
    // the pose calls' outputs; result and mask are then read only
    void* pose = nullptr;  // PoseResult records, or PlanePoseResult records for the homography
    uint8_t* mask_out = nullptr;
    float* points = nullptr;
    PlaneCandidate* candidates = nullptr;  // the homography's four per pair
};

// The cameras of a pose or an essential call as the kernels take them, by value.
PoseCameras cameras_of(const Call& c) {
    PoseCameras cams{};
    for (int p = 0; p < c.P; p++) {
        cams.q[p] = PoseCamera{c.cams_q[p].fx, c.cams_q[p].fy, c.cams_q[p].cx, c.cams_q[p].cy};
        cams.t[p] = PoseCamera{c.cams_t[p].fx, c.cams_t[p].fy, c.cams_t[p].cx, c.cams_t[p].cy};
    }
    return cams;
}

// The runners, one per operation, over the list type (VerifyInput or VerifyBatch): one launch per step for all the
// list's pairs.  Every index stays inside the handle's scratch: rows <= maxM, P <= maxP and K <= maxK (an essential
// call: K <= essK, in its own scratch) were checked.
template <class List>
int verify_on(sift_hip_verifier* v, const Call& c, const List& list, const Outputs& o) {
    const int K = c.params->hypotheses;
    const float e2 = c.params->max_error * c.params->max_error;
    launch_verify_gather(list, v->dPts, o.stream);
    if (c.model == VerifyModel::Essential) {  // K samples; their 10 K model slots are scored and selected as F
        const int S = kEssentialSlots * K;
        launch_verify_hypotheses_e(list, v->dPts, K, c.params->seed, cameras_of(c), v->dEssCams, v->dEssSamples,
                                   v->dEssF, v->dEssValid, o.stream);
        launch_verify_score(c.model, list, v->dPts, v->dEssF, v->dEssValid, S, e2, v->dEssCounts, o.stream);
        launch_verify_select(c.model, list, v->dPts, v->dEssF, v->dEssValid, v->dEssCounts, S, e2, o.result, o.out,
                             o.out_counts, o.mask, o.stream);
    } else {
        launch_verify_hypotheses(c.model, list, v->dPts, K, c.params->seed, e2, v->dSamples, v->dF, v->dValid, o.stream);
        launch_verify_score(c.model, list, v->dPts, v->dF, v->dValid, K, e2, v->dCounts, o.stream);
        launch_verify_select(c.model, list, v->dPts, v->dF, v->dValid, v->dCounts, K, e2, o.result, o.out, o.out_counts,
                             o.mask, o.stream);
    }
    HIPCHK(hipGetLastError());
    v->lastK = K;
    v->lastModel = (int)c.model;
    v->lastBatch = !c.single;
    return SIFT_HIP_OK;
}

template <class List>
int score_on(sift_hip_verifier* v, const Call& c, const List& list, const Outputs& o) {
    launch_verify_gather(list, v->dPts, o.stream);
    launch_verify_score(c.model, list, v->dPts, c.models, nullptr, c.params->hypotheses,
                        c.params->max_error * c.params->max_error, c.scores, o.stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// `rounds` rounds of fit -> rescore -> accept on the gathered list; out is written by the last round only.  The
// verifier's hypothesis scratch is not touched.
template <class List>
int refine_on(sift_hip_verifier* v, const Call& c, const List& list, const Outputs& o) {
    const float e2 = c.params->max_error * c.params->max_error;
    launch_verify_gather(list, v->dPts, o.stream);
    for (int r = 0; r < c.rounds; r++) {
        const bool last = r == c.rounds - 1;
        launch_refit_fit(c.model, list, v->dPts, o.mask, o.result, v->dCand, o.stream);
        launch_refit_accept(c.model, list, v->dPts, v->dCand, e2, o.result, o.mask, last ? o.out : nullptr,
                            last ? o.out_counts : nullptr, o.accepted, r == 0, o.stream);
    }
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// The gather, the candidates of every pair's record under its cameras, and the counts, winner and outputs.  The
// cameras travel by value; the verifier's hypothesis scratch is not touched.
template <class List>
int pose_on(sift_hip_verifier* v, const Call& c, const List& list, const Outputs& o) {
    const PoseCameras cams = cameras_of(c);
    launch_verify_gather(list, v->dPts, o.stream);
    if (c.model == VerifyModel::Homography) {
        launch_plane_decompose(cams, c.P, o.result, v->dPlaneCand, o.candidates, o.stream);
        launch_plane_select(list, v->dPts, o.mask, v->dPlaneCand, c.pose_params->max_depth,
                            c.pose_params->max_cos_parallax, static_cast<PlanePoseResult*>(o.pose), o.mask_out, o.points,
                            o.out, o.out_counts, o.stream);
    } else {
        launch_pose_decompose(cams, c.P, o.result, v->dPoseCand, o.stream);
        launch_pose_select(list, v->dPts, o.mask, v->dPoseCand, c.pose_params->max_depth,
                           c.pose_params->max_cos_parallax, static_cast<PoseResult*>(o.pose), o.mask_out, o.points, o.out,
                           o.out_counts, o.stream);
    }
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

template <class List>
int enqueue(sift_hip_verifier* v, const Call& c, const List& list, const Outputs& o) {
    return c.op == Op::Verify  ? verify_on(v, c, list, o)
           : c.op == Op::Score ? score_on(v, c, list, o)
           : c.op == Op::Pose  ? pose_on(v, c, list, o)
                               : refine_on(v, c, list, o);
}

// The host forms' copy-back, one loop over the pair table: the records, each pair's first min(n, cap) rows at its row0
// (the rows past them stay as they are, as on the device), and the mask.
int copy_rows(const sift_hip_verifier* v, const Call& c, const VerifyBatch& b, const int* n) {
    for (int p = 0; c.out && p < b.P; p++) {
        const int rows = std::min(n[p], b.pair[p].cap), row0 = b.pair[p].row0;
        if (rows > 0)
            HIPCHK(hipMemcpy(c.out + row0, v->dOut + row0, sizeof(MatchRecord) * (size_t)rows, hipMemcpyDeviceToHost));
    }
    return SIFT_HIP_OK;
}

int verify_to_host(const sift_hip_verifier* v, const Call& c, const VerifyBatch& b) {
    HIPCHK(hipMemcpy(c.result, v->dResult, sizeof(VerifyResult) * (size_t)b.P, hipMemcpyDeviceToHost));
    int n[kVerifyMaxPairs];
    for (int p = 0; p < b.P; p++) n[p] = static_cast<const VerifyResult*>(c.result)[p].inliers;
    if (int rc = copy_rows(v, c, b, n)) return rc;
    if (c.mask && b.rows > 0) HIPCHK(hipMemcpy(c.mask, v->dMask, (size_t)b.rows, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

int refine_from_host(const sift_hip_verifier* v, const Call& c, const VerifyBatch& b) {
    HIPCHK(hipMemcpy(v->dResult, c.result, sizeof(VerifyResult) * (size_t)b.P, hipMemcpyHostToDevice));
    if (b.rows > 0) HIPCHK(hipMemcpy(v->dMask, c.mask, (size_t)b.rows, hipMemcpyHostToDevice));
    return SIFT_HIP_OK;
}

int refine_to_host(const sift_hip_verifier* v, const Call& c, const VerifyBatch& b) {
    int n[kVerifyMaxPairs], accepted[kVerifyMaxPairs];
    HIPCHK(hipMemcpy(n, v->dRefineInts, sizeof(int) * (size_t)b.P, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(accepted, v->dRefineInts + v->maxP, sizeof(int) * (size_t)b.P, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(c.result, v->dResult, sizeof(VerifyResult) * (size_t)b.P, hipMemcpyDeviceToHost));
    if (b.rows > 0) HIPCHK(hipMemcpy(c.mask, v->dMask, (size_t)b.rows, hipMemcpyDeviceToHost));
    if (int rc = copy_rows(v, c, b, n)) return rc;
    if (c.out_counts) std::copy(n, n + b.P, c.out_counts);
    if (c.accepted) std::copy(accepted, accepted + b.P, c.accepted);
    return SIFT_HIP_OK;
}

// The pose calls' host form: the records and masks go up as for a refine call; the mask comes back as mask_out (on
// the device it is written over the uploaded mask, which the call allows), the points pair by pair up to each n.
int pose_to_host(const sift_hip_verifier* v, const Call& c, const VerifyBatch& b) {
    int n[kVerifyMaxPairs];
    HIPCHK(hipMemcpy(n, v->dRefineInts, sizeof(int) * (size_t)b.P, hipMemcpyDeviceToHost));
    if (c.model == VerifyModel::Homography) {
        HIPCHK(hipMemcpy(c.pose, v->dPlanePose, sizeof(PlanePoseResult) * (size_t)b.P, hipMemcpyDeviceToHost));
        if (c.candidates)
            HIPCHK(hipMemcpy(c.candidates, v->dPlaneOut, sizeof(PlaneCandidate) * 4 * (size_t)b.P, hipMemcpyDeviceToHost));
    } else {
        HIPCHK(hipMemcpy(c.pose, v->dPose, sizeof(PoseResult) * (size_t)b.P, hipMemcpyDeviceToHost));
    }
    if (c.mask_out && b.rows > 0) HIPCHK(hipMemcpy(c.mask_out, v->dMask, (size_t)b.rows, hipMemcpyDeviceToHost));
    if (c.points && b.rows > 0) {
        int counts[kVerifyMaxPairs];
        if (b.counts) HIPCHK(hipMemcpy(counts, b.counts, sizeof(int) * (size_t)b.P, hipMemcpyDeviceToHost));
        for (int p = 0; p < b.P; p++) {
            const int cap = b.pair[p].cap, rows = b.counts ? std::min(std::max(counts[p], 0), cap) : cap;
            if (rows > 0)
                HIPCHK(hipMemcpy(c.points + 3 * (size_t)b.pair[p].row0, v->dPoints + 3 * (size_t)b.pair[p].row0,
                                 sizeof(float) * 3 * (size_t)rows, hipMemcpyDeviceToHost));
        }
    }
    if (int rc = copy_rows(v, c, b, n)) return rc;
    if (c.out_counts) std::copy(n, n + b.P, c.out_counts);
    return SIFT_HIP_OK;
}

// Every list-taking entry point: the rules, for a host form the uploads, the launches, for a host form the copy-back.
int run(sift_hip_verifier* v, const Call& c) {
    VerifyBatch b;
    if (int rc = check(v, c, b)) return rc;
    const bool pose = c.op == Op::Pose, refine = c.op == Op::Refine || pose;  // both read a record and a mask
    HIPCHK(hipSetDevice(v->device));
    if (c.host && refine)
        if (int rc = refine_from_host(v, c, b)) return rc;
    Outputs o = c.host ? Outputs{v->dResult, v->dOut, refine ? v->dRefineInts : nullptr, v->dMask,
                                 refine ? v->dRefineInts + v->maxP : nullptr, nullptr}
                       : Outputs{static_cast<VerifyResult*>(c.result), reinterpret_cast<MatchRecord*>(c.out), c.out_counts,
                                 c.mask, c.accepted, (hipStream_t)c.stream};
    if (pose) {  // a host form writes the in-front mask over the uploaded mask, which the call allows
        const bool plane = c.model == VerifyModel::Homography;
        o.pose = !c.host ? c.pose : plane ? (void*)v->dPlanePose : (void*)v->dPose;
        o.candidates = !c.host ? static_cast<PlaneCandidate*>(c.candidates) : c.candidates ? v->dPlaneOut : nullptr;
        o.mask_out = !c.host ? c.mask_out : c.mask_out ? v->dMask : nullptr;
        o.points = !c.host ? c.points : c.points ? v->dPoints : nullptr;
    }
    const VerifyBatchPair& e = b.pair[0];
    const int rc = c.single ? enqueue(v, c, VerifyInput{b.matches, b.counts, e.cap, e.qxy, e.txy, b.qstride, b.tstride,
                                                        e.nq, e.nt}, o)
                            : enqueue(v, c, b, o);
    if (rc || !c.host) return rc;
    return pose ? pose_to_host(v, c, b) : refine ? refine_to_host(v, c, b) : verify_to_host(v, c, b);
}

// What the last verify call of `model` drew (m indices per hypothesis), solved and counted.
int hypotheses_host(sift_hip_verifier* v, VerifyModel model, int m, int* samples, float* M, int* counts, int cap) {
    if (!v) return fail(SIFT_HIP_ERR_INVALID, "null verifier");
    if (cap < 0) return fail(SIFT_HIP_ERR_INVALID, "verify: negative cap");
    if (v->lastK == 0) return fail(SIFT_HIP_ERR_STATE, "no verify call has run on this verifier");
    if (v->lastBatch) return fail(SIFT_HIP_ERR_STATE, "the verifier's last verify call was a batch");
    if (v->lastModel != (int)model)
        return fail(SIFT_HIP_ERR_STATE, "the verifier's last verify call was of the other model");  // or of another
    const size_t K = (size_t)std::min(cap, v->lastK), S = K * (size_t)model_slots(model);  // samples, model slots
    if (K == 0) return SIFT_HIP_OK;
    const bool ess = model == VerifyModel::Essential;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceSynchronize());
    if (samples)
        HIPCHK(hipMemcpy(samples, ess ? v->dEssSamples : v->dSamples, sizeof(int) * (size_t)m * K, hipMemcpyDeviceToHost));
    if (M) HIPCHK(hipMemcpy(M, ess ? v->dEssF : v->dF, sizeof(float) * 9 * S, hipMemcpyDeviceToHost));
    if (counts) HIPCHK(hipMemcpy(counts, ess ? v->dEssCounts : v->dCounts, sizeof(int) * S, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

// The projection's rows: in place (the same rows: a thread reads its row before it writes it) or apart; anything
// between is refused.  (differences, not sums: an extent may be as large as the address space)
bool rows_overlap(const float* xy, int stride, const float* out_xy, int out_stride, int n) {
    const uintptr_t ib = (uintptr_t)xy, ob = (uintptr_t)out_xy;
    const uintptr_t ibytes = sizeof(float) * ((size_t)(n - 1) * (size_t)stride + 2);
    const uintptr_t obytes = sizeof(float) * ((size_t)(n - 1) * (size_t)out_stride + 2);
    return !(ib == ob && stride == out_stride) && (ib <= ob ? ob - ib < ibytes : ib - ob < obytes);
}

// The affine calls' model argument; anything else is VerifyModel{0}, which check() refuses.
VerifyModel affine_model(int model) {
    return model == SIFT_HIP_MODEL_AFFINE       ? VerifyModel::Affine
           : model == SIFT_HIP_MODEL_SIMILARITY ? VerifyModel::Similarity
                                                : VerifyModel{0};
}

}  // namespace

extern "C" {

void sift_hip_default_pose_params(sift_hip_pose_params* p) {
    if (!p) return;
    p->max_depth = 50.f;
    p->max_cos_parallax = 0.99998f;
}

void sift_hip_default_verify_params(sift_hip_verify_params* p) {
    if (!p) return;
    p->hypotheses = 1024;
    p->seed = 0u;
    p->max_error = 1.5f;
}

int sift_hip_verifier_create(int device, int max_matches, int max_hypotheses, sift_hip_verifier_t* out) {
    if (max_matches > kVerifyMaxMatches) return fail(SIFT_HIP_ERR_INVALID, "bad verifier limits");
    return sift_hip_verifier_create_batched(device, max_matches, max_hypotheses, 1, out);
}

int sift_hip_verifier_create_batched(int device, int max_matches, int max_hypotheses, int max_pairs,
                                     sift_hip_verifier_t* out) {
    if (!out || max_matches < 1 || max_matches > kVerifyMaxPairs * kVerifyMaxMatches || max_hypotheses < 1 ||
        max_hypotheses > kVerifyMaxHypotheses || max_pairs < 1 || max_pairs > kVerifyMaxPairs)
        return fail(SIFT_HIP_ERR_INVALID, "bad verifier limits");
    *out = nullptr;
    auto* v = new sift_hip_verifier();
    if (device < 0) {
        if (hipGetDevice(&v->device) != hipSuccess) v->device = 0;
    } else {
        v->device = device;
    }
    v->maxM = max_matches;
    v->maxK = max_hypotheses;
    v->maxP = max_pairs;
    const size_t M = (size_t)max_matches, K = (size_t)max_hypotheses * (size_t)max_pairs;
    if (hipSetDevice(v->device) != hipSuccess || hipMalloc((void**)&v->dPts, sizeof(float4) * M) != hipSuccess ||
        hipMalloc((void**)&v->dSamples, sizeof(int) * 8 * K) != hipSuccess ||
        hipMalloc((void**)&v->dF, sizeof(float) * 9 * K) != hipSuccess ||
        hipMalloc((void**)&v->dValid, sizeof(int) * K) != hipSuccess ||
        hipMalloc((void**)&v->dCounts, sizeof(int) * K) != hipSuccess ||
        hipMalloc((void**)&v->dResult, sizeof(VerifyResult) * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dOut, sizeof(MatchRecord) * M) != hipSuccess ||
        hipMalloc((void**)&v->dMask, M) != hipSuccess ||
        hipMalloc((void**)&v->dCand, sizeof(RefitCandidate) * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dRefineInts, sizeof(int) * 2 * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dPoseCand, sizeof(PoseCandidates) * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dPose, sizeof(PoseResult) * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dPoints, sizeof(float) * 3 * M) != hipSuccess ||
        hipMalloc((void**)&v->dPlaneCand, sizeof(PlaneCandidates) * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dPlanePose, sizeof(PlanePoseResult) * (size_t)max_pairs) != hipSuccess ||
        hipMalloc((void**)&v->dPlaneOut, sizeof(PlaneCandidate) * 4 * (size_t)max_pairs) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete v;
        return fail(SIFT_HIP_ERR_NOMEM, "verifier allocation failed");
    }
    *out = v;
    return SIFT_HIP_OK;
}

int sift_hip_verifier_reserve_essential(sift_hip_verifier_t v, int max_samples) {
    if (!v) return fail(SIFT_HIP_ERR_INVALID, "null verifier");
    if (max_samples < 1 || max_samples > kVerifyMaxHypotheses)
        return fail(SIFT_HIP_ERR_INVALID, "reserve: max_samples outside 1.." + std::to_string(kVerifyMaxHypotheses));
    if (v->essK != 0) return fail(SIFT_HIP_ERR_STATE, "reserve: the verifier has its essential scratch");
    const size_t K = (size_t)max_samples * (size_t)v->maxP, S = K * kEssentialSlots;
    if (hipSetDevice(v->device) != hipSuccess || hipMalloc((void**)&v->dEssSamples, sizeof(int) * 5 * K) != hipSuccess ||
        hipMalloc((void**)&v->dEssF, sizeof(float) * 9 * S) != hipSuccess ||
        hipMalloc((void**)&v->dEssValid, sizeof(int) * S) != hipSuccess ||
        hipMalloc((void**)&v->dEssCounts, sizeof(int) * S) != hipSuccess ||
        hipMalloc((void**)&v->dEssCams, sizeof(PoseCamera) * 2 * kVerifyMaxPairs) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        for (void** p : {(void**)&v->dEssSamples, (void**)&v->dEssF, (void**)&v->dEssValid, (void**)&v->dEssCounts,
                         (void**)&v->dEssCams}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        return fail(SIFT_HIP_ERR_NOMEM, "essential scratch allocation failed");
    }
    v->essK = max_samples;
    return SIFT_HIP_OK;
}

int sift_hip_verifier_destroy(sift_hip_verifier_t v) {
    delete v;
    return SIFT_HIP_OK;
}

// The twenty-four verify and refine entry points: {fundamental, homography, affine} x {one pair, batch} x
// {verify, refine} x {device, host}.  Each fills the call record and runs it.  The affine calls carry one more
// argument, the model (affine map or similarity), behind the handle (MODEL_ARG).
#define SIFT_ONE_PAIR                                                                                               \
    const int* count, int cap, const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride, \
        int nt
#define SIFT_ONE_PAIR_LIST(c)                                         \
    const sift_hip_verify_pair one{query_xy, train_xy, nq, nt, cap}; \
    c.single = true, c.counts = count, c.P = 1, c.pairs = &one
#define SIFT_BATCH const int* counts, int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride
#define SIFT_BATCH_LIST(c) c.single = false, c.counts = counts, c.P = P, c.pairs = pairs

#define SIFT_VERIFIER_ENTRIES(name, MODEL_ARG, MODEL, RESULT, LIST_ARGS, LIST)                                           \
    int sift_hip_verify_##name##_device(sift_hip_verifier_t v, MODEL_ARG const sift_hip_dmatch* matches, LIST_ARGS,      \
                                        const sift_hip_verify_params* params, RESULT* result, sift_hip_dmatch* out,      \
                                        int* out_count, uint8_t* mask, void* stream) {                                   \
        Call c = make_call(Op::Verify, MODEL, false, matches, query_stride, train_stride);                               \
        LIST(c);                                                                                                         \
        c.params = params, c.result = result, c.out = out, c.out_counts = out_count, c.mask = mask, c.stream = stream;   \
        return run(v, c);                                                                                                \
    }                                                                                                                    \
    int sift_hip_verify_##name##_host(sift_hip_verifier_t v, MODEL_ARG const sift_hip_dmatch* matches, LIST_ARGS,        \
                                      const sift_hip_verify_params* params, RESULT* result_host,                         \
                                      sift_hip_dmatch* out_host, uint8_t* mask_host) {                                   \
        Call c = make_call(Op::Verify, MODEL, true, matches, query_stride, train_stride);                                \
        LIST(c);                                                                                                         \
        c.params = params, c.result = result_host, c.out = out_host, c.mask = mask_host;                                 \
        return run(v, c);                                                                                                \
    }                                                                                                                    \
    int sift_hip_refine_##name##_device(sift_hip_verifier_t v, MODEL_ARG const sift_hip_dmatch* matches, LIST_ARGS,      \
                                        float max_error, int rounds, RESULT* result, uint8_t* mask, sift_hip_dmatch* out, \
                                        int* out_count, int* accepted, void* stream) {                                   \
        const sift_hip_verify_params params{1, 0u, max_error}; /* the one-hypothesis budget every verifier has */        \
        Call c = make_call(Op::Refine, MODEL, false, matches, query_stride, train_stride);                               \
        LIST(c);                                                                                                         \
        c.params = &params, c.rounds = rounds, c.result = result, c.mask = mask, c.out = out, c.out_counts = out_count;  \
        c.accepted = accepted, c.stream = stream;                                                                        \
        return run(v, c);                                                                                                \
    }                                                                                                                    \
    int sift_hip_refine_##name##_host(sift_hip_verifier_t v, MODEL_ARG const sift_hip_dmatch* matches, LIST_ARGS,        \
                                      float max_error, int rounds, RESULT* result_host, uint8_t* mask_host,              \
                                      sift_hip_dmatch* out_host,                                                         \
                                      int* out_count_host, int* accepted_host) {                                         \
        const sift_hip_verify_params params{1, 0u, max_error};                                                           \
        Call c = make_call(Op::Refine, MODEL, true, matches, query_stride, train_stride);                                \
        LIST(c);                                                                                                         \
        c.params = &params, c.rounds = rounds, c.result = result_host, c.mask = mask_host, c.out = out_host;             \
        c.out_counts = out_count_host, c.accepted = accepted_host;                                                       \
        return run(v, c);                                                                                                \
    }
#define SIFT_NO_MODEL_ARG
#define SIFT_MODEL_ARG int model,
SIFT_VERIFIER_ENTRIES(fundamental, SIFT_NO_MODEL_ARG, VerifyModel::Fundamental, sift_hip_verify_result, SIFT_ONE_PAIR,
                      SIFT_ONE_PAIR_LIST)
SIFT_VERIFIER_ENTRIES(homography, SIFT_NO_MODEL_ARG, VerifyModel::Homography, sift_hip_homography_result, SIFT_ONE_PAIR,
                      SIFT_ONE_PAIR_LIST)
SIFT_VERIFIER_ENTRIES(affine, SIFT_MODEL_ARG, affine_model(model), sift_hip_affine_result, SIFT_ONE_PAIR,
                      SIFT_ONE_PAIR_LIST)
SIFT_VERIFIER_ENTRIES(fundamental_batched, SIFT_NO_MODEL_ARG, VerifyModel::Fundamental, sift_hip_verify_result,
                      SIFT_BATCH, SIFT_BATCH_LIST)
SIFT_VERIFIER_ENTRIES(homography_batched, SIFT_NO_MODEL_ARG, VerifyModel::Homography, sift_hip_homography_result,
                      SIFT_BATCH, SIFT_BATCH_LIST)
SIFT_VERIFIER_ENTRIES(affine_batched, SIFT_MODEL_ARG, affine_model(model), sift_hip_affine_result, SIFT_BATCH,
                      SIFT_BATCH_LIST)
#undef SIFT_MODEL_ARG
#undef SIFT_NO_MODEL_ARG
#undef SIFT_VERIFIER_ENTRIES

// The eight pose entry points: {from F, from H} x {one pair, batch} x {device, host}.  The plane pose calls carry one
// more argument, the nullable candidates, at the end (CAND_ARG, CAND_SET).
#define SIFT_POSE_ENTRIES(name, MODEL, RESULT, POSE, LIST_ARGS, LIST, CAND_ARG, CAND_SET)                               \
    int sift_hip_recover_pose##name##_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, LIST_ARGS,          \
                                             const RESULT* result, const uint8_t* mask,                                 \
                                             const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,        \
                                             const sift_hip_pose_params* params, POSE* pose, uint8_t* mask_out,         \
                                             float* points, sift_hip_dmatch* out, int* out_count CAND_ARG,              \
                                             void* stream) {                                                            \
        Call c = make_call(Op::Pose, MODEL, false, matches, query_stride, train_stride);                                \
        LIST(c);                                                                                                        \
        c.result = const_cast<RESULT*>(result), c.mask = const_cast<uint8_t*>(mask);                                    \
        c.cams_q = cam_query, c.cams_t = cam_train, c.pose_params = params, c.pose = pose, c.mask_out = mask_out;       \
        c.points = points, c.out = out, c.out_counts = out_count, c.stream = stream;                                    \
        CAND_SET;                                                                                                       \
        return run(v, c);                                                                                               \
    }                                                                                                                   \
    int sift_hip_recover_pose##name##_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, LIST_ARGS,            \
                                           const RESULT* result_host, const uint8_t* mask_host,                         \
                                           const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,          \
                                           const sift_hip_pose_params* params, POSE* pose_host, uint8_t* mask_out_host, \
                                           float* points_host, sift_hip_dmatch* out_host,                               \
                                           int* out_count_host CAND_ARG) {                                              \
        Call c = make_call(Op::Pose, MODEL, true, matches, query_stride, train_stride);                                 \
        LIST(c);                                                                                                        \
        c.result = const_cast<RESULT*>(result_host), c.mask = const_cast<uint8_t*>(mask_host);                          \
        c.cams_q = cam_query, c.cams_t = cam_train, c.pose_params = params, c.pose = pose_host;                         \
        c.mask_out = mask_out_host, c.points = points_host, c.out = out_host, c.out_counts = out_count_host;            \
        CAND_SET;                                                                                                       \
        return run(v, c);                                                                                               \
    }
#define SIFT_NO_CAND
#define SIFT_CAND_ARG , sift_hip_plane_candidate* candidates
SIFT_POSE_ENTRIES(, VerifyModel::Fundamental, sift_hip_verify_result, sift_hip_pose_result, SIFT_ONE_PAIR,
                  SIFT_ONE_PAIR_LIST, SIFT_NO_CAND, (void)0)
SIFT_POSE_ENTRIES(_batched, VerifyModel::Fundamental, sift_hip_verify_result, sift_hip_pose_result, SIFT_BATCH,
                  SIFT_BATCH_LIST, SIFT_NO_CAND, (void)0)
SIFT_POSE_ENTRIES(_homography, VerifyModel::Homography, sift_hip_homography_result, sift_hip_plane_pose_result,
                  SIFT_ONE_PAIR, SIFT_ONE_PAIR_LIST, SIFT_CAND_ARG, c.candidates = candidates)
SIFT_POSE_ENTRIES(_homography_batched, VerifyModel::Homography, sift_hip_homography_result, sift_hip_plane_pose_result,
                  SIFT_BATCH, SIFT_BATCH_LIST, SIFT_CAND_ARG, c.candidates = candidates)
#undef SIFT_CAND_ARG
#undef SIFT_NO_CAND
#undef SIFT_POSE_ENTRIES

// The four essential entry points: {one pair, batch} x {device, host}.  The verify calls' arguments with the cameras in
// front of the params.
#define SIFT_ESSENTIAL_ENTRIES(name, LIST_ARGS, LIST)                                                                   \
    int sift_hip_verify_essential##name##_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, LIST_ARGS,      \
                                                 const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,    \
                                                 const sift_hip_verify_params* params, sift_hip_verify_result* result,  \
                                                 sift_hip_dmatch* out, int* out_count, uint8_t* mask, void* stream) {   \
        Call c = make_call(Op::Verify, VerifyModel::Essential, false, matches, query_stride, train_stride);             \
        LIST(c);                                                                                                        \
        c.cams_q = cam_query, c.cams_t = cam_train;                                                                     \
        c.params = params, c.result = result, c.out = out, c.out_counts = out_count, c.mask = mask, c.stream = stream;  \
        return run(v, c);                                                                                               \
    }                                                                                                                   \
    int sift_hip_verify_essential##name##_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, LIST_ARGS,        \
                                               const sift_hip_camera* cam_query, const sift_hip_camera* cam_train,      \
                                               const sift_hip_verify_params* params,                                    \
                                               sift_hip_verify_result* result_host, sift_hip_dmatch* out_host,          \
                                               uint8_t* mask_host) {                                                    \
        Call c = make_call(Op::Verify, VerifyModel::Essential, true, matches, query_stride, train_stride);              \
        LIST(c);                                                                                                        \
        c.cams_q = cam_query, c.cams_t = cam_train;                                                                     \
        c.params = params, c.result = result_host, c.out = out_host, c.mask = mask_host;                                \
        return run(v, c);                                                                                               \
    }
SIFT_ESSENTIAL_ENTRIES(, SIFT_ONE_PAIR, SIFT_ONE_PAIR_LIST)
SIFT_ESSENTIAL_ENTRIES(_batched, SIFT_BATCH, SIFT_BATCH_LIST)
#undef SIFT_ESSENTIAL_ENTRIES
#undef SIFT_BATCH_LIST
#undef SIFT_BATCH

static int score_entry(sift_hip_verifier_t v, Call c, const float* M, int K, float max_error, int* counts, void* stream) {
    const sift_hip_verify_params params{K, 0u, max_error};
    c.params = &params, c.models = M, c.scores = counts, c.stream = stream;
    return run(v, c);
}

int sift_hip_score_fundamental_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, SIFT_ONE_PAIR, const float* F,
                                      int K, float max_error, int* counts, void* stream) {
    Call c = make_call(Op::Score, VerifyModel::Fundamental, false, matches, query_stride, train_stride);
    SIFT_ONE_PAIR_LIST(c);
    return score_entry(v, c, F, K, max_error, counts, stream);
}

int sift_hip_score_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, SIFT_ONE_PAIR, const float* H,
                                     int K, float max_error, int* counts, void* stream) {
    Call c = make_call(Op::Score, VerifyModel::Homography, false, matches, query_stride, train_stride);
    SIFT_ONE_PAIR_LIST(c);
    return score_entry(v, c, H, K, max_error, counts, stream);
}

// The predicate is both affine models' own, so the call takes no model argument.
int sift_hip_score_affine_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, SIFT_ONE_PAIR, const float* A,
                                 int K, float max_error, int* counts, void* stream) {
    Call c = make_call(Op::Score, VerifyModel::Affine, false, matches, query_stride, train_stride);
    SIFT_ONE_PAIR_LIST(c);
    return score_entry(v, c, A, K, max_error, counts, stream);
}
#undef SIFT_ONE_PAIR_LIST
#undef SIFT_ONE_PAIR

int sift_hip_verify_hypotheses_host(sift_hip_verifier_t v, int* samples, float* F, int* counts, int cap) {
    return hypotheses_host(v, VerifyModel::Fundamental, 8, samples, F, counts, cap);
}

int sift_hip_verify_homography_hypotheses_host(sift_hip_verifier_t v, int* samples, float* H, int* counts, int cap) {
    return hypotheses_host(v, VerifyModel::Homography, 4, samples, H, counts, cap);
}

int sift_hip_verify_affine_hypotheses_host(sift_hip_verifier_t v, int model, int* samples, float* A, int* counts,
                                           int cap) {
    const VerifyModel m = affine_model(model);
    if (v && (int)m == 0)
        return fail(SIFT_HIP_ERR_INVALID, "verify: model must be SIFT_HIP_MODEL_AFFINE or SIFT_HIP_MODEL_SIMILARITY");
    return hypotheses_host(v, m, sample_size(m), samples, A, counts, cap);
}

// samples: cap x 5, F: 10 cap x 9, counts: 10 cap.
int sift_hip_verify_essential_hypotheses_host(sift_hip_verifier_t v, int* samples, float* F, int* counts, int cap) {
    return hypotheses_host(v, VerifyModel::Essential, 5, samples, F, counts, cap);
}

int sift_hip_project_homography_device(const float* H, const float* xy, int stride, int n, float* out_xy, int out_stride,
                                       void* stream) {
    if (!H) return fail(SIFT_HIP_ERR_INVALID, "project: null H");
    if (stride < 2 || out_stride < 2) return fail(SIFT_HIP_ERR_INVALID, "project: a position stride below 2 floats");
    if (n < 0) return fail(SIFT_HIP_ERR_INVALID, "project: a negative row count");
    if (n == 0) return SIFT_HIP_OK;
    if (!xy || !out_xy) return fail(SIFT_HIP_ERR_INVALID, "project: null position pointer");
    if (rows_overlap(xy, stride, out_xy, out_stride, n))
        return fail(SIFT_HIP_ERR_INVALID, "project: out_xy overlaps xy (only out_xy == xy with equal strides may)");
    launch_project_homography(H, xy, stride, n, out_xy, out_stride, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

int sift_hip_project_homography_batched_device(const void* geometry, int geometry_stride_bytes, int P,
                                               const sift_hip_project_set* sets, int stride, int out_stride,
                                               void* stream) {
    if (!geometry) return fail(SIFT_HIP_ERR_INVALID, "project: null geometry");
    if (geometry_stride_bytes < 36 || geometry_stride_bytes % 4)
        return fail(SIFT_HIP_ERR_INVALID, "project: geometry_stride_bytes must be >= 36 and a multiple of 4");
    if (P <= 0 || P > kVerifyMaxPairs || !sets) return fail(SIFT_HIP_ERR_INVALID, "project: bad batch");
    if (stride < 2 || out_stride < 2) return fail(SIFT_HIP_ERR_INVALID, "project: a position stride below 2 floats");
    ProjectBatch b{};
    b.P = P;
    for (int p = 0; p < P; p++) {
        const int n = sets[p].n;
        if (n < 0) return fail(SIFT_HIP_ERR_INVALID, "project: a negative row count");
        b.pair[p] = ProjectPair{sets[p].xy, sets[p].out_xy, n};
        b.max_n = std::max(b.max_n, n);
        if (n == 0) continue;
        if (!sets[p].xy || !sets[p].out_xy) return fail(SIFT_HIP_ERR_INVALID, "project: null position pointer");
        if (rows_overlap(sets[p].xy, stride, sets[p].out_xy, out_stride, n))  // per pair as in the single call
            return fail(SIFT_HIP_ERR_INVALID, "project: out_xy overlaps xy (only out_xy == xy with equal strides may)");
    }
    if (b.max_n == 0) return SIFT_HIP_OK;
    launch_project_homography_batched(geometry, geometry_stride_bytes, b, stride, out_stride, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

}  // extern "C"
