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
    int* dSamples = nullptr;     // 8 per hypothesis (the homography uses 4), maxP x maxK hypotheses as are dF .. dCounts
    float* dF = nullptr;         // 9 per hypothesis (F, or H)
    int* dValid = nullptr;
    int* dCounts = nullptr;
    // the outputs of sift_hip_verify_fundamental_host / _homography_host and their batched forms
    VerifyResult* dResult = nullptr;  // maxP records
    MatchRecord* dOut = nullptr;
    uint8_t* dMask = nullptr;
    RefitCandidate* dCand = nullptr;  // the refit's candidate model per pair (sift_hip_refine_*), maxP records
    int* dRefineInts = nullptr;       // sift_hip_refine_*_host: maxP out counts, then maxP accepted rounds
    int lastK = 0;               // hypotheses of the last verify call (sift_hip_verify_*hypotheses_host)
    int lastModel = 0;           // its VerifyModel, 0: none
    bool lastBatch = false;      // it was a batched call (the getters read one pair's scratch layout)
    ~sift_hip_verifier() {
        (void)hipSetDevice(device);
        for (void* p : {(void*)dPts, (void*)dSamples, (void*)dF, (void*)dValid, (void*)dCounts, (void*)dResult,
                        (void*)dOut, (void*)dMask, (void*)dCand, (void*)dRefineInts})
            if (p) (void)hipFree(p);
    }
};

static_assert(sizeof(sift_hip_verify_result) == sizeof(VerifyResult), "the result record is written by the kernel");
static_assert(sizeof(sift_hip_homography_result) == sizeof(VerifyResult) &&
                  offsetof(sift_hip_homography_result, inliers) == offsetof(VerifyResult, inliers),
              "both models' result records share the kernel's layout");

namespace {

// What can be judged without the handle first (nothing is dereferenced), then the handle's limits.  Nothing is
// launched on a failure.
int check_input(const sift_hip_verifier* v, const sift_hip_dmatch* matches, int cap, const float* query_xy,
                int query_stride, int nq, const float* train_xy, int train_stride, int nt) {
    if (!v) return fail(SIFT_HIP_ERR_INVALID, "null verifier");
    if (cap < 0 || cap > kVerifyMaxMatches)
        return fail(SIFT_HIP_ERR_INVALID, "verify: cap must lie in 0.." + std::to_string(kVerifyMaxMatches));
    if (query_stride < 2 || train_stride < 2) return fail(SIFT_HIP_ERR_INVALID, "verify: a position stride below 2 floats");
    if (nq < 0 || nt < 0) return fail(SIFT_HIP_ERR_INVALID, "verify: a negative position row count");
    if (cap > 0 && !matches) return fail(SIFT_HIP_ERR_INVALID, "verify: null matches");
    if (cap > 0 && (!query_xy || !train_xy)) return fail(SIFT_HIP_ERR_INVALID, "verify: null position pointer");
    return SIFT_HIP_OK;
}
int check_error(float max_error) {
    if (!(max_error > 0.f) || !std::isfinite(max_error))
        return fail(SIFT_HIP_ERR_INVALID, "verify: max_error must be > 0 and finite");
    return SIFT_HIP_OK;
}
int check_limits(const sift_hip_verifier* v, int cap, int K) {
    if (K < 1 || K > kVerifyMaxHypotheses || K > v->maxK)
        return fail(SIFT_HIP_ERR_INVALID, "verify: hypotheses outside 1..max_hypotheses");
    if (cap > v->maxM) return fail(SIFT_HIP_ERR_INVALID, "verify: cap exceeds the verifier's max_matches");
    return SIFT_HIP_OK;
}

int verify_device(sift_hip_verifier* v, VerifyModel model, const VerifyInput& in, const sift_hip_verify_params& p,
                  VerifyResult* result, MatchRecord* out, int* out_count, uint8_t* mask, hipStream_t s) {
    const float e2 = p.max_error * p.max_error;
    HIPCHK(hipSetDevice(v->device));
    launch_verify_gather(in, v->dPts, s);
    launch_verify_hypotheses(model, in, v->dPts, p.hypotheses, p.seed, v->dSamples, v->dF, v->dValid, s);
    launch_verify_score(model, in, v->dPts, v->dF, v->dValid, p.hypotheses, e2, v->dCounts, s);
    launch_verify_select(model, in, v->dPts, v->dF, v->dValid, v->dCounts, p.hypotheses, e2, result, out, out_count, mask,
                         s);
    HIPCHK(hipGetLastError());
    v->lastK = p.hypotheses;
    v->lastModel = (int)model;
    v->lastBatch = false;
    return SIFT_HIP_OK;
}

// The refit's own argument rules (sift_hip_refine_*), judged without the handle.
struct RefineArgs {
    int rounds;
    const uint8_t* mask;
};
constexpr int kRefineMaxRounds = 8;

int check_refine(int rounds, const void* result, const uint8_t* mask, int rows) {
    if (!result) return fail(SIFT_HIP_ERR_INVALID, "refine: null result");
    if (rows > 0 && !mask) return fail(SIFT_HIP_ERR_INVALID, "refine: null mask (the mask is the fit set)");
    if (rounds < 1 || rounds > kRefineMaxRounds)
        return fail(SIFT_HIP_ERR_INVALID, "refine: rounds must lie in 1.." + std::to_string(kRefineMaxRounds));
    return SIFT_HIP_OK;
}

// The batched call's argument rules: what can be judged without the handle first, then its limits; `b` is the pair
// table the kernels take.  out: the device form's output rows (may not overlap matches), null otherwise.  refine: a
// refine call's further arguments, judged before the limits.
int check_batch(const sift_hip_verifier* v, const sift_hip_dmatch* matches, const int* counts, int P,
                const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                const sift_hip_verify_params* params, const void* results, const sift_hip_dmatch* out, VerifyBatch& b,
                const RefineArgs* refine = nullptr) {
    if (!v) return fail(SIFT_HIP_ERR_INVALID, "null verifier");
    if (!pairs) return fail(SIFT_HIP_ERR_INVALID, "verify: null pairs");
    if (!params || !results) return fail(SIFT_HIP_ERR_INVALID, "verify: null params or result");
    if (P < 1 || P > kVerifyMaxPairs)
        return fail(SIFT_HIP_ERR_INVALID, "verify: pairs outside 1.." + std::to_string(kVerifyMaxPairs));
    if (query_stride < 2 || train_stride < 2) return fail(SIFT_HIP_ERR_INVALID, "verify: a position stride below 2 floats");
    int rows = 0, max_cap = 0;  // P x 65536 fits
    for (int p = 0; p < P; p++) {
        const sift_hip_verify_pair& e = pairs[p];
        const std::string at = " (pair " + std::to_string(p) + ")";
        if (e.cap < 0 || e.cap > kVerifyMaxMatches)
            return fail(SIFT_HIP_ERR_INVALID, "verify: cap must lie in 0.." + std::to_string(kVerifyMaxMatches) + at);
        if (e.nq < 0 || e.nt < 0) return fail(SIFT_HIP_ERR_INVALID, "verify: a negative position row count" + at);
        if (e.cap > 0 && (!e.query_xy || !e.train_xy))
            return fail(SIFT_HIP_ERR_INVALID, "verify: null position pointer" + at);
        b.pair[p] = VerifyBatchPair{e.query_xy, e.train_xy, rows, e.cap, e.nq, e.nt};
        rows += e.cap;
        max_cap = std::max(max_cap, e.cap);
    }
    if (rows > 0 && !matches) return fail(SIFT_HIP_ERR_INVALID, "verify: null matches");
    if (int rc = check_error(params->max_error)) return rc;
    const uintptr_t ob = (uintptr_t)out, mb = (uintptr_t)matches, bytes = sizeof(sift_hip_dmatch) * (size_t)rows;
    if (out && rows > 0 && ob < mb + bytes && mb < ob + bytes)
        return fail(SIFT_HIP_ERR_INVALID, "verify: out aliases matches");
    if (refine)
        if (int rc = check_refine(refine->rounds, results, refine->mask, rows)) return rc;
    if (params->hypotheses < 1 || params->hypotheses > kVerifyMaxHypotheses || params->hypotheses > v->maxK)
        return fail(SIFT_HIP_ERR_INVALID, "verify: hypotheses outside 1..max_hypotheses");
    if (P > v->maxP) return fail(SIFT_HIP_ERR_INVALID, "verify: more pairs than the verifier's max_pairs");
    if (rows > v->maxM) return fail(SIFT_HIP_ERR_INVALID, "verify: the caps' sum exceeds the verifier's max_matches");
    b.matches = reinterpret_cast<const MatchRecord*>(matches);
    b.counts = counts;
    b.qstride = query_stride, b.tstride = train_stride;
    b.P = P, b.rows = rows, b.max_cap = max_cap;
    return SIFT_HIP_OK;
}

// One launch per step for the whole batch.  Every index stays inside the handle's scratch: rows <= maxM,
// P <= maxP and K <= maxK were checked.
int verify_batched_device(sift_hip_verifier* v, VerifyModel model, const VerifyBatch& b, const sift_hip_verify_params& p,
                          VerifyResult* results, MatchRecord* out, int* out_counts, uint8_t* mask, hipStream_t s) {
    const float e2 = p.max_error * p.max_error;
    HIPCHK(hipSetDevice(v->device));
    launch_verify_gather_batched(b, v->dPts, s);
    launch_verify_hypotheses_batched(model, b, v->dPts, p.hypotheses, p.seed, v->dSamples, v->dF, v->dValid, s);
    launch_verify_score_batched(model, b, v->dPts, v->dF, v->dValid, p.hypotheses, e2, v->dCounts, s);
    launch_verify_select_batched(model, b, v->dPts, v->dF, v->dValid, v->dCounts, p.hypotheses, e2, results, out,
                                 out_counts, mask, s);
    HIPCHK(hipGetLastError());
    v->lastK = p.hypotheses;
    v->lastModel = (int)model;
    v->lastBatch = true;
    return SIFT_HIP_OK;
}

int verify_model_batched_device(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches,
                                const int* counts, int P, const sift_hip_verify_pair* pairs, int query_stride,
                                int train_stride, const sift_hip_verify_params* params, void* results,
                                sift_hip_dmatch* out, int* out_counts, uint8_t* mask, void* stream) {
    VerifyBatch b{};
    if (int rc = check_batch(v, matches, counts, P, pairs, query_stride, train_stride, params, results, out, b)) return rc;
    return verify_batched_device(v, model, b, *params, static_cast<VerifyResult*>(results),
                                 reinterpret_cast<MatchRecord*>(out), out_counts, mask, (hipStream_t)stream);
}

int verify_model_batched_host(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* counts,
                              int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                              const sift_hip_verify_params* params, void* results_host, sift_hip_dmatch* out_host,
                              uint8_t* mask_host) {
    VerifyBatch b{};
    if (int rc = check_batch(v, matches, counts, P, pairs, query_stride, train_stride, params, results_host, nullptr, b))
        return rc;
    if (int rc = verify_batched_device(v, model, b, *params, v->dResult, v->dOut, nullptr, v->dMask, nullptr)) return rc;
    HIPCHK(hipMemcpy(results_host, v->dResult, sizeof(VerifyResult) * (size_t)P, hipMemcpyDeviceToHost));
    const VerifyResult* r = static_cast<const VerifyResult*>(results_host);
    for (int p = 0; out_host && p < P; p++) {  // a pair's rows past its inliers stay as they are, as on the device
        const int n = std::min(r[p].inliers, b.pair[p].cap), row0 = b.pair[p].row0;
        if (n > 0)
            HIPCHK(hipMemcpy(out_host + row0, v->dOut + row0, sizeof(MatchRecord) * (size_t)n, hipMemcpyDeviceToHost));
    }
    if (mask_host && b.rows > 0) HIPCHK(hipMemcpy(mask_host, v->dMask, (size_t)b.rows, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

// The entry points of both models (the record types share a layout): argument rules, then the launches.
int verify_model_device(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* count, int cap,
                        const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                        const sift_hip_verify_params* params, void* result, sift_hip_dmatch* out, int* out_count,
                        uint8_t* mask, void* stream) {
    if (int rc = check_input(v, matches, cap, query_xy, query_stride, nq, train_xy, train_stride, nt)) return rc;
    if (!params || !result) return fail(SIFT_HIP_ERR_INVALID, "verify: null params or result");
    if (int rc = check_error(params->max_error)) return rc;
    const uintptr_t ob = (uintptr_t)out, mb = (uintptr_t)matches, bytes = sizeof(sift_hip_dmatch) * (size_t)cap;
    if (out && cap > 0 && ob < mb + bytes && mb < ob + bytes)
        return fail(SIFT_HIP_ERR_INVALID, "verify: out aliases matches");
    if (int rc = check_limits(v, cap, params->hypotheses)) return rc;
    const VerifyInput in{reinterpret_cast<const MatchRecord*>(matches), count, cap, query_xy, train_xy, query_stride,
                         train_stride, nq, nt};
    return verify_device(v, model, in, *params, static_cast<VerifyResult*>(result), reinterpret_cast<MatchRecord*>(out),
                         out_count, mask, (hipStream_t)stream);
}

int verify_model_host(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* count, int cap,
                      const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                      const sift_hip_verify_params* params, void* result_host, sift_hip_dmatch* out_host,
                      uint8_t* mask_host) {
    if (int rc = check_input(v, matches, cap, query_xy, query_stride, nq, train_xy, train_stride, nt)) return rc;
    if (!params || !result_host) return fail(SIFT_HIP_ERR_INVALID, "verify: null params or result");
    if (int rc = check_error(params->max_error)) return rc;
    if (int rc = check_limits(v, cap, params->hypotheses)) return rc;
    const VerifyInput in{reinterpret_cast<const MatchRecord*>(matches), count, cap, query_xy, train_xy, query_stride,
                         train_stride, nq, nt};
    if (int rc = verify_device(v, model, in, *params, v->dResult, v->dOut, nullptr, v->dMask, nullptr)) return rc;
    HIPCHK(hipMemcpy(result_host, v->dResult, sizeof(VerifyResult), hipMemcpyDeviceToHost));
    const int n = std::min(static_cast<const VerifyResult*>(result_host)->inliers, cap);
    if (out_host && n > 0) HIPCHK(hipMemcpy(out_host, v->dOut, sizeof(MatchRecord) * (size_t)n, hipMemcpyDeviceToHost));
    if (mask_host && cap > 0) HIPCHK(hipMemcpy(mask_host, v->dMask, (size_t)cap, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

int score_model_device(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* count, int cap,
                       const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                       const float* M, int K, float max_error, int* counts, void* stream) {
    if (int rc = check_input(v, matches, cap, query_xy, query_stride, nq, train_xy, train_stride, nt)) return rc;
    if (!M || !counts)
        return fail(SIFT_HIP_ERR_INVALID, model == VerifyModel::Homography ? "verify: null H or counts"
                                                                           : "verify: null F or counts");
    if (int rc = check_error(max_error)) return rc;
    if (int rc = check_limits(v, cap, K)) return rc;
    const VerifyInput in{reinterpret_cast<const MatchRecord*>(matches), count, cap, query_xy, train_xy, query_stride,
                         train_stride, nq, nt};
    HIPCHK(hipSetDevice(v->device));
    launch_verify_gather(in, v->dPts, (hipStream_t)stream);
    launch_verify_score(model, in, v->dPts, M, nullptr, K, max_error * max_error, counts, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// What the last verify call of `model` drew (m indices per hypothesis), solved and counted.
int hypotheses_host(sift_hip_verifier* v, VerifyModel model, int m, int* samples, float* M, int* counts, int cap) {
    if (!v) return fail(SIFT_HIP_ERR_INVALID, "null verifier");
    if (cap < 0) return fail(SIFT_HIP_ERR_INVALID, "verify: negative cap");
    if (v->lastK == 0) return fail(SIFT_HIP_ERR_STATE, "no verify call has run on this verifier");
    if (v->lastBatch) return fail(SIFT_HIP_ERR_STATE, "the verifier's last verify call was a batch");
    if (v->lastModel != (int)model)
        return fail(SIFT_HIP_ERR_STATE, "the verifier's last verify call was of the other model");
    const size_t K = (size_t)std::min(cap, v->lastK);
    if (K == 0) return SIFT_HIP_OK;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipDeviceSynchronize());
    if (samples) HIPCHK(hipMemcpy(samples, v->dSamples, sizeof(int) * (size_t)m * K, hipMemcpyDeviceToHost));
    if (M) HIPCHK(hipMemcpy(M, v->dF, sizeof(float) * 9 * K, hipMemcpyDeviceToHost));
    if (counts) HIPCHK(hipMemcpy(counts, v->dCounts, sizeof(int) * K, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

// --- The refit (sift_hip_refine_*): `rounds` rounds of fit -> rescore -> accept on the gathered list; out is written
// by the last round only.  The verifier's hypothesis scratch is not touched.

int refine_device(sift_hip_verifier* v, VerifyModel model, const VerifyInput& in, float max_error, int rounds,
                  VerifyResult* result, uint8_t* mask, MatchRecord* out, int* out_count, int* accepted, hipStream_t s) {
    const float e2 = max_error * max_error;
    HIPCHK(hipSetDevice(v->device));
    launch_verify_gather(in, v->dPts, s);
    for (int r = 0; r < rounds; r++) {
        const bool last = r == rounds - 1;
        launch_refit_fit(model, in, v->dPts, mask, result, v->dCand, s);
        launch_refit_accept(model, in, v->dPts, v->dCand, e2, result, mask, last ? out : nullptr,
                            last ? out_count : nullptr, accepted, r == 0, s);
    }
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

int refine_batched_device(sift_hip_verifier* v, VerifyModel model, const VerifyBatch& b, float max_error, int rounds,
                          VerifyResult* results, uint8_t* mask, MatchRecord* out, int* out_counts, int* accepted,
                          hipStream_t s) {
    const float e2 = max_error * max_error;
    HIPCHK(hipSetDevice(v->device));
    launch_verify_gather_batched(b, v->dPts, s);
    for (int r = 0; r < rounds; r++) {
        const bool last = r == rounds - 1;
        launch_refit_fit_batched(model, b, v->dPts, mask, results, v->dCand, s);
        launch_refit_accept_batched(model, b, v->dPts, v->dCand, e2, results, mask, last ? out : nullptr,
                                    last ? out_counts : nullptr, accepted, r == 0, s);
    }
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// The single-pair argument rules: the verify call's, then the refit's own.
int check_refine_single(const sift_hip_verifier* v, const sift_hip_dmatch* matches, int cap, const float* query_xy,
                        int query_stride, int nq, const float* train_xy, int train_stride, int nt, float max_error,
                        int rounds, const void* result, const uint8_t* mask, const sift_hip_dmatch* out) {
    if (int rc = check_input(v, matches, cap, query_xy, query_stride, nq, train_xy, train_stride, nt)) return rc;
    if (int rc = check_refine(rounds, result, mask, cap)) return rc;
    if (int rc = check_error(max_error)) return rc;
    const uintptr_t ob = (uintptr_t)out, mb = (uintptr_t)matches, bytes = sizeof(sift_hip_dmatch) * (size_t)cap;
    if (out && cap > 0 && ob < mb + bytes && mb < ob + bytes)
        return fail(SIFT_HIP_ERR_INVALID, "verify: out aliases matches");
    return check_limits(v, cap, 1);
}

int refine_model_device(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* count, int cap,
                        const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                        float max_error, int rounds, void* result, uint8_t* mask, sift_hip_dmatch* out, int* out_count,
                        int* accepted, void* stream) {
    if (int rc = check_refine_single(v, matches, cap, query_xy, query_stride, nq, train_xy, train_stride, nt, max_error,
                                     rounds, result, mask, out))
        return rc;
    const VerifyInput in{reinterpret_cast<const MatchRecord*>(matches), count, cap, query_xy, train_xy, query_stride,
                         train_stride, nq, nt};
    return refine_device(v, model, in, max_error, rounds, static_cast<VerifyResult*>(result), mask,
                         reinterpret_cast<MatchRecord*>(out), out_count, accepted, (hipStream_t)stream);
}

int refine_model_host(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* count, int cap,
                      const float* query_xy, int query_stride, int nq, const float* train_xy, int train_stride, int nt,
                      float max_error, int rounds, void* result_host, uint8_t* mask_host, sift_hip_dmatch* out_host,
                      int* out_count_host, int* accepted_host) {
    if (int rc = check_refine_single(v, matches, cap, query_xy, query_stride, nq, train_xy, train_stride, nt, max_error,
                                     rounds, result_host, mask_host, nullptr))
        return rc;
    const VerifyInput in{reinterpret_cast<const MatchRecord*>(matches), count, cap, query_xy, train_xy, query_stride,
                         train_stride, nq, nt};
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMemcpy(v->dResult, result_host, sizeof(VerifyResult), hipMemcpyHostToDevice));
    if (cap > 0) HIPCHK(hipMemcpy(v->dMask, mask_host, (size_t)cap, hipMemcpyHostToDevice));
    if (int rc = refine_device(v, model, in, max_error, rounds, v->dResult, v->dMask, v->dOut, v->dRefineInts,
                               v->dRefineInts + v->maxP, nullptr))
        return rc;
    int ints[2] = {0, 0};
    HIPCHK(hipMemcpy(&ints[0], v->dRefineInts, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&ints[1], v->dRefineInts + v->maxP, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(result_host, v->dResult, sizeof(VerifyResult), hipMemcpyDeviceToHost));
    if (cap > 0) HIPCHK(hipMemcpy(mask_host, v->dMask, (size_t)cap, hipMemcpyDeviceToHost));
    const int n = std::min(ints[0], cap);
    if (out_host && n > 0) HIPCHK(hipMemcpy(out_host, v->dOut, sizeof(MatchRecord) * (size_t)n, hipMemcpyDeviceToHost));
    if (out_count_host) *out_count_host = ints[0];
    if (accepted_host) *accepted_host = ints[1];
    return SIFT_HIP_OK;
}

// The batched argument rules: check_batch's (with the one-hypothesis budget every verifier has), then the refit's own.
int check_refine_batch(const sift_hip_verifier* v, const sift_hip_dmatch* matches, const int* counts, int P,
                       const sift_hip_verify_pair* pairs, int query_stride, int train_stride, float max_error, int rounds,
                       const void* results, const uint8_t* mask, const sift_hip_dmatch* out, VerifyBatch& b) {
    const sift_hip_verify_params params{1, 0u, max_error};
    const RefineArgs refine{rounds, mask};
    return check_batch(v, matches, counts, P, pairs, query_stride, train_stride, &params, results, out, b, &refine);
}

int refine_model_batched_device(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* counts,
                                int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                float max_error, int rounds, void* results, uint8_t* mask, sift_hip_dmatch* out,
                                int* out_counts, int* accepted, void* stream) {
    VerifyBatch b{};
    if (int rc = check_refine_batch(v, matches, counts, P, pairs, query_stride, train_stride, max_error, rounds, results,
                                    mask, out, b))
        return rc;
    return refine_batched_device(v, model, b, max_error, rounds, static_cast<VerifyResult*>(results), mask,
                                 reinterpret_cast<MatchRecord*>(out), out_counts, accepted, (hipStream_t)stream);
}

int refine_model_batched_host(sift_hip_verifier* v, VerifyModel model, const sift_hip_dmatch* matches, const int* counts,
                              int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                              float max_error, int rounds, void* results_host, uint8_t* mask_host,
                              sift_hip_dmatch* out_host, int* out_counts_host, int* accepted_host) {
    VerifyBatch b{};
    if (int rc = check_refine_batch(v, matches, counts, P, pairs, query_stride, train_stride, max_error, rounds,
                                    results_host, mask_host, nullptr, b))
        return rc;
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMemcpy(v->dResult, results_host, sizeof(VerifyResult) * (size_t)P, hipMemcpyHostToDevice));
    if (b.rows > 0) HIPCHK(hipMemcpy(v->dMask, mask_host, (size_t)b.rows, hipMemcpyHostToDevice));
    if (int rc = refine_batched_device(v, model, b, max_error, rounds, v->dResult, v->dMask, v->dOut, v->dRefineInts,
                                       v->dRefineInts + v->maxP, nullptr))
        return rc;
    int ints[2 * kVerifyMaxPairs];
    HIPCHK(hipMemcpy(ints, v->dRefineInts, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ints + kVerifyMaxPairs, v->dRefineInts + v->maxP, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(results_host, v->dResult, sizeof(VerifyResult) * (size_t)P, hipMemcpyDeviceToHost));
    if (b.rows > 0) HIPCHK(hipMemcpy(mask_host, v->dMask, (size_t)b.rows, hipMemcpyDeviceToHost));
    for (int p = 0; p < P; p++) {  // a pair's rows past its records stay as they are, as on the device
        const int n = std::min(ints[p], b.pair[p].cap), row0 = b.pair[p].row0;
        if (out_host && n > 0)
            HIPCHK(hipMemcpy(out_host + row0, v->dOut + row0, sizeof(MatchRecord) * (size_t)n, hipMemcpyDeviceToHost));
        if (out_counts_host) out_counts_host[p] = ints[p];
        if (accepted_host) accepted_host[p] = ints[kVerifyMaxPairs + p];
    }
    return SIFT_HIP_OK;
}

}  // namespace

extern "C" {

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
        hipDeviceSynchronize() != hipSuccess) {
        delete v;
        return fail(SIFT_HIP_ERR_NOMEM, "verifier allocation failed");
    }
    *out = v;
    return SIFT_HIP_OK;
}

int sift_hip_verifier_destroy(sift_hip_verifier_t v) {
    delete v;
    return SIFT_HIP_OK;
}

int sift_hip_verify_fundamental_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                       const float* query_xy, int query_stride, int nq, const float* train_xy,
                                       int train_stride, int nt, const sift_hip_verify_params* params,
                                       sift_hip_verify_result* result, sift_hip_dmatch* out, int* out_count,
                                       uint8_t* mask, void* stream) {
    return verify_model_device(v, VerifyModel::Fundamental, matches, count, cap, query_xy, query_stride, nq, train_xy,
                               train_stride, nt, params, result, out, out_count, mask, stream);
}

int sift_hip_verify_fundamental_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                     const float* query_xy, int query_stride, int nq, const float* train_xy,
                                     int train_stride, int nt, const sift_hip_verify_params* params,
                                     sift_hip_verify_result* result_host, sift_hip_dmatch* out_host,
                                     uint8_t* mask_host) {
    return verify_model_host(v, VerifyModel::Fundamental, matches, count, cap, query_xy, query_stride, nq, train_xy,
                             train_stride, nt, params, result_host, out_host, mask_host);
}

int sift_hip_score_fundamental_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                      const float* query_xy, int query_stride, int nq, const float* train_xy,
                                      int train_stride, int nt, const float* F, int K, float max_error, int* counts,
                                      void* stream) {
    return score_model_device(v, VerifyModel::Fundamental, matches, count, cap, query_xy, query_stride, nq, train_xy,
                              train_stride, nt, F, K, max_error, counts, stream);
}

int sift_hip_verify_hypotheses_host(sift_hip_verifier_t v, int* samples, float* F, int* counts, int cap) {
    return hypotheses_host(v, VerifyModel::Fundamental, 8, samples, F, counts, cap);
}

int sift_hip_verify_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                      const float* query_xy, int query_stride, int nq, const float* train_xy,
                                      int train_stride, int nt, const sift_hip_verify_params* params,
                                      sift_hip_homography_result* result, sift_hip_dmatch* out, int* out_count,
                                      uint8_t* mask, void* stream) {
    return verify_model_device(v, VerifyModel::Homography, matches, count, cap, query_xy, query_stride, nq, train_xy,
                               train_stride, nt, params, result, out, out_count, mask, stream);
}

int sift_hip_verify_homography_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                    const float* query_xy, int query_stride, int nq, const float* train_xy,
                                    int train_stride, int nt, const sift_hip_verify_params* params,
                                    sift_hip_homography_result* result_host, sift_hip_dmatch* out_host,
                                    uint8_t* mask_host) {
    return verify_model_host(v, VerifyModel::Homography, matches, count, cap, query_xy, query_stride, nq, train_xy,
                             train_stride, nt, params, result_host, out_host, mask_host);
}

int sift_hip_score_homography_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,
                                     const float* query_xy, int query_stride, int nq, const float* train_xy,
                                     int train_stride, int nt, const float* H, int K, float max_error, int* counts,
                                     void* stream) {
    return score_model_device(v, VerifyModel::Homography, matches, count, cap, query_xy, query_stride, nq, train_xy,
                              train_stride, nt, H, K, max_error, counts, stream);
}

int sift_hip_verify_homography_hypotheses_host(sift_hip_verifier_t v, int* samples, float* H, int* counts, int cap) {
    return hypotheses_host(v, VerifyModel::Homography, 4, samples, H, counts, cap);
}

int sift_hip_verify_fundamental_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                               int P, const sift_hip_verify_pair* pairs, int query_stride,
                                               int train_stride, const sift_hip_verify_params* params,
                                               sift_hip_verify_result* results, sift_hip_dmatch* out, int* out_counts,
                                               uint8_t* mask, void* stream) {
    return verify_model_batched_device(v, VerifyModel::Fundamental, matches, counts, P, pairs, query_stride, train_stride,
                                       params, results, out, out_counts, mask, stream);
}

int sift_hip_verify_fundamental_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                             int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                             const sift_hip_verify_params* params, sift_hip_verify_result* results_host,
                                             sift_hip_dmatch* out_host, uint8_t* mask_host) {
    return verify_model_batched_host(v, VerifyModel::Fundamental, matches, counts, P, pairs, query_stride, train_stride,
                                     params, results_host, out_host, mask_host);
}

int sift_hip_verify_homography_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                              int P, const sift_hip_verify_pair* pairs, int query_stride,
                                              int train_stride, const sift_hip_verify_params* params,
                                              sift_hip_homography_result* results, sift_hip_dmatch* out, int* out_counts,
                                              uint8_t* mask, void* stream) {
    return verify_model_batched_device(v, VerifyModel::Homography, matches, counts, P, pairs, query_stride, train_stride,
                                       params, results, out, out_counts, mask, stream);
}

int sift_hip_verify_homography_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,
                                            int P, const sift_hip_verify_pair* pairs, int query_stride, int train_stride,
                                            const sift_hip_verify_params* params,
                                            sift_hip_homography_result* results_host, sift_hip_dmatch* out_host,
                                            uint8_t* mask_host) {
    return verify_model_batched_host(v, VerifyModel::Homography, matches, counts, P, pairs, query_stride, train_stride,
                                     params, results_host, out_host, mask_host);
}

#define SIFT_REFINE_ENTRIES(name, MODEL, RESULT)                                                                          \
    int sift_hip_refine_##name##_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap, \
                                        const float* query_xy, int query_stride, int nq, const float* train_xy,          \
                                        int train_stride, int nt, float max_error, int rounds, RESULT* result,           \
                                        uint8_t* mask, sift_hip_dmatch* out, int* out_count, int* accepted,              \
                                        void* stream) {                                                                  \
        return refine_model_device(v, MODEL, matches, count, cap, query_xy, query_stride, nq, train_xy, train_stride, nt, \
                                   max_error, rounds, result, mask, out, out_count, accepted, stream);                   \
    }                                                                                                                    \
    int sift_hip_refine_##name##_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* count, int cap,  \
                                      const float* query_xy, int query_stride, int nq, const float* train_xy,            \
                                      int train_stride, int nt, float max_error, int rounds, RESULT* result_host,        \
                                      uint8_t* mask_host, sift_hip_dmatch* out_host, int* out_count_host,                \
                                      int* accepted_host) {                                                              \
        return refine_model_host(v, MODEL, matches, count, cap, query_xy, query_stride, nq, train_xy, train_stride, nt,   \
                                 max_error, rounds, result_host, mask_host, out_host, out_count_host, accepted_host);    \
    }                                                                                                                    \
    int sift_hip_refine_##name##_batched_device(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts, \
                                                int P, const sift_hip_verify_pair* pairs, int query_stride,              \
                                                int train_stride, float max_error, int rounds, RESULT* results,          \
                                                uint8_t* mask, sift_hip_dmatch* out, int* out_counts, int* accepted,     \
                                                void* stream) {                                                          \
        return refine_model_batched_device(v, MODEL, matches, counts, P, pairs, query_stride, train_stride, max_error,   \
                                           rounds, results, mask, out, out_counts, accepted, stream);                    \
    }                                                                                                                    \
    int sift_hip_refine_##name##_batched_host(sift_hip_verifier_t v, const sift_hip_dmatch* matches, const int* counts,  \
                                              int P, const sift_hip_verify_pair* pairs, int query_stride,                \
                                              int train_stride, float max_error, int rounds, RESULT* results_host,       \
                                              uint8_t* mask_host, sift_hip_dmatch* out_host, int* out_counts_host,       \
                                              int* accepted_host) {                                                      \
        return refine_model_batched_host(v, MODEL, matches, counts, P, pairs, query_stride, train_stride, max_error,     \
                                         rounds, results_host, mask_host, out_host, out_counts_host, accepted_host);     \
    }
SIFT_REFINE_ENTRIES(fundamental, VerifyModel::Fundamental, sift_hip_verify_result)
SIFT_REFINE_ENTRIES(homography, VerifyModel::Homography, sift_hip_homography_result)
#undef SIFT_REFINE_ENTRIES

int sift_hip_project_homography_device(const float* H, const float* xy, int stride, int n, float* out_xy, int out_stride,
                                       void* stream) {
    if (!H) return fail(SIFT_HIP_ERR_INVALID, "project: null H");
    if (stride < 2 || out_stride < 2) return fail(SIFT_HIP_ERR_INVALID, "project: a position stride below 2 floats");
    if (n < 0) return fail(SIFT_HIP_ERR_INVALID, "project: a negative row count");
    if (n == 0) return SIFT_HIP_OK;
    if (!xy || !out_xy) return fail(SIFT_HIP_ERR_INVALID, "project: null position pointer");
    // In place (the same rows: a thread reads its row before it writes it) or apart; anything between is refused.
    const uintptr_t ib = (uintptr_t)xy, ob = (uintptr_t)out_xy;
    const uintptr_t ibytes = sizeof(float) * ((size_t)(n - 1) * (size_t)stride + 2);
    const uintptr_t obytes = sizeof(float) * ((size_t)(n - 1) * (size_t)out_stride + 2);
    // (differences, not sums: an extent may be as large as the address space)
    if (!(ib == ob && stride == out_stride) && (ib <= ob ? ob - ib < ibytes : ib - ob < obytes))
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
        // Per pair as in the single call: in place (the same rows) or apart.
        const uintptr_t ib = (uintptr_t)sets[p].xy, ob = (uintptr_t)sets[p].out_xy;
        const uintptr_t ibytes = sizeof(float) * ((size_t)(n - 1) * (size_t)stride + 2);
        const uintptr_t obytes = sizeof(float) * ((size_t)(n - 1) * (size_t)out_stride + 2);
        if (!(ib == ob && stride == out_stride) && (ib <= ob ? ob - ib < ibytes : ib - ob < obytes))
            return fail(SIFT_HIP_ERR_INVALID, "project: out_xy overlaps xy (only out_xy == xy with equal strides may)");
    }
    if (b.max_n == 0) return SIFT_HIP_OK;
    launch_project_homography_batched(geometry, geometry_stride_bytes, b, stride, out_stride, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

}  // extern "C"
