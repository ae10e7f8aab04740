// The relative pose from a verified fundamental matrix (sift_hip_recover_pose_*): E = Kt^T F Kq, its four (R, t)
// candidates, the depths of the fit records under each and the candidate that puts the most of them in front of both
// cameras -- cv::recoverPose on the verifier's record, mask and gathered list.  The rule -- associations, eigenvalue
// order, the closed-form depths, the tests, the winner -- is written out in include/sift_hip.h and mirrored in numpy by
// sift_amd.cv.recover_pose.
//
//  k_pose_decompose  one wave per pair: the record's usability, E, N = E^T E, the refit's Jacobi routine on N in LDS
//                    (jacobi<3>), the singular vectors by cross products, R1, R2 and t into the pair's scratch record.
//  k_pose_select     one 512-thread workgroup per pair.  Pass 1 strides over the records: per record the depths under
//                    (R1, t) and (R2, t) -- negating t negates both depths exactly, so the other two candidates cost
//                    nothing --, nine ballots (fit, four in front, four with parallax), popcounts per wave, the waves'
//                    counts combined through LDS; integer counts, exact in any order, no atomics.  Thread 0 writes the
//                    pose record.  Pass 2 (only when an optional output is asked for) recomputes the winner's depths
//                    and writes the mask, the points and k_verify_select's ordered compaction.
// Float64 with -ffp-contract=off: every operation is the one written, in the order written; float64 division and
// square root are correctly rounded.
#include "sift_jacobi_dev.h"
#include "sift_pose_dev.h"
#include "sift_verify.h"
#include "sift_verify_dev.h"

namespace sift_amd {

namespace {

constexpr int kPoseThreads = 512, kPoseWaves = kPoseThreads / 64;
constexpr int kPoseScalars = 29;  // R1, R2, t and the two cameras of a PoseCandidates record, its leading doubles
constexpr int kPoseCounters = 9;  // fit, in front x 4, with parallax x 4

}  // namespace

__global__ __launch_bounds__(64) void k_pose_decompose(PoseCameras cams, const VerifyResult* __restrict__ result,
                                                       PoseCandidates* __restrict__ cand) {
#pragma clang fp contract(off)
    __shared__ double s_A[9], s_V[9], s_rot[4][4];
    const int pair = blockIdx.x, lane = threadIdx.x;
    result += pair, cand += pair;
    const PoseCamera cq = cams.q[pair], ct = cams.t[pair];

    // The record: empty, or a model the guided matchers would refuse, has no pose (k_refit_fit's test).
    bool usable = result->hypothesis >= 0, any = false;
    double f[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float v = result->F[i];
        usable = usable && finite_f(v);
        any = any || v != 0.f;
        f[i] = (double)v;
    }
    usable = usable && any;  // wave-uniform, as the exit below is

    PoseCandidates out;
    out.kq[0] = (double)cq.fx, out.kq[1] = (double)cq.fy, out.kq[2] = (double)cq.cx, out.kq[3] = (double)cq.cy;
    out.kt[0] = (double)ct.fx, out.kt[1] = (double)ct.fy, out.kt[2] = (double)ct.cx, out.kt[3] = (double)ct.cy;
#pragma unroll
    for (int i = 0; i < 9; i++) out.R[0][i] = 0.0, out.R[1][i] = 0.0;
    out.t[0] = 0.0, out.t[1] = 0.0, out.t[2] = 0.0;
    out.usable = 0, out.pad = 0;
    if (!usable) {
        if (lane == 0) *cand = out;
        return;
    }

    // E = Kt^T (F Kq) for skew-free cameras.
    double G[9], E[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        G[3 * r + 0] = f[3 * r + 0] * out.kq[0];
        G[3 * r + 1] = f[3 * r + 1] * out.kq[1];
        G[3 * r + 2] = (f[3 * r + 0] * out.kq[2] + f[3 * r + 1] * out.kq[3]) + f[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        E[c] = out.kt[0] * G[c];
        E[3 + c] = out.kt[1] * G[3 + c];
        E[6 + c] = (out.kt[2] * G[c] + out.kt[3] * G[3 + c]) + G[6 + c];
    }

    // N = E^T E and its eigenvectors.
    if (lane < 9) {
        const int r = lane / 3, c = lane % 3;
        double e = 0.0;
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                const double v = (E[rr] * E[cc] + E[3 + rr] * E[3 + cc]) + E[6 + rr] * E[6 + cc];
                if (rr == r && cc == c) e = v;
            }
        s_A[lane] = e;
        s_V[lane] = r == c ? 1.0 : 0.0;
    }
    wave_sync();
    (void)jacobi<3>(s_A, s_V, s_rot, lane);
    // Descending eigenvalues, ties to the lower index.
    const double d0 = s_A[0], d1 = s_A[4], d2 = s_A[8];
    int i1 = 0;
    double w1 = d0;
    if (d1 > w1) i1 = 1, w1 = d1;
    if (d2 > w1) i1 = 2, w1 = d2;
    int i2 = -1;
    double w2 = 0.0;
    if (i1 != 0) i2 = 0, w2 = d0;
    if (i1 != 1 && (i2 < 0 || d1 > w2)) i2 = 1, w2 = d1;
    if (i1 != 2 && (i2 < 0 || d2 > w2)) i2 = 2, w2 = d2;
    const double s1 = __builtin_sqrt(w1), s2 = __builtin_sqrt(w2);
    if (!(pose_finite(s2) && s2 > 0.0)) {  // rank <= 1
        if (lane == 0) *cand = out;
        return;
    }
    const double v1[3] = {s_V[i1], s_V[3 + i1], s_V[6 + i1]}, v2[3] = {s_V[i2], s_V[3 + i2], s_V[6 + i2]};
    double v3[3], u1[3], u2[3], u3[3];
    cross3(v1, v2, v3);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        u1[r] = ((E[3 * r] * v1[0] + E[3 * r + 1] * v1[1]) + E[3 * r + 2] * v1[2]) / s1;
        u2[r] = ((E[3 * r] * v2[0] + E[3 * r + 1] * v2[1]) + E[3 * r + 2] * v2[2]) / s2;
    }
    cross3(u1, u2, u3);
    // R1 = U W V^T and R2 = U W^T V^T as sums of three outer products: W permutes and negates columns.
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            out.R[0][3 * r + c] = (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
            out.R[1][3 * r + c] = (u1[r] * v2[c] - u2[r] * v1[c]) + u3[r] * v3[c];
        }
    out.t[0] = u3[0], out.t[1] = u3[1], out.t[2] = u3[2];
    out.usable = 1;
    if (lane == 0) *cand = out;
}

// mask and mask_out may be the same array: a thread reads mask[j] before it writes mask_out[j], and no other thread
// reads that byte.
template <class List>
__global__ __launch_bounds__(kPoseThreads) void k_pose_select(List list, const float4* __restrict__ pts,
                                                              const uint8_t* mask,
                                                              const PoseCandidates* __restrict__ cand, float max_depth_f,
                                                              float max_cos_f, PoseResult* __restrict__ pose,
                                                              uint8_t* mask_out, float* __restrict__ points,
                                                              MatchRecord* __restrict__ out, int* __restrict__ out_count) {
#pragma clang fp contract(off)
    __shared__ int s_cnt[kPoseWaves][kPoseCounters];
    __shared__ int s_wave[kPoseWaves];
    __shared__ double s_cand[kPoseScalars];
    if constexpr (kBatched<List>) {
        const int p = pair_of(list), row0 = row0_of(list);
        pts += row0, mask += row0, cand += p, pose += p;
        if (mask_out) mask_out += row0;
        if (points) points += 3 * (size_t)row0;
        if (out) out += row0;
        if (out_count) out_count += p;
    }
    const VerifyInput in = list_of(list);
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double max_depth = (double)max_depth_f, max_cos = (double)max_cos_f;

    // The pair's candidates, through LDS into vector registers: read as uniform scalars their 58 words crowd the
    // scalar file out.
    const bool usable = cand->usable != 0;  // workgroup-uniform
    if (tid < kPoseScalars) s_cand[tid] = reinterpret_cast<const double*>(cand)[tid];
    __syncthreads();
    double R1[9], R2[9], t[3], kq[4], kt[4];
#pragma unroll
    for (int i = 0; i < 9; i++) R1[i] = s_cand[i], R2[i] = s_cand[9 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = s_cand[18 + i];
#pragma unroll
    for (int i = 0; i < 4; i++) kq[i] = s_cand[21 + i], kt[i] = s_cand[25 + i];

    // Pass 1: the fit set's size and the four candidates' counts.
    int cnt[kPoseCounters];
#pragma unroll
    for (int k = 0; k < kPoseCounters; k++) cnt[k] = 0;
    for (int c0 = 0; c0 < n; c0 += kPoseThreads) {  // workgroup-uniform
        const int j = c0 + tid;
        bool fit = false, front[4] = {false, false, false, false}, par[4] = {false, false, false, false};
        if (j < n) {
            const float4 p = pts[j];
            fit = pose_fit(p, mask[j]);
            if (fit && usable) {
                const PoseRays x = pose_rays(p, kq, kt);
                const PoseDepths d1 = pose_depths(R1, t, x), d2 = pose_depths(R2, t, x);
                front[0] = pose_front(d1.det, d1.a, d1.b, max_depth);
                front[1] = pose_front(d2.det, d2.a, d2.b, max_depth);
                front[2] = pose_front(d1.det, -d1.a, -d1.b, max_depth);
                front[3] = pose_front(d2.det, -d2.a, -d2.b, max_depth);
                const bool c1 = d1.cosine < max_cos, c2 = d2.cosine < max_cos;
                par[0] = front[0] && c1, par[1] = front[1] && c2, par[2] = front[2] && c1, par[3] = front[3] && c2;
            }
        }
        cnt[0] += __popcll(__ballot(fit));
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cnt[1 + k] += __popcll(__ballot(front[k]));
            cnt[5 + k] += __popcll(__ballot(par[k]));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kPoseCounters; k++) s_cnt[w][k] = cnt[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPoseCounters; k++) {
        int total = 0;
#pragma unroll
        for (int i = 0; i < kPoseWaves; i++) total += s_cnt[i][k];
        cnt[k] = total;
    }

    // The winner: the most records in front, ties to the lowest index; none in front is the empty result.
    int best = 0, best_cnt = cnt[1], best_par = cnt[5];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (cnt[1 + k] > best_cnt) best = k, best_cnt = cnt[1 + k], best_par = cnt[5 + k];
    const bool empty = best_cnt == 0;
    const bool second = (best & 1) != 0, negate = best >= 2;
    if (tid == 0) {
        PoseResult r;
#pragma unroll
        for (int i = 0; i < 9; i++) r.R[i] = empty ? 0.f : (float)(second ? R2[i] : R1[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) r.t[i] = empty ? 0.f : (float)(negate ? -t[i] : t[i]);
        r.in_front = empty ? 0 : best_cnt;
        r.with_parallax = empty ? 0 : best_par;
#pragma unroll
        for (int k = 0; k < 4; k++) r.counts[k] = cnt[1 + k];
        r.candidate = empty ? -1 : best;
        r.fit = cnt[0];
        *pose = r;
    }
    if (!mask_out && !points && !out && !out_count) return;  // workgroup-uniform

    // Pass 2: the winner's mask, points and records in input order; mask bytes at and past n are 0.
    const float nan = __uint_as_float(0x7FC00000u);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int base = 0;
    for (int c0 = 0; c0 < in.cap; c0 += kPoseThreads) {  // workgroup-uniform
        const int j = c0 + tid;
        bool keep = false;
        float X[3] = {nan, nan, nan};
        if (j < n && !empty) {
            const float4 p = pts[j];
            if (pose_fit(p, mask[j])) {
                const PoseRays x = pose_rays(p, kq, kt);
                const PoseDepths d = second ? pose_depths(R2, t, x) : pose_depths(R1, t, x);
                const double a = negate ? -d.a : d.a, b = negate ? -d.b : d.b;
                keep = pose_front(d.det, a, b, max_depth);
                if (keep) X[0] = (float)(a * x.q0), X[1] = (float)(a * x.q1), X[2] = (float)a;
            }
        }
        if (j < in.cap && mask_out) mask_out[j] = keep ? 1 : 0;
        if (j < n && points) {
            points[3 * (size_t)j + 0] = X[0];
            points[3 * (size_t)j + 1] = X[1];
            points[3 * (size_t)j + 2] = X[2];
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(bal);
        __syncthreads();
        int before = 0, sum = 0;
#pragma unroll
        for (int i = 0; i < kPoseWaves; i++) {
            const int c = s_wave[i];
            before += i < w ? c : 0;
            sum += c;
        }
        if (keep && out) out[base + before + __popcll(bal & lt_mask)] = in.matches[j];
        base += sum;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0 && out_count) *out_count = base;
}

void launch_pose_decompose(const PoseCameras& cams, int P, const VerifyResult* result, PoseCandidates* cand,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_pose_decompose, dim3(P), dim3(64), 0, s, cams, result, cand);
}

template <class List>
void launch_pose_select(const List& list, const float4* pts, const uint8_t* mask, const PoseCandidates* cand,
                        float max_depth, float max_cos_parallax, PoseResult* pose, uint8_t* mask_out, float* points,
                        MatchRecord* out, int* out_count, hipStream_t s) {
    const dim3 grid(1, list_pairs(list)), block(kPoseThreads);
    hipLaunchKernelGGL((k_pose_select<List>), grid, block, 0, s, list, pts, mask, cand, max_depth, max_cos_parallax, pose,
                       mask_out, points, out, out_count);
}

#define SIFT_POSE_LAUNCHERS(List)                                                                                       \
    template void launch_pose_select<List>(const List&, const float4*, const uint8_t*, const PoseCandidates*, float,   \
                                           float, PoseResult*, uint8_t*, float*, MatchRecord*, int*, hipStream_t);
SIFT_POSE_LAUNCHERS(VerifyInput)
SIFT_POSE_LAUNCHERS(VerifyBatch)
#undef SIFT_POSE_LAUNCHERS

}  // namespace sift_amd
