// The relative pose from a verified homography (sift_hip_recover_pose_homography_*): A = Kt^-1 H Kq, its four
// (R, t, n, distance) candidates (Ma, Soatto, Kosecka, Sastry, 5.3.3), the depths of the fit records under each and the
// candidate that puts the most of them in front of both cameras -- cv::decomposeHomographyMat and
// cv::filterHomographyDecompByVisibleRefpoints on the verifier's record, mask and gathered list.  The rule is written
// out in include/sift_hip.h and mirrored in numpy by sift_amd.cv.recover_pose_homography.
//
//  k_plane_decompose  one wave per pair: the record's usability, A, S = A^T A, the refit's Jacobi routine on S in LDS
//                     (jacobi<3>), u+ and u- from the eigenvalues, and per u the rotation, the translation, the normal
//                     and the distance into the pair's scratch record; the four candidates as float32 on request.
//  k_plane_select     one 512-thread workgroup per pair: k_pose_select (pose.hip) with a translation per rotation and
//                     w > 0 under H in the fit test.  Negating t negates both depths exactly, so the four candidates
//                     cost two evaluations.  Integer counts by ballot and popcount, exact in any order, no atomics.
// Float64 with -ffp-contract=off: every operation is the one written, in the order written; float64 division and
// square root are correctly rounded.
#include "sift_jacobi_dev.h"
#include "sift_pose_dev.h"
#include "sift_verify.h"
#include "sift_verify_dev.h"

namespace sift_amd {

namespace {

constexpr int kPlaneThreads = 512, kPlaneWaves = kPlaneThreads / 64;
constexpr int kPlaneScalars = 43;      // a PlaneCandidates record's doubles
constexpr int kPlaneLoopScalars = 35;  // of which the record loop needs R+, R-, t+, t-, the two cameras and h3
constexpr int kPlaneCounters = 9;      // fit, in front x 4, with parallax x 4

// The fit test of the plane pose rule: the refit's set, and in front of the camera under H as it is signed.
__device__ __forceinline__ bool plane_fit(const float4 p, uint8_t m, const double (&h3)[3]) {
#pragma clang fp contract(off)
    const double w = (h3[0] * (double)p.x + h3[1] * (double)p.y) + h3[2];
    return pose_fit(p, m) && w > 0.0;
}

}  // namespace

__global__ __launch_bounds__(64) void k_plane_decompose(PoseCameras cams, const VerifyResult* __restrict__ result,
                                                        PlaneCandidates* __restrict__ cand,
                                                        PlaneCandidate* __restrict__ candidates) {
#pragma clang fp contract(off)
    __shared__ double s_A[9], s_V[9], s_rot[4][4];
    const int pair = blockIdx.x, lane = threadIdx.x;
    result += pair, cand += pair;
    if (candidates) candidates += 4 * pair;
    const PoseCamera cq = cams.q[pair], ct = cams.t[pair];

    // The record: empty, or a model the guided matchers would refuse, has no pose (k_refit_fit's test).
    bool usable = result->hypothesis >= 0, any = false;
    double h[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float v = result->F[i];
        usable = usable && finite_f(v);
        any = any || v != 0.f;
        h[i] = (double)v;
    }
    usable = usable && any;  // wave-uniform, as the exits below are

    PlaneCandidates out;
    out.kq[0] = (double)cq.fx, out.kq[1] = (double)cq.fy, out.kq[2] = (double)cq.cx, out.kq[3] = (double)cq.cy;
    out.kt[0] = (double)ct.fx, out.kt[1] = (double)ct.fy, out.kt[2] = (double)ct.cx, out.kt[3] = (double)ct.cy;
    out.h3[0] = h[6], out.h3[1] = h[7], out.h3[2] = h[8];
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
        for (int i = 0; i < 9; i++) out.R[k][i] = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) out.t[k][i] = 0.0, out.N[k][i] = 0.0;
        out.distance[k] = 0.0;
    }
    out.usable = 0, out.pad = 0;
    // No decomposition: the scratch record says so and the candidates are zero.
    const auto none = [&] {
        if (lane == 0) *cand = out;
        if (candidates && lane < 64) reinterpret_cast<float*>(candidates)[lane] = 0.f;  // 4 x 16 floats
    };
    if (!usable) {
        none();
        return;
    }

    // A = Kt^-1 (H Kq) for skew-free cameras.
    double G[9], A[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        G[3 * r + 0] = h[3 * r + 0] * out.kq[0];
        G[3 * r + 1] = h[3 * r + 1] * out.kq[1];
        G[3 * r + 2] = (h[3 * r + 0] * out.kq[2] + h[3 * r + 1] * out.kq[3]) + h[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        A[c] = (G[c] - out.kt[2] * G[6 + c]) / out.kt[0];
        A[3 + c] = (G[3 + c] - out.kt[3] * G[6 + c]) / out.kt[1];
        A[6 + c] = G[6 + c];
    }

    // S = A^T A and its eigenvectors.
    if (lane < 9) {
        const int r = lane / 3, c = lane % 3;
        double e = 0.0;
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                const double v = (A[rr] * A[cc] + A[3 + rr] * A[3 + cc]) + A[6 + rr] * A[6 + cc];
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
    const int i3 = 3 - i1 - i2;
    const double w3 = i3 == 0 ? d0 : (i3 == 1 ? d1 : d2);
    const double span = w1 - w3;
    if (!(pose_finite(w2) && w2 > 0.0) || !(span > 0.0)) {  // rank <= 1, or no spread to split
        none();
        return;
    }
    const double s = __builtin_sqrt(w2);
    double Hn[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Hn[i] = A[i] / s;
    double d23 = w2 - w3, d12 = w1 - w2;
    d23 = d23 > 0.0 ? d23 : 0.0;
    d12 = d12 > 0.0 ? d12 : 0.0;
    const double a = __builtin_sqrt(d23 / span), b = __builtin_sqrt(d12 / span);
    const double v1[3] = {s_V[i1], s_V[3 + i1], s_V[6 + i1]}, v2[3] = {s_V[i2], s_V[3 + i2], s_V[6 + i2]};
    double v3[3];
    cross3(v1, v2, v3);

    bool ok = true;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        double u[3], N[3], hv[3], hu[3], hc[3], T[3];
#pragma unroll
        for (int i = 0; i < 3; i++) u[i] = k == 0 ? a * v1[i] + b * v3[i] : a * v1[i] - b * v3[i];
        cross3(v2, u, N);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            hv[r] = (Hn[3 * r] * v2[0] + Hn[3 * r + 1] * v2[1]) + Hn[3 * r + 2] * v2[2];
            hu[r] = (Hn[3 * r] * u[0] + Hn[3 * r + 1] * u[1]) + Hn[3 * r + 2] * u[2];
        }
        cross3(hv, hu, hc);
        // R = W U^T as a sum of three outer products, T = (Hn - R) N.
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) out.R[k][3 * r + c] = (hv[r] * v2[c] + hu[r] * u[c]) + hc[r] * N[c];
#pragma unroll
        for (int r = 0; r < 3; r++)
            T[r] = ((Hn[3 * r] - out.R[k][3 * r]) * N[0] + (Hn[3 * r + 1] - out.R[k][3 * r + 1]) * N[1]) +
                   (Hn[3 * r + 2] - out.R[k][3 * r + 2]) * N[2];
        const double norm = __builtin_sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2]);
        ok = ok && pose_finite(norm) && norm > 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) out.t[k][i] = T[i] / norm, out.N[k][i] = N[i];
        out.distance[k] = 1.0 / norm;
    }
    if (!ok) {  // a translation without a length: zero the record again
#pragma unroll
        for (int k = 0; k < 2; k++) {
#pragma unroll
            for (int i = 0; i < 9; i++) out.R[k][i] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) out.t[k][i] = 0.0, out.N[k][i] = 0.0;
            out.distance[k] = 0.0;
        }
        none();
        return;
    }
    out.usable = 1;
    if (lane == 0) {
        *cand = out;
        if (candidates) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                PlaneCandidate c;
#pragma unroll
                for (int i = 0; i < 9; i++) c.R[i] = (float)out.R[k & 1][i];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    c.t[i] = (float)(k >= 2 ? -out.t[k & 1][i] : out.t[k & 1][i]);
                    c.normal[i] = (float)(k >= 2 ? -out.N[k & 1][i] : out.N[k & 1][i]);
                }
                c.distance = (float)out.distance[k & 1];
                candidates[k] = c;
            }
        }
    }
}

// mask and mask_out may be the same array: a thread reads mask[j] before it writes mask_out[j], and no other thread
// reads that byte.
template <class List>
__global__ __launch_bounds__(kPlaneThreads) void k_plane_select(List list, const float4* __restrict__ pts,
                                                                const uint8_t* mask,
                                                                const PlaneCandidates* __restrict__ cand,
                                                                float max_depth_f, float max_cos_f,
                                                                PlanePoseResult* __restrict__ pose, uint8_t* mask_out,
                                                                float* __restrict__ points, MatchRecord* __restrict__ out,
                                                                int* __restrict__ out_count) {
#pragma clang fp contract(off)
    __shared__ int s_cnt[kPlaneWaves][kPlaneCounters];
    __shared__ int s_wave[kPlaneWaves];
    __shared__ double s_cand[kPlaneScalars];
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

    // The pair's candidates, through LDS into vector registers: read as uniform scalars their words crowd the scalar
    // file out (k_pose_select).
    const bool usable = cand->usable != 0;  // workgroup-uniform
    if (tid < kPlaneScalars) s_cand[tid] = reinterpret_cast<const double*>(cand)[tid];
    __syncthreads();
    double R1[9], R2[9], t1[3], t2[3], kq[4], kt[4], h3[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R1[i] = s_cand[i], R2[i] = s_cand[9 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) t1[i] = s_cand[18 + i], t2[i] = s_cand[21 + i], h3[i] = s_cand[32 + i];
#pragma unroll
    for (int i = 0; i < 4; i++) kq[i] = s_cand[24 + i], kt[i] = s_cand[28 + i];
    static_assert(kPlaneLoopScalars == 35 && offsetof(PlaneCandidates, h3) == 32 * sizeof(double) &&
                      offsetof(PlaneCandidates, N) == 35 * sizeof(double),
                  "the record's doubles as read here");

    // Pass 1: the fit set's size and the four candidates' counts.
    int cnt[kPlaneCounters];
#pragma unroll
    for (int k = 0; k < kPlaneCounters; k++) cnt[k] = 0;
    for (int c0 = 0; c0 < n; c0 += kPlaneThreads) {  // workgroup-uniform
        const int j = c0 + tid;
        bool fit = false, front[4] = {false, false, false, false}, par[4] = {false, false, false, false};
        if (j < n) {
            const float4 p = pts[j];
            fit = plane_fit(p, mask[j], h3);
            if (fit && usable) {
                const PoseRays x = pose_rays(p, kq, kt);
                const PoseDepths d1 = pose_depths(R1, t1, x), d2 = pose_depths(R2, t2, x);
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
        for (int k = 0; k < kPlaneCounters; k++) s_cnt[w][k] = cnt[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPlaneCounters; k++) {
        int total = 0;
#pragma unroll
        for (int i = 0; i < kPlaneWaves; i++) total += s_cnt[i][k];
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
        PlanePoseResult r;
#pragma unroll
        for (int i = 0; i < 9; i++) r.pose.R[i] = empty ? 0.f : (float)(second ? R2[i] : R1[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double ti = second ? t2[i] : t1[i], ni = s_cand[35 + (second ? 3 : 0) + i];
            r.pose.t[i] = empty ? 0.f : (float)(negate ? -ti : ti);
            r.normal[i] = empty ? 0.f : (float)(negate ? -ni : ni);
        }
        r.distance = empty ? 0.f : (float)s_cand[41 + (second ? 1 : 0)];
        r.pose.in_front = empty ? 0 : best_cnt;
        r.pose.with_parallax = empty ? 0 : best_par;
#pragma unroll
        for (int k = 0; k < 4; k++) r.pose.counts[k] = cnt[1 + k];
        r.pose.candidate = empty ? -1 : best;
        r.pose.fit = cnt[0];
        *pose = r;
    }
    if (!mask_out && !points && !out && !out_count) return;  // workgroup-uniform

    // Pass 2: the winner's mask, points and records in input order; mask bytes at and past n are 0.
    const float nan = __uint_as_float(0x7FC00000u);
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int base = 0;
    for (int c0 = 0; c0 < in.cap; c0 += kPlaneThreads) {  // workgroup-uniform
        const int j = c0 + tid;
        bool keep = false;
        float X[3] = {nan, nan, nan};
        if (j < n && !empty) {
            const float4 p = pts[j];
            if (plane_fit(p, mask[j], h3)) {
                const PoseRays x = pose_rays(p, kq, kt);
                const PoseDepths d = second ? pose_depths(R2, t2, x) : pose_depths(R1, t1, x);
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
        for (int i = 0; i < kPlaneWaves; i++) {
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

void launch_plane_decompose(const PoseCameras& cams, int P, const VerifyResult* result, PlaneCandidates* cand,
                            PlaneCandidate* candidates, hipStream_t s) {
    hipLaunchKernelGGL(k_plane_decompose, dim3(P), dim3(64), 0, s, cams, result, cand, candidates);
}

template <class List>
void launch_plane_select(const List& list, const float4* pts, const uint8_t* mask, const PlaneCandidates* cand,
                         float max_depth, float max_cos_parallax, PlanePoseResult* pose, uint8_t* mask_out, float* points,
                         MatchRecord* out, int* out_count, hipStream_t s) {
    const dim3 grid(1, list_pairs(list)), block(kPlaneThreads);
    hipLaunchKernelGGL((k_plane_select<List>), grid, block, 0, s, list, pts, mask, cand, max_depth, max_cos_parallax,
                       pose, mask_out, points, out, out_count);
}

#define SIFT_PLANE_LAUNCHERS(List)                                                                                     \
    template void launch_plane_select<List>(const List&, const float4*, const uint8_t*, const PlaneCandidates*, float, \
                                            float, PlanePoseResult*, uint8_t*, float*, MatchRecord*, int*, hipStream_t);
SIFT_PLANE_LAUNCHERS(VerifyInput)
SIFT_PLANE_LAUNCHERS(VerifyBatch)
#undef SIFT_PLANE_LAUNCHERS

}  // namespace sift_amd
