// The refit of a verified model on its inliers (sift_hip_refine_*): the least-squares fundamental matrix or
// homography of the records a verify call marked, rescored with the verifier's own predicate and kept when it counts
// at least as many.  The rule -- fit set, summation order, Jacobi pivots and sweeps, rank 2, denormalisation, accept --
// is written out in include/sift_hip.h and mirrored in numpy by sift_amd.cv.refit_* / refine_*.
//
//  k_refit_fit     one 256-thread workgroup per pair.  Three passes over the pair's gathered points (means, mean
//                  distances, the 45 sums of A^T A), each a per-lane sequential sum over the records j = lane mod 256
//                  in ascending j, a shuffle tree inside the wave and a fixed combination of the four waves: the
//                  rule's one summation order, no atomics.  Wave 0 then runs the Jacobi sweeps on the 9 x 9 matrix
//                  in LDS -- the four disjoint rotations of a round side by side, one lane per updated row or
//                  block (jacobi, sift_jacobi_dev.h) --, the 3 x 3 problem of the rank-2 step the same way, and the
//                  denormalisation; lane 0 writes the candidate.
//  k_refit_fit_a   the affine map and the similarity (sift_hip_refine_affine_*): the same fit set and summation order,
//                  two passes (means, the seven sums of centred products) and a closed-form solve by one thread; no
//                  Jacobi, the problem is linear and centred.  Mirrored by sift_amd.cv.refit_affine.
//  k_refit_accept  one 1024-thread workgroup per pair: the candidate's count over the n records (ballot + popcount),
//                  the accept decision, and k_verify_select's mask and ordered compaction.
// All are templates over the list, as the verify kernels are.  The fit is float64 with -ffp-contract=off: every
// operation is the one written, in the order written; float64 division and square root are correctly rounded.
#include <limits.h>

#include "sift_jacobi_dev.h"
#include "sift_verify.h"
#include "sift_verify_dev.h"

namespace sift_amd {

namespace {

constexpr int kRefitThreads = 256, kRefitWaves = kRefitThreads / 64;
constexpr int kAcceptThreads = 1024, kAcceptWaves = kAcceptThreads / 64;

__device__ __forceinline__ bool finite_d(double v) { return __builtin_fabs(v) < (double)INFINITY; }

// The halving tree of a wave's 64 slots: lane 0 returns the sum.
__device__ __forceinline__ double wave_tree(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d);
    return v;
}

// The rule's sum of N per-slot values over the workgroup's 256 slots, into every thread: (g0 + g1) + (g2 + g3) of
// the four waves' trees.  s_red is free again on return.
template <int N>
__device__ __forceinline__ void block_tree(double (&v)[N], double (*s_red)[45], int lane, int w) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < N; i++) {
        const double t = wave_tree(v[i]);
        if (lane == 0) s_red[w][i] = t;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = (s_red[0][i] + s_red[1][i]) + (s_red[2][i] + s_red[3][i]);
    __syncthreads();
}

// acc += the upper triangle of a a^T in row-major order.  lo >= 0: a's entries outside [lo, lo + 3) and [6, 9) are
// structural zeros (a homography row); their products, which add nothing to a finite sum, are not formed.
template <int lo>
__device__ __forceinline__ void add_outer(double (&acc)[45], const double (&a)[9]) {
#pragma clang fp contract(off)
    int idx = 0;
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = r; c < 9; c++, idx++) {
            const bool nz = lo < 0 || (((r >= lo && r < lo + 3) || r >= 6) && ((c >= lo && c < lo + 3) || c >= 6));
            if (nz) acc[idx] = acc[idx] + a[r] * a[c];
        }
}

template <VerifyModel Model>
constexpr int kFitMin = Model == VerifyModel::Fundamental ? 8 : 4;

}  // namespace

template <VerifyModel Model, class List>
__global__ __launch_bounds__(kRefitThreads) void k_refit_fit(List list, const float4* __restrict__ pts,
                                                            const uint8_t* __restrict__ mask,
                                                            const VerifyResult* __restrict__ result,
                                                            RefitCandidate* __restrict__ cand) {
#pragma clang fp contract(off)
    __shared__ double s_red[kRefitWaves][45];
    __shared__ int s_cnt[kRefitWaves], s_first[kRefitWaves];
    __shared__ double s_A[81], s_V[81], s_rot[4][4];
    if constexpr (kBatched<List>) {
        const int p = pair_of(list), row0 = row0_of(list);
        pts += row0, mask += row0, result += p, cand += p;
    }
    const VerifyInput in = list_of(list);
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    // The current record: empty, or a model the guided matchers would refuse, is left alone.
    bool usable = result->hypothesis >= 0, any = false;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float f = result->F[i];
        usable = usable && finite_f(f);
        any = any || f != 0.f;
    }
    usable = usable && any;

    // Pass 1: the fit set's size, first record and coordinate sums.
    int cnt = 0, first = INT_MAX;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += kRefitThreads) {
        const float4 p = pts[j];
        if (mask[j] != 0 && finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w)) {
            cnt++;
            first = min(first, j);
            sum[0] = sum[0] + (double)p.x;
            sum[1] = sum[1] + (double)p.y;
            sum[2] = sum[2] + (double)p.z;
            sum[3] = sum[3] + (double)p.w;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cnt += __shfl_xor(cnt, d);
        first = min(first, __shfl_xor(first, d));
    }
    if (lane == 0) s_cnt[w] = cnt, s_first[w] = first;
    block_tree<4>(sum, s_red, lane, w);  // its barriers publish s_cnt and s_first too
    int m = 0, j0 = INT_MAX;
#pragma unroll
    for (int i = 0; i < kRefitWaves; i++) m += s_cnt[i], j0 = min(j0, s_first[i]);

    bool ok = usable && m >= kFitMin<Model>;  // workgroup-uniform, as every exit below is
    if (!ok) {
        if (tid == 0) *cand = RefitCandidate{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0};
        return;
    }
    const double dm = (double)m;
    const double mqx = sum[0] / dm, mqy = sum[1] / dm, mtx = sum[2] / dm, mty = sum[3] / dm;

    // Pass 2: the mean distances to the means.
    double sd[2] = {0.0, 0.0};
    for (int j = tid; j < n; j += kRefitThreads) {
        const float4 p = pts[j];
        if (mask[j] != 0 && finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w)) {
            const double dx = (double)p.x - mqx, dy = (double)p.y - mqy;
            const double du = (double)p.z - mtx, dv = (double)p.w - mty;
            sd[0] = sd[0] + __builtin_sqrt(dx * dx + dy * dy);
            sd[1] = sd[1] + __builtin_sqrt(du * du + dv * dv);
        }
    }
    block_tree<2>(sd, s_red, lane, w);
    const double sq = 1.4142135623730951 / (sd[0] / dm), st = 1.4142135623730951 / (sd[1] / dm);
    if (!(finite_d(sq) && finite_d(st))) {
        if (tid == 0) *cand = RefitCandidate{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0};
        return;
    }

    // Pass 3: the 45 sums of A^T A over the rows the minimal solvers use, in normalised coordinates.
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; i++) acc[i] = 0.0;
    for (int j = tid; j < n; j += kRefitThreads) {
        const float4 p = pts[j];
        if (mask[j] != 0 && finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w)) {
            const double x = ((double)p.x - mqx) * sq, y = ((double)p.y - mqy) * sq;
            const double u = ((double)p.z - mtx) * st, v = ((double)p.w - mty) * st;
            if constexpr (Model == VerifyModel::Fundamental) {
                const double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
                add_outer<-1>(acc, a);
            } else {
                const double e[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y), -u};
                const double o[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y), -v};
                add_outer<0>(acc, e);
                add_outer<3>(acc, o);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 45; i++) {
        const double t = wave_tree(acc[i]);
        if (lane == 0) s_red[w][i] = t;
    }
    __syncthreads();
    if (w != 0) return;  // no workgroup barrier below

    // Wave 0: the matrix, its smallest eigenvector.
    for (int t = lane; t < 81; t += 64) {
        const int r = t / 9, c = t % 9, lo = min(r, c), hi = max(r, c);
        const int idx = lo * 9 - lo * (lo - 1) / 2 + (hi - lo);
        s_A[t] = (s_red[0][idx] + s_red[1][idx]) + (s_red[2][idx] + s_red[3][idx]);
        s_V[t] = r == c ? 1.0 : 0.0;
    }
    wave_sync();
    const int best = jacobi<9>(s_A, s_V, s_rot, lane);
    double g[9];
#pragma unroll
    for (int i = 0; i < 9; i++) g[i] = s_V[i * 9 + best];
    wave_sync();  // s_A and s_V are reused below

    if constexpr (Model == VerifyModel::Fundamental) {
        // Rank 2: G <- G - (G v3) v3^T, v3 the eigenvector of G^T G with the smallest eigenvalue.
        if (lane < 9) {
            const int r = lane / 3, c = lane % 3;
            double e = 0.0;
#pragma unroll
            for (int rr = 0; rr < 3; rr++)
#pragma unroll
                for (int cc = 0; cc < 3; cc++) {
                    const double v = (g[rr] * g[cc] + g[3 + rr] * g[3 + cc]) + g[6 + rr] * g[6 + cc];
                    if (rr == r && cc == c) e = v;
                }
            s_A[lane] = e;
            s_V[lane] = r == c ? 1.0 : 0.0;
        }
        wave_sync();
        const int b3 = jacobi<3>(s_A, s_V, s_rot, lane);
        const double v0 = s_V[b3], v1 = s_V[3 + b3], v2 = s_V[6 + b3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double gv = (g[3 * r] * v0 + g[3 * r + 1] * v1) + g[3 * r + 2] * v2;
            g[3 * r] = g[3 * r] - gv * v0;
            g[3 * r + 1] = g[3 * r + 1] - gv * v1;
            g[3 * r + 2] = g[3 * r + 2] - gv * v2;
        }
    }

    // Denormalise with the minimal solvers' formulas: T = G Tq, then Tt^T T (fundamental) or Tt^-1 T (homography).
    const double oqx = -(sq * mqx), oqy = -(sq * mqy);
    double T[9], R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        T[3 * r + 0] = g[3 * r + 0] * sq;
        T[3 * r + 1] = g[3 * r + 1] * sq;
        T[3 * r + 2] = (g[3 * r + 0] * oqx + g[3 * r + 1] * oqy) + g[3 * r + 2];
    }
    if constexpr (Model == VerifyModel::Fundamental) {
        const double otx = -(st * mtx), oty = -(st * mty);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            R[c] = st * T[c];
            R[3 + c] = st * T[3 + c];
            R[6 + c] = (otx * T[c] + oty * T[3 + c]) + T[6 + c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            R[c] = T[c] / st + mtx * T[6 + c];
            R[3 + c] = T[3 + c] / st + mty * T[6 + c];
            R[6 + c] = T[6 + c];
        }
    }
    double ss = R[0] * R[0];
#pragma unroll
    for (int i = 1; i < 9; i++) ss = ss + R[i] * R[i];
    const double nrm = __builtin_sqrt(ss);
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = R[i] / nrm;
    if constexpr (Model == VerifyModel::Homography) {
        // The sign that puts the first fit record in front.
        const float4 p0 = pts[j0];
        const double w0 = (R[6] * (double)p0.x + R[7] * (double)p0.y) + R[8];
        ok = w0 != 0.0;
        if (w0 < 0.0) {
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = -R[i];
        }
    }
    RefitCandidate out;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        out.m[i] = (float)R[i];
        ok = ok && finite_f(out.m[i]);
    }
    out.valid = ok ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 9; i++) out.m[i] = ok ? out.m[i] : 0.f;
    if (lane == 0) *cand = out;
}

// The affine map and the similarity: k_refit_fit's fit set and summation order, the means, the seven sums of centred
// products and the closed-form solution of the normal equations -- the problem is linear and centred, so there is no
// normalisation and no Jacobi.  Every thread holds the sums; thread 0 solves.
template <VerifyModel Model, class List>
__global__ __launch_bounds__(kRefitThreads) void k_refit_fit_a(List list, const float4* __restrict__ pts,
                                                              const uint8_t* __restrict__ mask,
                                                              const VerifyResult* __restrict__ result,
                                                              RefitCandidate* __restrict__ cand) {
#pragma clang fp contract(off)
    __shared__ double s_red[kRefitWaves][45];
    __shared__ int s_cnt[kRefitWaves];
    if constexpr (kBatched<List>) {
        const int p = pair_of(list), row0 = row0_of(list);
        pts += row0, mask += row0, result += p, cand += p;
    }
    const VerifyInput in = list_of(list);
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    // The current record: empty, or a model the guided matchers would refuse, is left alone.
    bool usable = result->hypothesis >= 0, any = false;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const float f = result->F[i];
        usable = usable && finite_f(f);
        any = any || f != 0.f;
    }
    usable = usable && any;

    // Pass 1: the fit set's size and coordinate sums.
    int cnt = 0;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += kRefitThreads) {
        const float4 p = pts[j];
        if (mask[j] != 0 && finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w)) {
            cnt++;
            sum[0] = sum[0] + (double)p.x;
            sum[1] = sum[1] + (double)p.y;
            sum[2] = sum[2] + (double)p.z;
            sum[3] = sum[3] + (double)p.w;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) s_cnt[w] = cnt;
    block_tree<4>(sum, s_red, lane, w);  // its barriers publish s_cnt too
    int m = 0;
#pragma unroll
    for (int i = 0; i < kRefitWaves; i++) m += s_cnt[i];

    const RefitCandidate none{{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0};
    if (!(usable && m >= sample_size(Model))) {  // workgroup-uniform
        if (tid == 0) *cand = none;
        return;
    }
    const double dm = (double)m;
    const double mqx = sum[0] / dm, mqy = sum[1] / dm, mtx = sum[2] / dm, mty = sum[3] / dm;

    // Pass 2: Sxx, Sxy, Syy, Txx, Txy, Tyx, Tyy of the centred coordinates.
    double S[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += kRefitThreads) {
        const float4 p = pts[j];
        if (mask[j] != 0 && finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w)) {
            const double x = (double)p.x - mqx, y = (double)p.y - mqy;
            const double u = (double)p.z - mtx, v = (double)p.w - mty;
            S[0] = S[0] + x * x;
            S[1] = S[1] + x * y;
            S[2] = S[2] + y * y;
            S[3] = S[3] + u * x;
            S[4] = S[4] + u * y;
            S[5] = S[5] + v * x;
            S[6] = S[6] + v * y;
        }
    }
    block_tree<7>(S, s_red, lane, w);
    if (tid != 0) return;  // no barrier below

    const double Sxx = S[0], Sxy = S[1], Syy = S[2], Txx = S[3], Txy = S[4], Tyx = S[5], Tyy = S[6];
    double a, b, c, d;
    bool ok;
    if constexpr (Model == VerifyModel::Affine) {
        const double det = Sxx * Syy - Sxy * Sxy;
        ok = finite_d(det) && det > 0.0;
        a = (Txx * Syy - Txy * Sxy) / det;
        b = (Txy * Sxx - Txx * Sxy) / det;
        c = (Tyx * Syy - Tyy * Sxy) / det;
        d = (Tyy * Sxx - Tyx * Sxy) / det;
    } else {
        const double den = Sxx + Syy;
        ok = finite_d(den) && den > 0.0;
        a = (Txx + Tyy) / den;
        c = (Tyx - Txy) / den;
        b = -c, d = a;
    }
    const double R[6] = {a, b, mtx - (a * mqx + b * mqy), c, d, mty - (c * mqx + d * mqy)};
    RefitCandidate out = none;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        out.m[i] = (float)R[i];
        ok = ok && finite_f(out.m[i]);
    }
    out.m[8] = 1.f;
    out.valid = 1;
    *cand = ok ? out : none;
}

template <class Pass, class List>
__global__ __launch_bounds__(kAcceptThreads) void k_refit_accept(List list, const float4* __restrict__ pts,
                                                                 const RefitCandidate* __restrict__ cand, float e2,
                                                                 VerifyResult* __restrict__ result,
                                                                 uint8_t* __restrict__ mask, MatchRecord* __restrict__ out,
                                                                 int* __restrict__ out_count, int* __restrict__ accepted,
                                                                 int first_round) {
    __shared__ int s_wave[kAcceptWaves];
    if constexpr (kBatched<List>) {
        const int p = pair_of(list), row0 = row0_of(list);
        pts += row0, cand += p, result += p, mask += row0;
        if (out) out += row0;
        if (out_count) out_count += p;
        if (accepted) accepted += p;
    }
    const VerifyInput in = list_of(list);
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float f[9];
#pragma unroll
    for (int i = 0; i < 9; i++) f[i] = cand->m[i];
    const bool valid = cand->valid != 0;
    const int current = result->inliers;  // read by every thread before thread 0 may write it (behind the barrier)

    // The candidate's count over all n records.
    int cnt = 0;
    if (valid)
        for (int c0 = 0; c0 < n; c0 += kAcceptThreads) {  // workgroup-uniform
            const int j = c0 + tid;
            cnt += __popcll(__ballot(j < n && Pass::pass(f, pts[j < n ? j : 0], e2)));
        }
    if (lane == 0) s_wave[w] = cnt;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int i = 0; i < kAcceptWaves; i++) total += s_wave[i];
    __syncthreads();  // s_wave is rewritten below
    const bool accept = valid && total >= current;
    if (tid == 0) {
        if (accept) {
#pragma unroll
            for (int i = 0; i < 9; i++) result->F[i] = f[i];
            result->inliers = total;
        }
        if (accepted) *accepted = (first_round ? 0 : *accepted) + (accept ? 1 : 0);
    }
    if (!accept && !out && !out_count) return;  // workgroup-uniform

    // The mask as it now stands -- the candidate's on an accepted round -- and its records in input order.
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += kAcceptThreads) {  // workgroup-uniform
        const int j = c0 + tid;
        bool keep = false;
        if (j < n) {
            keep = accept ? Pass::pass(f, pts[j], e2) : mask[j] != 0;
            if (accept) mask[j] = keep ? 1 : 0;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(bal);
        __syncthreads();
        int before = 0, sum = 0;
#pragma unroll
        for (int i = 0; i < kAcceptWaves; i++) {
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

// The launchers: one workgroup per pair (list_pairs), the model picks the instantiation.
template <class List>
void launch_refit_fit(VerifyModel model, const List& list, const float4* pts, const uint8_t* mask,
                      const VerifyResult* result, RefitCandidate* cand, hipStream_t s) {
    const dim3 grid(1, list_pairs(list)), block(kRefitThreads);
    if (model == VerifyModel::Homography)
        hipLaunchKernelGGL((k_refit_fit<VerifyModel::Homography, List>), grid, block, 0, s, list, pts, mask, result, cand);
    else if (model == VerifyModel::Affine)
        hipLaunchKernelGGL((k_refit_fit_a<VerifyModel::Affine, List>), grid, block, 0, s, list, pts, mask, result, cand);
    else if (model == VerifyModel::Similarity)
        hipLaunchKernelGGL((k_refit_fit_a<VerifyModel::Similarity, List>), grid, block, 0, s, list, pts, mask, result,
                           cand);
    else
        hipLaunchKernelGGL((k_refit_fit<VerifyModel::Fundamental, List>), grid, block, 0, s, list, pts, mask, result, cand);
}

template <class List>
void launch_refit_accept(VerifyModel model, const List& list, const float4* pts, const RefitCandidate* cand, float e2,
                         VerifyResult* result, uint8_t* mask, MatchRecord* out, int* out_count, int* accepted,
                         bool first_round, hipStream_t s) {
    const dim3 grid(1, list_pairs(list)), block(kAcceptThreads);
    if (model == VerifyModel::Homography)
        hipLaunchKernelGGL((k_refit_accept<TransferPass, List>), grid, block, 0, s, list, pts, cand, e2, result, mask, out,
                           out_count, accepted, first_round ? 1 : 0);
    else if (is_affine(model))
        hipLaunchKernelGGL((k_refit_accept<AffinePass, List>), grid, block, 0, s, list, pts, cand, e2, result, mask, out,
                           out_count, accepted, first_round ? 1 : 0);
    else
        hipLaunchKernelGGL((k_refit_accept<SampsonPass, List>), grid, block, 0, s, list, pts, cand, e2, result, mask, out,
                           out_count, accepted, first_round ? 1 : 0);
}

#define SIFT_REFIT_LAUNCHERS(List)                                                                                  \
    template void launch_refit_fit<List>(VerifyModel, const List&, const float4*, const uint8_t*, const VerifyResult*, \
                                         RefitCandidate*, hipStream_t);                                             \
    template void launch_refit_accept<List>(VerifyModel, const List&, const float4*, const RefitCandidate*, float,   \
                                            VerifyResult*, uint8_t*, MatchRecord*, int*, int*, bool, hipStream_t);
SIFT_REFIT_LAUNCHERS(VerifyInput)
SIFT_REFIT_LAUNCHERS(VerifyBatch)
#undef SIFT_REFIT_LAUNCHERS

}  // namespace sift_amd
