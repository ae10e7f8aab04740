// Two-view verification: a fixed-budget RANSAC over a match list, on the device,
// for the fundamental matrix (sift_hip_verify_fundamental_*), the homography
// (sift_hip_verify_homography_*) and the affine map and similarity
// (sift_hip_verify_affine_*), and the projection of positions through a
// homography (sift_hip_project_homography_device).  The rules -- sampler,
// solver, score, selection -- are written out in include/sift_hip.h and
// mirrored in numpy by sift_amd.cv.ransac_fundamental / ransac_homography /
// ransac_affine.
//
//  k_verify_gather        record j -> (qx, qy, tx, ty) in scratch, NaN for a
//                         record whose index lies outside its position array:
//                         the only kernel that reads positions through a record.
//  k_verify_hypotheses    one thread per hypothesis: the counter-based draw of 8
//                         distinct matches and the normalised 8-point solve.
//                         Full pivoting indexes the 8 x 9 system by run-time
//                         row and column, so it lives in LDS laid out
//                         [entry][lane] (a lane's entries are 64 floats apart:
//                         every access of a wave is one conflict-free row).
//  k_verify_hypotheses_h  the same for the homography: 4 matches, the
//                         orientation test, the 8 x 9 DLT system through the
//                         same elimination (solve_8x9), the sign of w.
//  k_verify_hypotheses_a  the affine map (3 matches) and the similarity (2):
//                         the closed-form solve in registers, no LDS.
//  k_verify_score         the hot path, K x n predicate evaluations: one wave
//                         per hypothesis, the workgroup's waves share an
//                         LDS-staged tile of the gathered matches, lanes stride
//                         over it, ballot + popcount count, one store per
//                         hypothesis.  One body for both models: the predicate
//                         is a template parameter (SampsonPass: sift_epipolar.h's,
//                         the matcher's own; TransferPass: the forward transfer
//                         error with the chirality test; AffinePass: the
//                         same error where w is 1).
//  k_verify_select        one 1024-thread workgroup: argmax with the tie rule,
//                         the winner rescored into the mask, and the ordered
//                         compaction of k_match_select (prefix sums, no atomics:
//                         the same bytes in every run).  The same template; its key
//                         width is a parameter (the essential matrix's 10 K slots
//                         need 16 bits of index: a 64-bit key).
//  k_project_homography   one thread per position row.
// The four verify kernels are templates over the list they take.  VerifyInput:
// the single-pair call's list.  VerifyBatch (sift_hip_verify_*_batched_*): all P
// pairs of a batch in one launch, the pair is blockIdx.y, its list and
// positions come from a table passed by value, and it works on its own slices
// of the scratch with the seed `seed + p` -- the same code on the same values,
// so pair p's bytes are the single call's.  A workgroup serves one pair.
// Everything is float32 with -ffp-contract=off and correctly rounded division
// and square root: the operation order written here is the one executed.
#include <float.h>
#include <math.h>

#include <type_traits>

#include "sift_epipolar.h"
#include "sift_verify.h"
#include "sift_verify_dev.h"

namespace sift_amd {

namespace {

// Hartley normalisation of one side of a sample of M points: x, y become the
// normalised coordinates, (s, ox, oy) the similarity x' = s x + ox, (mx, my) the
// mean.
template <int M>
__device__ __forceinline__ void normalise(float (&x)[M], float (&y)[M], float& s, float& ox, float& oy, float& mx,
                                          float& my) {
#pragma clang fp contract(off)
    float sx = x[0], sy = y[0];
#pragma unroll
    for (int i = 1; i < M; i++) {
        sx = sx + x[i];
        sy = sy + y[i];
    }
    mx = sx / (float)M, my = sy / (float)M;
    float sd = 0.f;
#pragma unroll
    for (int i = 0; i < M; i++) {
        x[i] = x[i] - mx;
        y[i] = y[i] - my;
        const float d = __builtin_sqrtf(x[i] * x[i] + y[i] * y[i]);
        sd = i == 0 ? d : sd + d;
    }
    const float md = sd / (float)M;
    s = 1.41421354f / md;
#pragma unroll
    for (int i = 0; i < M; i++) {
        x[i] = x[i] * s;
        y[i] = y[i] * s;
    }
    ox = -(s * mx);
    oy = -(s * my);
}

constexpr int kHypThreads = 64;

// A lane's column of the [entry][lane] LDS arrays of the hypothesis kernels.
#define VA(r, c) A[((r) * 9 + (c)) * kHypThreads]

// The solver both models share, on one lane's 8 x 9 system A (entry e = 9 row + col at A[e * kHypThreads]), with Y
// (9 entries) and P (9 entries) its scratch: Gaussian elimination with full pivoting, back-substitution with the free
// variable 1, the column permutation undone into g.  False for a zero or non-finite pivot (g is then not written).
__device__ __forceinline__ bool solve_8x9(float* const A, float* const Y, int* const P, float (&g)[9]) {
#pragma clang fp contract(off)
    for (int c = 0; c < 9; c++) P[c * kHypThreads] = c;
    // The pivot: the largest |entry| of rows and columns >= c, the scan starting at (c, c) in row-major order and
    // moving on a strictly larger value only.
    for (int c = 0; c < 8; c++) {
        float best = __builtin_fabsf(VA(c, c));
        int pr = c, pc = c;
        for (int r = c; r < 8; r++)
            for (int j = c; j < 9; j++) {
                const float a = __builtin_fabsf(VA(r, j));
                if (a > best) best = a, pr = r, pc = j;
            }
        if (pr != c)
            for (int j = c; j < 9; j++) {
                const float t = VA(c, j);
                VA(c, j) = VA(pr, j);
                VA(pr, j) = t;
            }
        if (pc != c) {
            for (int r = 0; r < 8; r++) {
                const float t = VA(r, c);
                VA(r, c) = VA(r, pc);
                VA(r, pc) = t;
            }
            const int t = P[c * kHypThreads];
            P[c * kHypThreads] = P[pc * kHypThreads];
            P[pc * kHypThreads] = t;
        }
        const float p = VA(c, c);
        if (!(p != 0.f && finite_f(p))) return false;
        for (int r = c + 1; r < 8; r++) {
            const float m = VA(r, c) / p;
            for (int j = c + 1; j < 9; j++) VA(r, j) = VA(r, j) - m * VA(c, j);
        }
    }
    // The free variable (position 8) is 1; back-substitution, sums in ascending column order.
    Y[8 * kHypThreads] = 1.0f;
    for (int i = 7; i >= 0; i--) {
        float acc = VA(i, i + 1) * Y[(i + 1) * kHypThreads];
        for (int j = i + 2; j < 9; j++) acc = acc + VA(i, j) * Y[j * kHypThreads];
        Y[i * kHypThreads] = (-acc) / VA(i, i);
    }
    // Undo the column permutation (through the system's storage, no longer needed).
    for (int j = 0; j < 9; j++) A[P[j * kHypThreads] * kHypThreads] = Y[j * kHypThreads];
#pragma unroll
    for (int i = 0; i < 9; i++) g[i] = A[i * kHypThreads];
    return true;
}

// Scales m to unit Frobenius norm (ss summed in index order).
__device__ __forceinline__ void unit_norm(float (&m)[9]) {
#pragma clang fp contract(off)
    float ss = m[0] * m[0];
#pragma unroll
    for (int i = 1; i < 9; i++) ss = ss + m[i] * m[i];
    const float nrm = __builtin_sqrtf(ss);
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = m[i] / nrm;
}

// The signed area of the triangle (i, j, k) of a sample side, twice.
__device__ __forceinline__ float area2(const float (&x)[4], const float (&y)[4], int i, int j, int k) {
#pragma clang fp contract(off)
    return (x[j] - x[i]) * (y[k] - y[i]) - (y[j] - y[i]) * (x[k] - x[i]);
}

// The LDS of a hypothesis workgroup.  Declared here, in a plain function, not in the kernel templates: the compiler
// allocates 20,736 B per workgroup for it as declared here (one 9-entry array is optimised away, as before the
// kernels became templates) and all 23,040 B when the arrays are a template's own.
struct HypLds {
    float* a;   // the 8 x 9 system, entry e = 9 row + col of lane l at [e][l]
    float* y;   // the solution in pivot order, then in column order
    int* perm;  // the original column at each position
};
__device__ __forceinline__ HypLds hyp_lds() {
    __shared__ float s_a[72 * kHypThreads];
    __shared__ float s_y[9 * kHypThreads];
    __shared__ int s_perm[9 * kHypThreads];
    return HypLds{s_a, s_y, s_perm};
}

}  // namespace

template <class List>
__global__ __launch_bounds__(256) void k_verify_gather(List list, float4* __restrict__ pts) {
    if constexpr (kBatched<List>) pts += row0_of(list);
    const VerifyInput in = list_of(list);
    const int n = verify_n(in.count, in.cap);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const MatchRecord r = in.matches[j];
    float4 p{NAN, NAN, NAN, NAN};
    if (r.queryIdx >= 0 && r.queryIdx < in.nq && r.trainIdx >= 0 && r.trainIdx < in.nt) {
        const float* q = in.qxy + (size_t)r.queryIdx * in.qstride;
        const float* t = in.txy + (size_t)r.trainIdx * in.tstride;
        p = float4{q[0], q[1], t[0], t[1]};
    }
    pts[j] = p;
}

template <class List>
__global__ __launch_bounds__(kHypThreads) void k_verify_hypotheses(List list, const float4* __restrict__ pts, int K,
                                                                  unsigned seed, int* __restrict__ samples,
                                                                  float* __restrict__ Fout, int* __restrict__ valid) {
#pragma clang fp contract(off)
    if constexpr (kBatched<List>) {
        const size_t k0 = (size_t)K * pair_of(list);
        pts += row0_of(list), seed += (unsigned)pair_of(list), samples += 8 * k0, Fout += 9 * k0, valid += k0;
    }
    const VerifyInput in = list_of(list);
    const HypLds lds = hyp_lds();
    float* const s_a = lds.a;
    float* const s_y = lds.y;
    int* const s_perm = lds.perm;
    const int lane = threadIdx.x;
    const int k = blockIdx.x * kHypThreads + lane;
    if (k >= K) return;  // no barrier below: a lane works on its own LDS column
    const int n = verify_n(in.count, in.cap);
    float* const A = s_a + lane;

    bool ok = n >= 8;
    int pick[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pick[j] = -1;
    float g[9];
#pragma unroll
    for (int i = 0; i < 9; i++) g[i] = 0.f;
    float sq = 0.f, oqx = 0.f, oqy = 0.f, st = 0.f, otx = 0.f, oty = 0.f;
    if (ok) {
        draw<8>(seed, k, n, pick);
        float qx[8], qy[8], tx[8], ty[8], mx, my;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 p = pts[pick[j]];
            qx[j] = p.x, qy[j] = p.y, tx[j] = p.z, ty[j] = p.w;
        }
        normalise<8>(qx, qy, sq, oqx, oqy, mx, my);
        normalise<8>(tx, ty, st, otx, oty, mx, my);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            VA(r, 0) = tx[r] * qx[r];
            VA(r, 1) = tx[r] * qy[r];
            VA(r, 2) = tx[r];
            VA(r, 3) = ty[r] * qx[r];
            VA(r, 4) = ty[r] * qy[r];
            VA(r, 5) = ty[r];
            VA(r, 6) = qx[r];
            VA(r, 7) = qy[r];
            VA(r, 8) = 1.0f;
        }
        ok = solve_8x9(A, s_y + lane, s_perm + lane, g);
    }
    if (ok) {
        // F = Tt^T G Tq: H = G Tq, then F = Tt^T H.
        float H[9], F[9];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            H[3 * r + 0] = g[3 * r + 0] * sq;
            H[3 * r + 1] = g[3 * r + 1] * sq;
            H[3 * r + 2] = (g[3 * r + 0] * oqx + g[3 * r + 1] * oqy) + g[3 * r + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            F[c] = st * H[c];
            F[3 + c] = st * H[3 + c];
            F[6 + c] = (otx * H[c] + oty * H[3 + c]) + H[6 + c];
        }
        unit_norm(F);
#pragma unroll
        for (int i = 0; i < 9; i++) {
            g[i] = F[i];
            ok = ok && finite_f(g[i]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) samples[8 * (size_t)k + j] = pick[j];
#pragma unroll
    for (int i = 0; i < 9; i++) Fout[9 * (size_t)k + i] = ok ? g[i] : 0.f;
    valid[k] = ok ? 1 : 0;
}

template <class List>
__global__ __launch_bounds__(kHypThreads) void k_verify_hypotheses_h(List list, const float4* __restrict__ pts, int K,
                                                                    unsigned seed, float e2, int* __restrict__ samples,
                                                                    float* __restrict__ Hout, int* __restrict__ valid) {
#pragma clang fp contract(off)
    if constexpr (kBatched<List>) {
        const size_t k0 = (size_t)K * pair_of(list);
        pts += row0_of(list), seed += (unsigned)pair_of(list), samples += 4 * k0, Hout += 9 * k0, valid += k0;
    }
    const VerifyInput in = list_of(list);
    const HypLds lds = hyp_lds();  // as in k_verify_hypotheses
    float* const s_a = lds.a;
    float* const s_y = lds.y;
    int* const s_perm = lds.perm;
    const int lane = threadIdx.x;
    const int k = blockIdx.x * kHypThreads + lane;
    if (k >= K) return;  // no barrier below: a lane works on its own LDS column
    const int n = verify_n(in.count, in.cap);
    float* const A = s_a + lane;

    bool ok = n >= 4;
    int pick[4];
#pragma unroll
    for (int j = 0; j < 4; j++) pick[j] = -1;
    float g[9];
#pragma unroll
    for (int i = 0; i < 9; i++) g[i] = 0.f;
    float qx[4], qy[4], tx[4], ty[4];
    float4 own[4];  // the sample's raw pairs: the sign rule reads pair 0, the own-sample rule all four
#pragma unroll
    for (int j = 0; j < 4; j++) own[j] = float4{0.f, 0.f, 0.f, 0.f};
    if (ok) {
        draw<4>(seed, k, n, pick);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float4 p = pts[pick[j]];
            own[j] = p;
            qx[j] = p.x, qy[j] = p.y, tx[j] = p.z, ty[j] = p.w;
        }
        // The orientation test on the raw coordinates: every triple keeps, or every triple flips, its orientation.
        // A zero (three collinear points) or a NaN fails both.
        bool keeps = true, flips = true;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int i = t < 3 ? 0 : 1, j = t < 2 ? 1 : 2, l = t == 0 ? 2 : 3;  // (0,1,2) (0,1,3) (0,2,3) (1,2,3)
            const float p = area2(qx, qy, i, j, l) * area2(tx, ty, i, j, l);
            keeps = keeps && p > 0.f;
            flips = flips && p < 0.f;
        }
        ok = keeps || flips;
    }
    float sq = 0.f, oqx = 0.f, oqy = 0.f, st = 0.f, otx = 0.f, oty = 0.f, mqx, mqy, mtx = 0.f, mty = 0.f;
    if (ok) {
        normalise<4>(qx, qy, sq, oqx, oqy, mqx, mqy);
        normalise<4>(tx, ty, st, otx, oty, mtx, mty);
#pragma unroll
        for (int i = 0; i < 4; i++) {  // rows 2 i and 2 i + 1: pair i, (x, y) -> (u, v)
            const float x = qx[i], y = qy[i], u = tx[i], v = ty[i];
            VA(2 * i, 0) = x, VA(2 * i, 1) = y, VA(2 * i, 2) = 1.0f;
            VA(2 * i, 3) = 0.f, VA(2 * i, 4) = 0.f, VA(2 * i, 5) = 0.f;
            VA(2 * i, 6) = -(u * x), VA(2 * i, 7) = -(u * y), VA(2 * i, 8) = -u;
            VA(2 * i + 1, 0) = 0.f, VA(2 * i + 1, 1) = 0.f, VA(2 * i + 1, 2) = 0.f;
            VA(2 * i + 1, 3) = x, VA(2 * i + 1, 4) = y, VA(2 * i + 1, 5) = 1.0f;
            VA(2 * i + 1, 6) = -(v * x), VA(2 * i + 1, 7) = -(v * y), VA(2 * i + 1, 8) = -v;
        }
        ok = solve_8x9(A, s_y + lane, s_perm + lane, g);
    }
    if (ok) {
        // H = Tt^-1 G Tq: M = G Tq, then H = Tt^-1 M.
        float M[9], H[9];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            M[3 * r + 0] = g[3 * r + 0] * sq;
            M[3 * r + 1] = g[3 * r + 1] * sq;
            M[3 * r + 2] = (g[3 * r + 0] * oqx + g[3 * r + 1] * oqy) + g[3 * r + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            H[c] = M[c] / st + mtx * M[6 + c];
            H[3 + c] = M[3 + c] / st + mty * M[6 + c];
            H[6 + c] = M[6 + c];
        }
        unit_norm(H);
        // The sign that puts sample 0 in front (w > 0), so the score's chirality test means something.
        const float w0 = (H[6] * own[0].x + H[7] * own[0].y) + H[8];
        ok = w0 != 0.f;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            g[i] = w0 < 0.f ? -H[i] : H[i];
            ok = ok && finite_f(g[i]);
        }
        // The own-sample rule: a hypothesis that does not count each of its four pairs is invalid.
#pragma unroll
        for (int j = 0; j < 4; j++) ok = ok && TransferPass::pass(g, own[j], e2);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) samples[4 * (size_t)k + j] = pick[j];
#pragma unroll
    for (int i = 0; i < 9; i++) Hout[9 * (size_t)k + i] = ok ? g[i] : 0.f;
    valid[k] = ok ? 1 : 0;
}
#undef VA

// The affine map (3 matches) and the similarity (2 matches): the closed-form solve on the raw sample coordinates, all
// in registers -- no LDS, no elimination, no normalisation.  The model is {m0 .. m5, 0, 0, 1}.
template <VerifyModel Model, class List>
__global__ __launch_bounds__(kHypThreads) void k_verify_hypotheses_a(List list, const float4* __restrict__ pts, int K,
                                                                    unsigned seed, int* __restrict__ samples,
                                                                    float* __restrict__ Aout, int* __restrict__ valid) {
#pragma clang fp contract(off)
    constexpr int M = sample_size(Model);
    if constexpr (kBatched<List>) {
        const size_t k0 = (size_t)K * pair_of(list);
        pts += row0_of(list), seed += (unsigned)pair_of(list), samples += M * k0, Aout += 9 * k0, valid += k0;
    }
    const VerifyInput in = list_of(list);
    const int k = blockIdx.x * kHypThreads + threadIdx.x;
    if (k >= K) return;
    const int n = verify_n(in.count, in.cap);

    bool ok = n >= M;
    int pick[M];
#pragma unroll
    for (int j = 0; j < M; j++) pick[j] = -1;
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) {
        draw<M>(seed, k, n, pick);
        float4 p[M];
#pragma unroll
        for (int j = 0; j < M; j++) p[j] = pts[pick[j]];
        const float d1x = p[1].x - p[0].x, d1y = p[1].y - p[0].y, e1x = p[1].z - p[0].z, e1y = p[1].w - p[0].w;
        if constexpr (Model == VerifyModel::Affine) {
            const float d2x = p[2].x - p[0].x, d2y = p[2].y - p[0].y, e2x = p[2].z - p[0].z, e2y = p[2].w - p[0].w;
            const float det = d1x * d2y - d1y * d2x, dett = e1x * e2y - e1y * e2x;
            const float s = det * dett;  // zero: a collinear triple or a repeated position on either side; or a NaN
            ok = s > 0.f || s < 0.f;
            g[0] = (e1x * d2y - e2x * d1y) / det;
            g[1] = (e2x * d1x - e1x * d2x) / det;
            g[3] = (e1y * d2y - e2y * d1y) / det;
            g[4] = (e2y * d1x - e1y * d2x) / det;
        } else {
            const float den = d1x * d1x + d1y * d1y, dent = e1x * e1x + e1y * e1y;
            ok = den > 0.f && dent > 0.f;
            const float a = (d1x * e1x + d1y * e1y) / den, b = (d1x * e1y - d1y * e1x) / den;
            g[0] = a, g[1] = -b, g[3] = b, g[4] = a;
        }
        g[2] = p[0].z - (g[0] * p[0].x + g[1] * p[0].y);
        g[5] = p[0].w - (g[3] * p[0].x + g[4] * p[0].y);
#pragma unroll
        for (int i = 0; i < 6; i++) ok = ok && finite_f(g[i]);
    }
#pragma unroll
    for (int j = 0; j < M; j++) samples[M * (size_t)k + j] = pick[j];
#pragma unroll
    for (int i = 0; i < 6; i++) Aout[9 * (size_t)k + i] = ok ? g[i] : 0.f;
    Aout[9 * (size_t)k + 6] = 0.f;
    Aout[9 * (size_t)k + 7] = 0.f;
    Aout[9 * (size_t)k + 8] = ok ? 1.f : 0.f;
    valid[k] = ok ? 1 : 0;
}

constexpr int kScoreWaves = 4;    // hypotheses per workgroup
constexpr int kScoreUnroll = 4;    // matches per lane and loop iteration
constexpr int kScoreTile = 2048;   // matches per LDS tile (32 KiB): 2000 matches are one tile

template <class Pass, class List>
__global__ __launch_bounds__(64 * kScoreWaves) void k_verify_score(List list, const float4* __restrict__ pts,
                                                                   const float* __restrict__ F,
                                                                   const int* __restrict__ valid, int K, float e2,
                                                                   int* __restrict__ counts) {
    if constexpr (kBatched<List>) {
        const size_t k0 = (size_t)K * pair_of(list);
        pts += row0_of(list), F += 9 * k0, valid += k0, counts += k0;  // a batch always has valid flags
    }
    const VerifyInput in = list_of(list);
    __shared__ float4 s_pts[kScoreTile];
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = blockIdx.x * kScoreWaves + __builtin_amdgcn_readfirstlane(tid >> 6);
    // The model and the flag are loaded side by side (an invalid hypothesis' row is zero, not garbage).
    float f[9];
#pragma unroll
    for (int i = 0; i < 9; i++) f[i] = k < K ? F[9 * (size_t)k + i] : 0.f;
    const bool live = k < K && (!valid || valid[k] != 0);  // wave-uniform
    int cnt = 0;
    for (int t0 = 0; t0 < n; t0 += kScoreTile) {  // workgroup-uniform
        const int m = min(kScoreTile, n - t0);
        __syncthreads();  // the previous tile has been read
        for (int i = tid; i < m; i += 64 * kScoreWaves) s_pts[i] = pts[t0 + i];
        __syncthreads();
        if (live)
            for (int i0 = 0; i0 < m; i0 += 64 * kScoreUnroll) {  // wave-uniform
                bool pass[kScoreUnroll];  // independent matches: their arithmetic interleaves
#pragma unroll
                for (int u = 0; u < kScoreUnroll; u++) {
                    const int i = i0 + 64 * u + lane;
                    pass[u] = (i < m) & Pass::pass(f, s_pts[i < m ? i : 0], e2);  // no branch: m >= 1 here
                }
#pragma unroll
                for (int u = 0; u < kScoreUnroll; u++) cnt += __popcll(__ballot(pass[u]));
            }
    }
    if (lane == 0 && k < K) counts[k] = cnt;
}

constexpr int kVSelThreads = 1024, kVSelWaves = kVSelThreads / 64;

// kSlotBits is the width of the hypothesis index in the argmax key: 12 for the models with one slot per sample
// (K <= 4096, an int key, the code as it was before the parameter), 16 for the essential matrix's ten slots per sample
// (10 K <= 40960, a 64-bit key).
// A batch: one workgroup per pair, result and out_count its entries, out and mask (each nullable) its rows.
template <class Pass, class List, int kSlotBits = 12>
__global__ __launch_bounds__(kVSelThreads) void k_verify_select(List list, const float4* __restrict__ pts,
                                                                const float* __restrict__ F,
                                                                const int* __restrict__ valid,
                                                                const int* __restrict__ counts, int K, float e2,
                                                                VerifyResult* __restrict__ result,
                                                                MatchRecord* __restrict__ out, int* __restrict__ out_count,
                                                                uint8_t* __restrict__ mask) {
    using Key = std::conditional_t<(kSlotBits > 12), long long, int>;
    constexpr int kSlots = 1 << kSlotBits;
    __shared__ Key s_key[kVSelWaves];
    __shared__ int s_nv[kVSelWaves], s_wave[kVSelWaves];
    if constexpr (kBatched<List>) {
        const int p = pair_of(list), row0 = row0_of(list);
        const size_t k0 = (size_t)K * p;
        pts += row0, F += 9 * k0, valid += k0, counts += k0, result += p;
        if (out) out += row0;
        if (out_count) out_count += p;
        if (mask) mask += row0;
    }
    const VerifyInput in = list_of(list);
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // The winner: most inliers among the valid hypotheses, ties to the lowest k, as the largest key
    // count * 4096 + (4095 - k) (count <= 65536, k < 4096; 65536 and 65535 - k for the wide key); -1: none.
    Key key = -1;
    int nv = 0;
    for (int k = tid; k < K; k += kVSelThreads)
        if (valid[k]) {
            nv++;
            key = max(key, (Key)counts[k] * kSlots + (kSlots - 1 - k));
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        key = max(key, __shfl_xor(key, d));
        nv += __shfl_xor(nv, d);
    }
    if (lane == 0) s_key[w] = key, s_nv[w] = nv;
    __syncthreads();
    key = -1, nv = 0;
#pragma unroll
    for (int i = 0; i < kVSelWaves; i++) {
        key = max(key, s_key[i]);
        nv += s_nv[i];
    }
    const int hyp = key < 0 ? -1 : kSlots - 1 - (int)(key & (kSlots - 1));
    float f[9];
#pragma unroll
    for (int i = 0; i < 9; i++) f[i] = hyp < 0 ? 0.f : F[9 * (size_t)hyp + i];
    if (tid == 0) {
        VerifyResult r;
#pragma unroll
        for (int i = 0; i < 9; i++) r.F[i] = f[i];
        r.inliers = key < 0 ? 0 : (int)(key >> kSlotBits);
        r.hypothesis = hyp;
        r.matches = n;
        r.valid_hypotheses = nv;
        *result = r;
    }
    // The winner's inliers: the mask (every one of the cap bytes is written) and the records in input order.
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int base = 0;
    for (int c0 = 0; c0 < in.cap; c0 += kVSelThreads) {  // workgroup-uniform
        const int j = c0 + tid;
        const bool keep = hyp >= 0 && j < n && Pass::pass(f, pts[j < n ? j : 0], e2);
        if (mask && j < in.cap) mask[j] = keep ? 1 : 0;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < kVSelWaves; i++) {
            const int c = s_wave[i];
            before += i < w ? c : 0;
            total += c;
        }
        if (keep && out) out[base + before + __popcll(bal & lt_mask)] = in.matches[j];
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0 && out_count) *out_count = base;
}

// Row i of xy through H: (px / w, py / w), NaN x 2 where w is not > 0.  out may be xy itself (equal strides): a
// thread reads its row before it writes it.
__global__ __launch_bounds__(256) void k_project_homography(const float* H, const float* xy, int stride, int n,
                                                            float* out, int out_stride) {
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    float h[9];
#pragma unroll
    for (int e = 0; e < 9; e++) h[e] = H[e];
    const float x = xy[(size_t)i * stride], y = xy[(size_t)i * stride + 1];
    const float px = (h[0] * x + h[1] * y) + h[2];
    const float py = (h[3] * x + h[4] * y) + h[5];
    const float w = (h[6] * x + h[7] * y) + h[8];
    const bool front = w > 0.f;
    out[(size_t)i * out_stride] = front ? px / w : NAN;
    out[(size_t)i * out_stride + 1] = front ? py / w : NAN;
}

// The same rows rule for pair blockIdx.y of a batch: its matrix from its geometry record, its own rows.
__global__ __launch_bounds__(256) void k_project_homography_batch(const char* geometry, int geometry_stride,
                                                                  ProjectBatch batch, int stride, int out_stride) {
#pragma clang fp contract(off)
    const int p = blockIdx.y;
    const ProjectPair pr = batch.pair[p];
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)pr.n) return;
    const float* H = reinterpret_cast<const float*>(geometry + (size_t)p * geometry_stride);
    float h[9];
#pragma unroll
    for (int e = 0; e < 9; e++) h[e] = H[e];
    const float x = pr.xy[(size_t)i * stride], y = pr.xy[(size_t)i * stride + 1];
    const float px = (h[0] * x + h[1] * y) + h[2];
    const float py = (h[3] * x + h[4] * y) + h[5];
    const float w = (h[6] * x + h[7] * y) + h[8];
    const bool front = w > 0.f;
    pr.out[(size_t)i * out_stride] = front ? px / w : NAN;
    pr.out[(size_t)i * out_stride + 1] = front ? py / w : NAN;
}

// The launchers: one per step over the list type.  The grid's y and the gather's extent are the list's (list_pairs,
// list_extent), the model picks the instantiation.
template <class List>
void launch_verify_gather(const List& list, float4* pts, hipStream_t s) {
    if (list_extent(list) > 0)
        hipLaunchKernelGGL(k_verify_gather<List>, dim3((list_extent(list) + 255) / 256, list_pairs(list)), dim3(256), 0, s,
                           list, pts);
}

template <class List>
void launch_verify_hypotheses(VerifyModel model, const List& list, const float4* pts, int K, unsigned seed, float e2,
                              int* samples, float* F, int* valid, hipStream_t s) {
    const dim3 grid((K + kHypThreads - 1) / kHypThreads, list_pairs(list)), block(kHypThreads);
    if (model == VerifyModel::Homography)
        hipLaunchKernelGGL(k_verify_hypotheses_h<List>, grid, block, 0, s, list, pts, K, seed, e2, samples, F, valid);
    else if (model == VerifyModel::Affine)
        hipLaunchKernelGGL((k_verify_hypotheses_a<VerifyModel::Affine, List>), grid, block, 0, s, list, pts, K, seed,
                           samples, F, valid);
    else if (model == VerifyModel::Similarity)
        hipLaunchKernelGGL((k_verify_hypotheses_a<VerifyModel::Similarity, List>), grid, block, 0, s, list, pts, K, seed,
                           samples, F, valid);
    else
        hipLaunchKernelGGL(k_verify_hypotheses<List>, grid, block, 0, s, list, pts, K, seed, samples, F, valid);
}

template <class List>
void launch_verify_score(VerifyModel model, const List& list, const float4* pts, const float* F, const int* valid, int K,
                         float e2, int* counts, hipStream_t s) {
    const dim3 grid((K + kScoreWaves - 1) / kScoreWaves, list_pairs(list)), block(64 * kScoreWaves);
    if (model == VerifyModel::Homography)
        hipLaunchKernelGGL((k_verify_score<TransferPass, List>), grid, block, 0, s, list, pts, F, valid, K, e2, counts);
    else if (is_affine(model))
        hipLaunchKernelGGL((k_verify_score<AffinePass, List>), grid, block, 0, s, list, pts, F, valid, K, e2, counts);
    else
        hipLaunchKernelGGL((k_verify_score<SampsonPass, List>), grid, block, 0, s, list, pts, F, valid, K, e2, counts);
}

template <class List>
void launch_verify_select(VerifyModel model, const List& list, const float4* pts, const float* F, const int* valid,
                          const int* counts, int K, float e2, VerifyResult* result, MatchRecord* out, int* out_count,
                          uint8_t* mask, hipStream_t s) {
    const dim3 grid(1, list_pairs(list)), block(kVSelThreads);
    if (model == VerifyModel::Essential)
        hipLaunchKernelGGL((k_verify_select<SampsonPass, List, 16>), grid, block, 0, s, list, pts, F, valid, counts, K, e2,
                           result, out, out_count, mask);
    else if (model == VerifyModel::Homography)
        hipLaunchKernelGGL((k_verify_select<TransferPass, List>), grid, block, 0, s, list, pts, F, valid, counts, K, e2,
                           result, out, out_count, mask);
    else if (is_affine(model))
        hipLaunchKernelGGL((k_verify_select<AffinePass, List>), grid, block, 0, s, list, pts, F, valid, counts, K, e2,
                           result, out, out_count, mask);
    else
        hipLaunchKernelGGL((k_verify_select<SampsonPass, List>), grid, block, 0, s, list, pts, F, valid, counts, K, e2,
                           result, out, out_count, mask);
}

#define SIFT_VERIFY_LAUNCHERS(List)                                                                                     \
    template void launch_verify_gather<List>(const List&, float4*, hipStream_t);                                        \
    template void launch_verify_hypotheses<List>(VerifyModel, const List&, const float4*, int, unsigned, float, int*,   \
                                                 float*, int*, hipStream_t);                                            \
    template void launch_verify_score<List>(VerifyModel, const List&, const float4*, const float*, const int*, int,     \
                                            float, int*, hipStream_t);                                                  \
    template void launch_verify_select<List>(VerifyModel, const List&, const float4*, const float*, const int*,         \
                                             const int*, int, float, VerifyResult*, MatchRecord*, int*, uint8_t*,       \
                                             hipStream_t);
SIFT_VERIFY_LAUNCHERS(VerifyInput)
SIFT_VERIFY_LAUNCHERS(VerifyBatch)
#undef SIFT_VERIFY_LAUNCHERS

void launch_project_homography(const float* H, const float* xy, int stride, int n, float* out, int out_stride,
                               hipStream_t s) {
    if (n > 0)
        hipLaunchKernelGGL(k_project_homography, dim3((unsigned)(((size_t)n + 255) / 256)), dim3(256), 0, s, H, xy, stride,
                           n, out, out_stride);
}

void launch_project_homography_batched(const void* geometry, int geometry_stride, const ProjectBatch& batch, int stride,
                                       int out_stride, hipStream_t s) {
    if (batch.max_n > 0)
        hipLaunchKernelGGL(k_project_homography_batch, dim3((unsigned)(((size_t)batch.max_n + 255) / 256), batch.P),
                           dim3(256), 0, s, reinterpret_cast<const char*>(geometry), geometry_stride, batch, stride,
                           out_stride);
}

}  // namespace sift_amd
