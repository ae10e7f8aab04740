// The cyclic Jacobi routine the verifier's float64 kernels share (refit.hip: the 9 x 9 normal matrix and the 3 x 3
// rank-2 step; pose.hip: the 3 x 3 problem E^T E): one wave on a symmetric matrix in LDS.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

namespace sift_amd {

namespace {

constexpr int kRefitSweeps = 8;  // REFIT_SWEEPS of sift_amd/cv.py

// LDS written by some lanes of a wave is read by others: the writes land, and the compiler moves nothing across.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Pivot i (0 .. (M - 1) / 2 - 1) of round r of a sweep: ((r + i + 1) mod M, (r - i - 1) mod M) as p < q.  The pivots
// of a round are disjoint and index r rests (_jacobi_pivots of sift_amd/cv.py).
template <int M>
__device__ __forceinline__ void pivot(int r, int i, int& p, int& q) {
    const int a = (r + i + 1) % M, b = (r + M - i - 1) % M;
    p = min(a, b), q = max(a, b);
}

// Cyclic Jacobi by one wave on the symmetric M x M matrix A (M odd) and V = I, both in LDS, row-major: kRefitSweeps
// sweeps over the pivots in round-robin order; a pivot that is exactly 0 is skipped.  The rule applies the rotations
// one after the other.  The H = (M - 1) / 2 rotations of a round touch disjoint rows and columns, so here they run
// side by side and give the same bytes: lanes 0 .. H - 1 compute them (rot: c, s, t, a per pivot), then one lane per
// work item applies them --
//   a row of V under one pivot (M H items); a pivot's own 2 x 2 block; the resting index' two entries under one
//   pivot; and the 2 x 2 block two pivots i < j share, rotated by i, then by j, as the sequential order does.
// Returns the index of the smallest diagonal entry (ties to the lowest): column `best` of V is the eigenvector.
template <int M>
__device__ __forceinline__ int jacobi(double* const A, double* const V, double (*const rot)[4], int lane) {
#pragma clang fp contract(off)
    constexpr int H = (M - 1) / 2, kRows = M * H, kCross = H * (H - 1) / 2;
    static_assert(kRows + 2 * H + kCross <= 64 && H <= 4, "one lane per work item");
    for (int sweep = 0; sweep < kRefitSweeps; sweep++)
        for (int r = 0; r < M; r++) {
            if (lane < H) {
                int p, q;
                pivot<M>(r, lane, p, q);
                const double a = A[p * M + q];
                double c = 1.0, s = 0.0, t = 0.0;
                if (a != 0.0) {
                    const double theta = (A[q * M + q] - A[p * M + p]) / (2.0 * a);
                    const double root = __builtin_sqrt(theta * theta + 1.0);
                    t = 1.0 / (__builtin_fabs(theta) + root);
                    if (theta < 0.0) t = -t;
                    c = 1.0 / __builtin_sqrt(t * t + 1.0);
                    s = t * c;
                }
                rot[lane][0] = c, rot[lane][1] = s, rot[lane][2] = t, rot[lane][3] = a;
            }
            wave_sync();
            if (lane < kRows + 2 * H) {
                const bool row = lane < kRows, diag = !row && lane < kRows + H;
                const int i = row ? lane % H : (lane - kRows) % H;
                int p, q;
                pivot<M>(r, i, p, q);
                const double c = rot[i][0], s = rot[i][1], t = rot[i][2], a = rot[i][3];
                if (a != 0.0) {
                    if (diag) {
                        A[p * M + p] = A[p * M + p] - t * a;
                        A[q * M + q] = A[q * M + q] + t * a;
                        A[p * M + q] = 0.0, A[q * M + p] = 0.0;
                    } else {
                        double* const R = row ? V : A;
                        const int k = row ? lane / H : r;  // a row of V, or the resting index' row of A
                        const double kp = R[k * M + p], kq = R[k * M + q];
                        const double np = c * kp - s * kq, nq = s * kp + c * kq;
                        R[k * M + p] = np, R[k * M + q] = nq;
                        if (!row) A[p * M + k] = np, A[q * M + k] = nq;
                    }
                }
            } else if (lane < kRows + 2 * H + kCross) {
                const int x = lane - (kRows + 2 * H);  // (i, j), i < j: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
                const int i = x < 3 ? 0 : (x < 5 ? 1 : 2), j = x < 3 ? x + 1 : (x < 5 ? x - 1 : 3);
                int pi, qi, pj, qj;
                pivot<M>(r, i, pi, qi);
                pivot<M>(r, j, pj, qj);
                double e00 = A[pi * M + pj], e01 = A[pi * M + qj], e10 = A[qi * M + pj], e11 = A[qi * M + qj];
                if (rot[i][3] != 0.0) {  // rotation i: rows k = pj, qj, their entries in columns pi, qi
                    const double c = rot[i][0], s = rot[i][1];
                    const double n00 = c * e00 - s * e10, n10 = s * e00 + c * e10;
                    const double n01 = c * e01 - s * e11, n11 = s * e01 + c * e11;
                    e00 = n00, e10 = n10, e01 = n01, e11 = n11;
                }
                if (rot[j][3] != 0.0) {  // then rotation j: rows k = pi, qi, their entries in columns pj, qj
                    const double c = rot[j][0], s = rot[j][1];
                    const double n00 = c * e00 - s * e01, n01 = s * e00 + c * e01;
                    const double n10 = c * e10 - s * e11, n11 = s * e10 + c * e11;
                    e00 = n00, e01 = n01, e10 = n10, e11 = n11;
                }
                A[pi * M + pj] = e00, A[pj * M + pi] = e00;
                A[pi * M + qj] = e01, A[qj * M + pi] = e01;
                A[qi * M + pj] = e10, A[pj * M + qi] = e10;
                A[qi * M + qj] = e11, A[qj * M + qi] = e11;
            }
            wave_sync();
        }
    int best = 0;
    double least = A[0];
    for (int i = 1; i < M; i++) {
        const double d = A[i * M + i];
        if (d < least) least = d, best = i;
    }
    return best;
}

}  // namespace

}  // namespace sift_amd
