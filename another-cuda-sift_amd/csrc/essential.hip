// Essential-matrix hypotheses: the 5-point minimal solver of sift_hip_verify_essential_* (the rule is written out in
// include/sift_hip.h, "Essential-matrix verification", and mirrored in numpy by sift_amd.cv.essential_from_5).
//
//  k_verify_hypotheses_e  one lane per sample: the counter-based draw of 5 distinct matches, the calibrated rays, the
//                         null space of the 5 x 9 system, the ten cubic constraints, their reduction, the degree-10
//                         polynomial in z, its real roots by the derivative chain, and per root the pixel-space
//                         F = Kt^-T E Kq^-1 of unit norm into the sample's ten model slots.
// Everything is float64 with -ffp-contract=off; division and square root are correctly rounded and nothing else is
// called, so the operation order written here is the one executed and the device's bytes are the mirror's.
//
// Where the numbers live.  The two eliminations pick their pivots at run time, so their systems are indexed by
// run-time row and column and live in LDS laid out [entry][lane], as solve_8x9's system does: a lane's entries are
// kEssThreads doubles apart and every access of the workgroup is one conflict-free row.  The storage is staged -- the
// 5 x 9 system and the basis it yields (81 entries) are dead before the 10 x 20 constraint matrix (200 entries) is
// written over them.  Everything else -- the polynomial products, the derivative chain, the brackets -- is unrolled
// at compile time and indexed by constants only, so it lives in registers.  A workgroup is 32 lanes: 200 x 32 doubles
// are 51,200 B (52,352 B with the permutation), under the 64 KiB a workgroup may take without opting in, and three fit
// a CU's 160 KiB; the registers (256 VGPRs and 62 AGPRs: one wave per SIMD) would allow four.  A 32-lane workgroup
// leaves half of its wave64 idle; 64 lanes would need 104,704 B of LDS, one workgroup per CU and 64 resident samples
// where this shape has 96, so the half-empty wave is the cheaper one.  The kernel is small and latency-bound (K = 256
// samples are eight workgroups); occupancy is not what it needs.
#include <float.h>
#include <math.h>

#include <type_traits>

#include "sift_verify.h"
#include "sift_verify_dev.h"

namespace sift_amd {

namespace {

constexpr int kEssThreads = 32;
constexpr int kEssBisections = 48;  // per bracket with a sign change
constexpr int kEssNewton = 3;       // after them, each step kept only inside the bracket

__device__ __forceinline__ bool finite_d(double v) { return __builtin_fabs(v) < (double)INFINITY; }

// A lane's column of the [entry][lane] LDS array: the 5 x 9 system, the four basis vectors behind it, and the
// 10 x 20 constraint matrix over both.
#define EA(r, c) M[((r) * 9 + (c)) * kEssThreads]
#define EB(f, i) M[(45 + (f) * 9 + (i)) * kEssThreads]
#define EM(r, c) M[((r) * 20 + (c)) * kEssThreads]

// The null space of the 5 x 9 system at EA: Gauss-Jordan with full pivoting (solve_8x9's scan and tie rule), then the
// four solutions with one free variable (positions 5 .. 8) set to 1 and the others to 0, the column permutation undone,
// at EB(f, .).  False for a zero or non-finite pivot.
__device__ __forceinline__ bool ess_null_space(double* const M, int* const P) {
#pragma clang fp contract(off)
    for (int c = 0; c < 9; c++) P[c * kEssThreads] = c;
    for (int c = 0; c < 5; c++) {
        double best = __builtin_fabs(EA(c, c));
        int pr = c, pc = c;
        for (int r = c; r < 5; r++)
            for (int j = c; j < 9; j++) {
                const double a = __builtin_fabs(EA(r, j));
                if (a > best) best = a, pr = r, pc = j;
            }
        if (pr != c)
            for (int j = c; j < 9; j++) {
                const double t = EA(c, j);
                EA(c, j) = EA(pr, j);
                EA(pr, j) = t;
            }
        if (pc != c) {
            for (int r = 0; r < 5; r++) {
                const double t = EA(r, c);
                EA(r, c) = EA(r, pc);
                EA(r, pc) = t;
            }
            const int t = P[c * kEssThreads];
            P[c * kEssThreads] = P[pc * kEssThreads];
            P[pc * kEssThreads] = t;
        }
        const double p = EA(c, c);
        if (!(p != 0.0 && finite_d(p))) return false;
        for (int r = 0; r < 5; r++) {
            if (r == c) continue;
            const double m = EA(r, c) / p;
            for (int j = c + 1; j < 9; j++) EA(r, j) = EA(r, j) - m * EA(c, j);
        }
    }
    for (int f = 0; f < 4; f++)
        for (int j = 0; j < 9; j++) {
            const double y = j < 5 ? (-EA(j, 5 + f)) / EA(j, j) : (j == 5 + f ? 1.0 : 0.0);
            EB(f, P[j * kEssThreads]) = y;
        }
    return true;
}

// Products of the constraint polynomials.  The variables are 0 = x, 1 = y, 2 = z, 3 = 1; a quadratic's coefficients
// are those of the pairs i <= j in lexicographic order, a cubic's are in Nister's column order
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
// Every coefficient is summed from zero in loop order.
__device__ __forceinline__ void ess_mul11(const double (&a)[4], const double (&b)[4], double (&c)[10]) {
#pragma clang fp contract(off)
    constexpr int T2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
#pragma unroll
    for (int i = 0; i < 10; i++) c[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) c[T2[i][j]] = c[T2[i][j]] + a[i] * b[j];
}

__device__ __forceinline__ void ess_mul21(const double (&a)[10], const double (&b)[4], double (&c)[20]) {
#pragma clang fp contract(off)
    constexpr int T3[10][4] = {{0, 2, 4, 5},     {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},  {3, 1, 6, 7},
                               {8, 6, 13, 14},   {9, 7, 14, 15},   {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
    for (int i = 0; i < 20; i++) c[i] = 0.0;
#pragma unroll
    for (int m = 0; m < 10; m++)
#pragma unroll
        for (int k = 0; k < 4; k++) c[T3[m][k]] = c[T3[m][k]] + a[m] * b[k];
}

// a b - c d on quadratics from linear polynomials.
__device__ __forceinline__ void ess_minor(const double (&a)[4], const double (&b)[4], const double (&c)[4],
                                          const double (&d)[4], double (&out)[10]) {
#pragma clang fp contract(off)
    double u[10], v[10];
    ess_mul11(a, b, u);
    ess_mul11(c, d, v);
#pragma unroll
    for (int i = 0; i < 10; i++) out[i] = u[i] - v[i];
}

// Row `row` of the constraint matrix: (a0 b0 + s a1 b1) + a2 b2, s = -1 for the determinant and +1 otherwise.
template <bool kDet>
__device__ __forceinline__ void ess_row(double* const M, int row, const double (&a0)[10], const double (&b0)[4],
                                        const double (&a1)[10], const double (&b1)[4], const double (&a2)[10],
                                        const double (&b2)[4]) {
#pragma clang fp contract(off)
    double u[20], v[20], w[20];
    ess_mul21(a0, b0, u);
    ess_mul21(a1, b1, v);
    ess_mul21(a2, b2, w);
#pragma unroll
    for (int i = 0; i < 20; i++) EM(row, i) = (kDet ? u[i] - v[i] : u[i] + v[i]) + w[i];
}

// The ten cubic constraints of E = x X + y Y + z Z + W, e[i] the linear polynomial of entry i (row-major): det E = 0
// in row 0, the entries of (E E^T - tr(E E^T) / 2) E = 0 in rows 1 .. 9.
__device__ __forceinline__ void ess_constraints(double* const M, const double (&e)[9][4]) {
#pragma clang fp contract(off)
    {
        double m0[10], m1[10], m2[10];
        ess_minor(e[4], e[8], e[5], e[7], m0);
        ess_minor(e[3], e[8], e[5], e[6], m1);
        ess_minor(e[3], e[7], e[4], e[6], m2);
        ess_row<true>(M, 0, m0, e[0], m1, e[1], m2, e[2]);
    }
    double G[3][3][10];  // E E^T, the lower triangle a copy of the upper
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) {
            double u[10], v[10], w[10];
            ess_mul11(e[3 * i], e[3 * j], u);
            ess_mul11(e[3 * i + 1], e[3 * j + 1], v);
            ess_mul11(e[3 * i + 2], e[3 * j + 2], w);
#pragma unroll
            for (int k = 0; k < 10; k++) G[i][j][k] = (u[k] + v[k]) + w[k], G[j][i][k] = G[i][j][k];
        }
#pragma unroll
    for (int k = 0; k < 10; k++) {
        const double half = 0.5 * ((G[0][0][k] + G[1][1][k]) + G[2][2][k]);
        G[0][0][k] = G[0][0][k] - half;
        G[1][1][k] = G[1][1][k] - half;
        G[2][2][k] = G[2][2][k] - half;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) ess_row<false>(M, 1 + 3 * i + j, G[i][0], e[j], G[i][1], e[3 + j], G[i][2], e[6 + j]);
}

// Gauss-Jordan on the first ten columns of the constraint matrix with row pivoting: the largest |entry| of column c in
// rows >= c, the scan starting at row c and moving on a strictly larger value only.  False for a zero or non-finite
// pivot.
__device__ __forceinline__ bool ess_reduce(double* const M) {
#pragma clang fp contract(off)
    for (int c = 0; c < 10; c++) {
        double best = __builtin_fabs(EM(c, c));
        int pr = c;
        for (int r = c + 1; r < 10; r++) {
            const double a = __builtin_fabs(EM(r, c));
            if (a > best) best = a, pr = r;
        }
        if (pr != c)
            for (int j = c; j < 20; j++) {
                const double t = EM(c, j);
                EM(c, j) = EM(pr, j);
                EM(pr, j) = t;
            }
        const double p = EM(c, c);
        if (!(p != 0.0 && finite_d(p))) return false;
        for (int r = 0; r < 10; r++) {
            if (r == c) continue;
            const double m = EM(r, c) / p;
            for (int j = c + 1; j < 20; j++) EM(r, j) = EM(r, j) - m * EM(c, j);
        }
    }
    return true;
}

// Polynomials in z, coefficients ascending.
template <int LA, int LB>
__device__ __forceinline__ void ess_conv(const double (&a)[LA], const double (&b)[LB], double (&c)[LA + LB - 1]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < LA + LB - 1; i++) c[i] = 0.0;
#pragma unroll
    for (int i = 0; i < LA; i++)
#pragma unroll
        for (int j = 0; j < LB; j++) c[i + j] = c[i + j] + a[i] * b[j];
}

// (a b - c d) e.
template <int LA, int LB, int LC, int LD, int LE>
__device__ __forceinline__ void ess_minor_times(const double (&a)[LA], const double (&b)[LB], const double (&c)[LC],
                                                const double (&d)[LD], const double (&e)[LE], double (&out)[11]) {
#pragma clang fp contract(off)
    static_assert(LA + LB == LC + LD && LA + LB - 1 + LE - 1 == 11, "a term of the degree-10 determinant");
    double u[LA + LB - 1], v[LA + LB - 1];
    ess_conv(a, b, u);
    ess_conv(c, d, v);
#pragma unroll
    for (int i = 0; i < LA + LB - 1; i++) u[i] = u[i] - v[i];
    ess_conv(u, e, out);
}

template <int D>
__device__ __forceinline__ double ess_horner(const double (&c)[D + 1], double z) {
#pragma clang fp contract(off)
    double acc = c[D];
#pragma unroll
    for (int k = D - 1; k >= 0; k--) acc = acc * z + c[k];
    return acc;
}

// Horner's value where z is finite; at z = -inf / +inf a value with the polynomial's sign there.
template <int D>
__device__ __forceinline__ double ess_value(const double (&c)[D + 1], double z) {
    if (z == -(double)INFINITY) return (D % 2) ? -c[D] : c[D];
    if (z == (double)INFINITY) return c[D];
    return ess_horner<D>(c, z);
}

// The point of the real line that s in [-1, 1] stands for.
__device__ __forceinline__ double ess_z(double s) {
#pragma clang fp contract(off)
    return s / (1.0 - __builtin_fabs(s));
}

// The derivative chain.  run() takes the polynomial c of degree D and returns the D + 2 nodes -inf, the D bracket
// results, +inf (as s in [-1, 1] and as z = s / (1 - |s|)), and per bracket whether it held a root: the nodes of the
// derivative (degree D - 1, each coefficient the previous one's times its exponent) cut the real line into D brackets
// on each of which c is monotonic; a bracket (lo, hi] with a sign change gets kEssBisections bisection steps in s --
// no root bound is needed, and the steps resolve a root of any magnitude to a relative 2^-47 -- and kEssNewton Newton
// steps in z kept only inside what the bisection left; a bracket without one hands its lower end on as a node.
template <int D>
struct EssChain {
    static __device__ __forceinline__ void run(const double (&c)[D + 1], double (&out_s)[D + 2], double (&out_z)[D + 2],
                                               bool (&has)[D]) {
#pragma clang fp contract(off)
        double dc[D];
#pragma unroll
        for (int k = 0; k < D; k++) dc[k] = c[k + 1] * (double)(k + 1);
        double ns[D + 1], nz[D + 1];
        if constexpr (D == 1) {
            ns[0] = -1.0, ns[1] = 1.0;
            nz[0] = -(double)INFINITY, nz[1] = (double)INFINITY;
        } else {
            bool below[D - 1];
            EssChain<D - 1>::run(dc, ns, nz, below);
        }
        double f[D + 1];
#pragma unroll
        for (int i = 0; i <= D; i++) f[i] = ess_value<D>(c, nz[i]);
        out_s[0] = ns[0], out_z[0] = nz[0];
#pragma unroll
        for (int i = 0; i < D; i++) {
            const double flo = f[i], fhi = f[i + 1];
            const bool h = (flo < 0.0 && fhi >= 0.0) || (flo > 0.0 && fhi <= 0.0);
            double s = ns[i], z = nz[i];
            if (h) {
                double a = ns[i], b = ns[i + 1];
#pragma unroll 1
                for (int t = 0; t < kEssBisections; t++) {
                    const double mid = 0.5 * (a + b);
                    const double fm = ess_value<D>(c, ess_z(mid));
                    const bool same = flo < 0.0 ? fm < 0.0 : fm > 0.0;
                    a = same ? mid : a;
                    b = same ? b : mid;
                }
                z = ess_z(0.5 * (a + b));
                const double za = ess_z(a), zb = ess_z(b);
#pragma unroll 1
                for (int t = 0; t < kEssNewton; t++) {
                    const double zn = z - ess_horner<D>(c, z) / ess_horner<D - 1>(dc, z);
                    z = (zn >= za && zn <= zb) ? zn : z;
                }
                s = z / (1.0 + __builtin_fabs(z));
                s = s < a ? a : s;
                s = s > b ? b : s;
            }
            out_s[i + 1] = s, out_z[i + 1] = z;
            has[i] = h;
        }
        out_s[D + 1] = ns[D], out_z[D + 1] = nz[D];
    }
};

// The LDS of a workgroup, declared in a plain function as verify.hip's is.
struct EssLds {
    double* m;  // 200 entries per lane
    int* perm;  // 9 entries per lane
};
__device__ __forceinline__ EssLds ess_lds() {
    __shared__ double s_m[200 * kEssThreads];
    __shared__ int s_perm[9 * kEssThreads];
    return EssLds{s_m, s_perm};
}

// The cameras as the kernel takes them.  A single call's two travel by value; a batch's table and the cameras of 64
// pairs together would not fit the 4 KiB of kernel arguments, so k_essential_cameras writes them to the verifier's
// scratch first (query cameras at [0, kVerifyMaxPairs), train cameras behind them) and the kernel reads its pair's.
struct EssCameraPair {
    PoseCamera q, t;
};
struct EssCameraTable {
    const PoseCamera* cams;
};
__device__ __forceinline__ EssCameraPair cameras_of(const EssCameraPair& c) { return c; }
__device__ __forceinline__ EssCameraPair cameras_of(const EssCameraTable& c) {
    return EssCameraPair{c.cams[blockIdx.y], c.cams[kVerifyMaxPairs + blockIdx.y]};
}

}  // namespace

__global__ __launch_bounds__(kVerifyMaxPairs) void k_essential_cameras(PoseCameras cams, int P,
                                                                       PoseCamera* __restrict__ out) {
    const int p = threadIdx.x;
    if (p >= P) return;
    out[p] = cams.q[p];
    out[kVerifyMaxPairs + p] = cams.t[p];
}

template <class List, class Cams>
__global__ __launch_bounds__(kEssThreads) void k_verify_hypotheses_e(List list, const float4* __restrict__ pts, int K,
                                                                    unsigned seed, Cams cameras,
                                                                    int* __restrict__ samples, float* __restrict__ Fout,
                                                                    int* __restrict__ valid) {
#pragma clang fp contract(off)
    if constexpr (kBatched<List>) {
        const int pair = pair_of(list);
        const size_t k0 = (size_t)K * pair;
        pts += row0_of(list), seed += (unsigned)pair, samples += 5 * k0, Fout += 9 * kEssentialSlots * k0;
        valid += kEssentialSlots * k0;
    }
    const VerifyInput in = list_of(list);
    const EssLds lds = ess_lds();
    const int lane = threadIdx.x;
    const int k = blockIdx.x * kEssThreads + lane;
    if (k >= K) return;  // no barrier below: a lane works on its own LDS column
    const int n = verify_n(in.count, in.cap);
    double* const M = lds.m + lane;
    const EssCameraPair cams = cameras_of(cameras);
    const double fxq = cams.q.fx, fyq = cams.q.fy, cxq = cams.q.cx, cyq = cams.q.cy;
    const double fxt = cams.t.fx, fyt = cams.t.fy, cxt = cams.t.cx, cyt = cams.t.cy;

    bool ok = n >= 5;
    int pick[5];
#pragma unroll
    for (int j = 0; j < 5; j++) pick[j] = -1;
    if (ok) {
        draw<5>(seed, k, n, pick);
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const float4 p = pts[pick[r]];
            const double qx = ((double)p.x - cxq) / fxq, qy = ((double)p.y - cyq) / fyq;
            const double tx = ((double)p.z - cxt) / fxt, ty = ((double)p.w - cyt) / fyt;
            EA(r, 0) = tx * qx;
            EA(r, 1) = tx * qy;
            EA(r, 2) = tx;
            EA(r, 3) = ty * qx;
            EA(r, 4) = ty * qy;
            EA(r, 5) = ty;
            EA(r, 6) = qx;
            EA(r, 7) = qy;
            EA(r, 8) = 1.0;
        }
        ok = ess_null_space(M, lds.perm + lane);
    }
    double e[9][4];  // entry i of E as X[i] x + Y[i] y + Z[i] z + W[i]
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int f = 0; f < 4; f++) e[i][f] = ok ? EB(f, i) : 0.0;
    if (ok) {
        ess_constraints(M, e);
        ok = ess_reduce(M);
    }
    // The 3 x 3 matrix in z over (x, y, 1): row i is <row 4 + 2 i> - z <row 5 + 2 i> of the reduced system, each
    // divided by its pivot; the right-hand columns are x z^2, x z, x, y z^2, y z, y, z^3, z^2, z, 1.
    double bx[3][4], by[3][4], b1[3][5];
    double c[11];
#pragma unroll
    for (int i = 0; i < 11; i++) c[i] = 0.0;
    if (ok) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double u[10], v[10];
            const double pu = EM(4 + 2 * i, 4 + 2 * i), pv = EM(5 + 2 * i, 5 + 2 * i);
#pragma unroll
            for (int j = 0; j < 10; j++) u[j] = EM(4 + 2 * i, 10 + j) / pu, v[j] = EM(5 + 2 * i, 10 + j) / pv;
            bx[i][0] = u[2], bx[i][1] = u[1] - v[2], bx[i][2] = u[0] - v[1], bx[i][3] = -v[0];
            by[i][0] = u[5], by[i][1] = u[4] - v[5], by[i][2] = u[3] - v[4], by[i][3] = -v[3];
            b1[i][0] = u[9], b1[i][1] = u[8] - v[9], b1[i][2] = u[7] - v[8], b1[i][3] = u[6] - v[7], b1[i][4] = -v[6];
        }
        // det = (B00 (B11 B22 - B12 B21) - B01 (B10 B22 - B12 B20)) + B02 (B10 B21 - B11 B20).
        double t0[11], t1[11], t2[11];
        ess_minor_times(by[1], b1[2], b1[1], by[2], bx[0], t0);
        ess_minor_times(bx[1], b1[2], b1[1], bx[2], by[0], t1);
        ess_minor_times(bx[1], by[2], by[1], bx[2], b1[0], t2);
#pragma unroll
        for (int i = 0; i < 11; i++) c[i] = (t0[i] - t1[i]) + t2[i];
    }
    // A polynomial without its leading coefficient, or with a non-finite one: no model from this sample.
    if (ok) {
        ok = c[10] != 0.0;
#pragma unroll
        for (int i = 0; i < 11; i++) ok = ok && finite_d(c[i]);
    }
    double nodes_s[12], nodes[12];
    bool has[10];
#pragma unroll
    for (int i = 0; i < 10; i++) has[i] = false;
    if (ok) EssChain<10>::run(c, nodes_s, nodes, has);

    int slot = 0;
    float* const Fk = Fout + 9 * kEssentialSlots * (size_t)k;
    int* const vk = valid + kEssentialSlots * (size_t)k;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        if (!(ok && has[i])) continue;
        const double z = nodes[i + 1];
        // Cramer's rule on the row pair (0, 1), (0, 2) or (1, 2) of B(z) with the largest |d|, the first on a tie.
        double bz[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
            bz[r][0] = ess_horner<3>(bx[r], z), bz[r][1] = ess_horner<3>(by[r], z), bz[r][2] = ess_horner<4>(b1[r], z);
        double d = 0.0, x = 0.0, y = 0.0;
#pragma unroll
        for (int pr = 0; pr < 3; pr++) {
            const int u = pr < 2 ? 0 : 1, v = pr == 0 ? 1 : 2;
            const double du = bz[u][0] * bz[v][1] - bz[u][1] * bz[v][0];
            const double xu = bz[u][1] * bz[v][2] - bz[u][2] * bz[v][1];
            const double yu = bz[u][2] * bz[v][0] - bz[u][0] * bz[v][2];
            const bool better = pr == 0 || __builtin_fabs(du) > __builtin_fabs(d);
            d = better ? du : d, x = better ? xu : x, y = better ? yu : y;
        }
        x = x / d, y = y / d;
        double E[9], G[9];
#pragma unroll
        for (int j = 0; j < 9; j++) E[j] = ((x * e[j][0] + y * e[j][1]) + z * e[j][2]) + e[j][3];
        // F = Kt^-T E Kq^-1: E Kq^-1 column by column, then Kt^-T on the rows.
#pragma unroll
        for (int r = 0; r < 3; r++) {
            E[3 * r] = E[3 * r] / fxq;
            E[3 * r + 1] = E[3 * r + 1] / fyq;
            E[3 * r + 2] = E[3 * r + 2] - (E[3 * r] * cxq + E[3 * r + 1] * cyq);
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            G[j] = E[j] / fxt;
            G[3 + j] = E[3 + j] / fyt;
            G[6 + j] = E[6 + j] - (G[j] * cxt + G[3 + j] * cyt);
        }
        double ss = G[0] * G[0];
#pragma unroll
        for (int j = 1; j < 9; j++) ss = ss + G[j] * G[j];
        const double nrm = __builtin_sqrt(ss);
        float g[9];
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            g[j] = (float)(G[j] / nrm);
            fin = fin && finite_f(g[j]);
        }
#pragma unroll
        for (int j = 0; j < 9; j++) Fk[9 * slot + j] = fin ? g[j] : 0.f;
        vk[slot] = fin ? 1 : 0;
        slot++;
    }
    for (; slot < kEssentialSlots; slot++) {
        for (int j = 0; j < 9; j++) Fk[9 * slot + j] = 0.f;
        vk[slot] = 0;
    }
#pragma unroll
    for (int j = 0; j < 5; j++) samples[5 * (size_t)k + j] = pick[j];
}
#undef EA
#undef EB
#undef EM

template <class List>
void launch_verify_hypotheses_e(const List& list, const float4* pts, int K, unsigned seed, const PoseCameras& cams,
                                PoseCamera* cam_scratch, int* samples, float* F, int* valid, hipStream_t s) {
    const dim3 grid((K + kEssThreads - 1) / kEssThreads, list_pairs(list)), block(kEssThreads);
    if constexpr (std::is_same_v<List, VerifyBatch>) {
        hipLaunchKernelGGL(k_essential_cameras, dim3(1), dim3(kVerifyMaxPairs), 0, s, cams, list.P, cam_scratch);
        hipLaunchKernelGGL((k_verify_hypotheses_e<List, EssCameraTable>), grid, block, 0, s, list, pts, K, seed,
                           EssCameraTable{cam_scratch}, samples, F, valid);
    } else {
        hipLaunchKernelGGL((k_verify_hypotheses_e<List, EssCameraPair>), grid, block, 0, s, list, pts, K, seed,
                           EssCameraPair{cams.q[0], cams.t[0]}, samples, F, valid);
    }
}

template void launch_verify_hypotheses_e<VerifyInput>(const VerifyInput&, const float4*, int, unsigned, const PoseCameras&,
                                                      PoseCamera*, int*, float*, int*, hipStream_t);
template void launch_verify_hypotheses_e<VerifyBatch>(const VerifyBatch&, const float4*, int, unsigned, const PoseCameras&,
                                                      PoseCamera*, int*, float*, int*, hipStream_t);

}  // namespace sift_amd
