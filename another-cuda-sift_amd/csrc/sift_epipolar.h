// The epipolar predicate (the rule is in include/sift_hip.h), shared by the
// matcher's epipolar gate (sift_match_dev.h; match.hip's k_match_epipolar, match_knn.hip) and the two-view
// verifier's score (verify.hip): one statement of the float32 operation order.
#pragma once
#include <hip/hip_runtime.h>

namespace sift_amd {

// Train row t is a candidate of query i when its Sampson distance to the pair's
// fundamental matrix is at most max_error and it lies in the query's window.
// float32, round to nearest, the operations in the order written and never
// fused: a query's side is its line (a, b, c) = F x_q and nq = a^2 + b^2, a
// row's side nr = u^2 + v^2 of (u, v, .) = F^T x_t, and a pair costs
// r = (a tx + b ty) + c, r r <= e2 (nq + nr).  Any NaN fails the compare.
struct EpiQuery {
    float a, b, c, nq, qx, qy;
};
__device__ __forceinline__ EpiQuery epi_query(const float (&F)[9], float qx, float qy) {
#pragma clang fp contract(off)
    EpiQuery e;
    e.a = (F[0] * qx + F[1] * qy) + F[2];
    e.b = (F[3] * qx + F[4] * qy) + F[5];
    e.c = (F[6] * qx + F[7] * qy) + F[8];
    e.nq = e.a * e.a + e.b * e.b;
    e.qx = qx;
    e.qy = qy;
    return e;
}
__device__ __forceinline__ float epi_row(const float (&F)[9], float tx, float ty) {
#pragma clang fp contract(off)
    const float u = (F[0] * tx + F[3] * ty) + F[6];
    const float v = (F[1] * tx + F[4] * ty) + F[7];
    return u * u + v * v;
}
// The pair's side for V = float or two rows at once, V = f32x2 (the same
// operations per component): r r and e2 (nq + nr) to compare, and the window's
// two differences.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <class V>
__device__ __forceinline__ void epi_terms(const EpiQuery& q, V tx, V ty, V nr, float e2, V& lhs, V& rhs, V& dx, V& dy) {
#pragma clang fp contract(off)
    const V r = (q.a * tx + q.b * ty) + q.c;
    lhs = r * r;
    rhs = e2 * (q.nq + nr);
    dx = tx - q.qx;
    dy = ty - q.qy;
}
__device__ __forceinline__ bool epi_in(float lhs, float rhs, float dx, float dy, float radius) {
    return (lhs <= rhs) & (__builtin_fabsf(dx) <= radius) & (__builtin_fabsf(dy) <= radius);
}
__device__ __forceinline__ bool epi_pass(const EpiQuery& q, float tx, float ty, float nr, float e2, float radius) {
    float lhs, rhs, dx, dy;
    epi_terms(q, tx, ty, nr, e2, lhs, rhs, dx, dy);
    return epi_in(lhs, rhs, dx, dy, radius);
}
// Two train rows at once: the integer fold takes keys in pairs of adjacent rows,
// whose staged values sit in adjacent registers, so the packed fp32
// instructions apply and a pair of keys costs what one did.
__device__ __forceinline__ void epi_pass2(const EpiQuery& q, f32x2 tx, f32x2 ty, f32x2 nr, float e2, float radius,
                                          bool& p0, bool& p1) {
    f32x2 lhs, rhs, dx, dy;
    epi_terms(q, tx, ty, nr, e2, lhs, rhs, dx, dy);
    p0 = epi_in(lhs[0], rhs[0], dx[0], dy[0], radius);
    p1 = epi_in(lhs[1], rhs[1], dx[1], dy[1], radius);
}

}  // namespace sift_amd
