// The per-record steps the verifier's pose kernels share (pose.hip: the pose from a verified F; pose_homography.hip: from
// a verified H): the fit test, the normalised rays, the closed-form depths and the in-front test of the rule in
// include/sift_hip.h, step 6 of "Relative pose from a verified fundamental matrix".  Float64, nothing fused.  Included
// by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include "sift_verify_dev.h"

namespace sift_amd {

namespace {

__device__ __forceinline__ bool pose_finite(double v) { return __builtin_fabs(v) < (double)INFINITY; }

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// A record's normalised rays and the fit test (the refit rule's: marked, four finite coordinates).
struct PoseRays {
    double q0, q1, t0, t1;
};
__device__ __forceinline__ bool pose_fit(const float4 p, uint8_t m) {
    return m != 0 && finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w);
}
__device__ __forceinline__ PoseRays pose_rays(const float4 p, const double (&kq)[4], const double (&kt)[4]) {
#pragma clang fp contract(off)
    return PoseRays{((double)p.x - kq[2]) / kq[0], ((double)p.y - kq[3]) / kq[1], ((double)p.z - kt[2]) / kt[0],
                    ((double)p.w - kt[3]) / kt[1]};
}

// The depths (a, b) that minimise |a p + t - b x|^2, p = R xq, with det of the 2 x 2 normal equations and the cosine
// of the angle between the rays.
struct PoseDepths {
    double a, b, det, cosine;
};
__device__ __forceinline__ PoseDepths pose_depths(const double (&R)[9], const double (&t)[3], const PoseRays& x) {
#pragma clang fp contract(off)
    const double p0 = (R[0] * x.q0 + R[1] * x.q1) + R[2];
    const double p1 = (R[3] * x.q0 + R[4] * x.q1) + R[5];
    const double p2 = (R[6] * x.q0 + R[7] * x.q1) + R[8];
    const double pp = (p0 * p0 + p1 * p1) + p2 * p2;
    const double xx = (x.t0 * x.t0 + x.t1 * x.t1) + 1.0;
    const double px = (p0 * x.t0 + p1 * x.t1) + p2;
    const double pt = (p0 * t[0] + p1 * t[1]) + p2 * t[2];
    const double xt = (x.t0 * t[0] + x.t1 * t[1]) + t[2];
    const double det = pp * xx - px * px;
    return PoseDepths{(px * xt - pt * xx) / det, (pp * xt - px * pt) / det, det, px / __builtin_sqrt(pp * xx)};
}
// In front of both cameras, nearer than max_depth; a NaN fails every comparison.
__device__ __forceinline__ bool pose_front(double det, double a, double b, double max_depth) {
    return det > 0.0 && a > 0.0 && b > 0.0 && a < max_depth && b < max_depth;
}

}  // namespace

}  // namespace sift_amd
