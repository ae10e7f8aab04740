// Rows of the descriptor window: which samples j of row i pass the oracle's
// bin test (calcSIFTDescriptor: -1 < rbin < d and -1 < cbin < d), as one exact
// interval per row.  Plain C++ (the CPU test tests/cpp/test_desc_rows.cpp
// includes it), __host__ __device__ under hipcc: k_descriptor and
// k_descriptor_exact (descriptor.hip) enumerate exactly these samples.
//
// For a fixed row i, rbin(j) = ((fl(j*sin) + i*cos) + 2) - 0.5 and cbin(j) =
// ((fl(j*cos) - i*sin) + 2) - 0.5 are compositions of monotone float
// operations in j (a rounded product with a constant, rounded additions of
// constants), so each of the four compares holds on an interval of j and the
// set of passing samples is one interval.  desc_row_interval starts from a
// conservative superset (desc_clip_interval: the real-number bounds widened
// by a margin) and moves each end inward while desc_bins_inside -- the
// per-sample test, float operation for float operation -- fails.
//
// Every translation unit that uses this header is compiled with
// -ffp-contract=off: the products and sums below must round separately, as
// they do in the sample loops.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SIFT_ROWS_FN __host__ __device__ __forceinline__
#else
#define SIFT_ROWS_FN inline
#endif
// The trim loops run a few steps: kept as plain loops (vectorised and unrolled
// they cost the kernels code size and registers for nothing).
#if defined(__clang__)
#define SIFT_ROWS_SHORT_LOOP _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")
#else
#define SIFT_ROWS_SHORT_LOOP
#endif

namespace sift_amd {

constexpr int kDescD = 4;  // d: the descriptor is d x d cells

// The bin test of window sample (i, j).  nis = -(i * sin) and ic = i * cos are
// the row's terms (rounded products); per sample: j*cos, j*sin, + (nis, ic),
// + d/2, - 0.5, then the four compares -- desc_sample's operations
// (a - b and a + (-b) are the same IEEE operation).
SIFT_ROWS_FN bool desc_bins_inside(float cos_t, float sin_t, float nis, float ic, int j) {
    const float fj = (float)j;
    const float c_rot = fj * cos_t + nis;
    const float r_rot = fj * sin_t + ic;
    const float rbin = r_rot + (float)(kDescD / 2) - 0.5f;
    const float cbin = c_rot + (float)(kDescD / 2) - 0.5f;
    return rbin > -1 && rbin < kDescD && cbin > -1 && cbin < kDescD;
}

// Shrink [lo, hi] to a superset of the integers j with -1 < j*s + b < d
// (margin 1e-4 in bin units and one sample each side, so float rounding of the
// exact per-sample test can never fall outside the enumerated range).
// inv_s = 1 / s (computed once per keypoint; an approximate reciprocal will
// do).  Float: the bounds before clamping to +-(R+2) carry a relative error of
// a few 1e-7, i.e. < 1e-4 samples for R <= 63, far inside the one-sample
// margin each side.
SIFT_ROWS_FN void desc_clip_interval(int& lo, int& hi, float s, float inv_s, float b, int R) {
    constexpr float lb = -1.f - 1e-4f, ub = kDescD + 1e-4f;
    if (fabsf(s) < 1e-12f) {
        if (b <= lb || b >= ub) hi = lo - 1;
        return;
    }
    float x1 = (lb - b) * inv_s, x2 = (ub - b) * inv_s;
    if (x1 > x2) {
        const float t = x1;
        x1 = x2;
        x2 = t;
    }
    x1 = fmaxf(x1, (float)(-R - 2));
    x2 = fminf(x2, (float)(R + 2));
    const int l = (int)floorf(x1) - 1, h = (int)ceilf(x2) + 1;
    lo = lo > l ? lo : l;
    hi = hi < h ? hi : h;
}

// The conservative interval of row i inside [lo, hi] (the caller's image
// clipping; hi < lo: empty).
SIFT_ROWS_FN void desc_row_conservative(int& lo, int& hi, int i, float cos_t, float sin_t, float inv_cos, float inv_sin,
                                        int R) {
    desc_clip_interval(lo, hi, sin_t, inv_sin, (float)i * cos_t + (kDescD / 2 - 0.5f), R);
    desc_clip_interval(lo, hi, cos_t, inv_cos, -(float)i * sin_t + (kDescD / 2 - 0.5f), R);
}

// The exact interval of row i inside [lo, hi]: on return every j in [lo, hi]
// passes desc_bins_inside and no other j of the caller's interval does; an
// empty row returns hi < lo.  The trims take at most hi - lo + 1 steps in all
// (a handful in practice: the conservative ends are 1-3 samples out).
SIFT_ROWS_FN void desc_row_interval(int& lo, int& hi, int i, float cos_t, float sin_t, float inv_cos, float inv_sin,
                                    int R) {
    desc_row_conservative(lo, hi, i, cos_t, sin_t, inv_cos, inv_sin, R);
    const float fi = (float)i, nis = -(fi * sin_t), ic = fi * cos_t;
    SIFT_ROWS_SHORT_LOOP
    while (lo <= hi && !desc_bins_inside(cos_t, sin_t, nis, ic, lo)) lo++;
    SIFT_ROWS_SHORT_LOOP
    while (hi >= lo && !desc_bins_inside(cos_t, sin_t, nis, ic, hi)) hi--;
}

}  // namespace sift_amd
