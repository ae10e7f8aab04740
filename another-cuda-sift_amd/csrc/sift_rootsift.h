// RootSIFT (Arandjelovic & Zisserman 2012) on descriptor bytes: the one rule
// shared by k_descriptor, k_descriptor_exact (descriptor.hip) and k_rootsift
// (rootsift.hip); include/sift_hip.h states it for callers and
// sift_amd.cv.rootsift is its numpy mirror.
//
//   b[i]   = clamp(cvRound(v[i]), 0, 255), NaN -> 0   (identity on the detector's bytes)
//   s      = sum b[i]                                 (integer, <= 32,640: exact in any order)
//   out[i] = s == 0 ? 0 : min(255, cvRound(512 * sqrtf((float)b[i] / (float)s)))
//
// Division and square root are IEEE correctly rounded float32 operations (the
// build's -fhip-fp32-correctly-rounded-divide-sqrt on the device) and nothing
// is fused (-ffp-contract=off), 512 * r is exact, so the device, the host and
// numpy give the same byte.  sum r^2 = 1: the rows keep the scale of OpenCV's
// rows (norm ~512); the clamp at 255 acts only where one entry holds more than
// (254.5 / 512)^2 = 24.7 % of the row's L1 mass.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SIFT_ROOT_HD __host__ __device__ __forceinline__
#else
#define SIFT_ROOT_HD inline
#endif

namespace sift_amd {

// Step 1: a row entry of any float value to its byte (round half even).
SIFT_ROOT_HD int root_input_byte(float v) {
    const float r = __builtin_rintf(v);
    return r >= 255.f ? 255 : (r > 0.f ? (int)r : 0);  // NaN fails both tests: 0
}

// Steps 3-5: byte b of a row whose bytes sum to s.
SIFT_ROOT_HD int root_byte(int b, int s) {
    if (s == 0) return 0;
    const float r = __builtin_sqrtf((float)b / (float)s);
    const int o = (int)__builtin_rintf(512.f * r);
    return o > 255 ? 255 : o;
}

}  // namespace sift_amd
