// Device-side pieces the verifier's kernels share (verify.hip, essential.hip, refit.hip): how a kernel finds its list
// -- the call's own, or pair blockIdx.y's of a batch --, the counter-based sampler and the models' predicates.  Included
// by .hip files only.
#pragma once
#include <float.h>
#include <math.h>

#include "sift_epipolar.h"
#include "sift_verify.h"

namespace sift_amd {

namespace {

__device__ __forceinline__ int verify_n(const int* count, int cap) {
    if (!count) return cap;
    const int c = *count;
    return c < 0 ? 0 : (c < cap ? c : cap);
}

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) < INFINITY; }

// lowbias32 (the header writes it out).
__device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// The draw of hypothesis k: M distinct indices of [0, n), n >= M, a function of (seed, k, n).
template <int M>
__device__ __forceinline__ void draw(unsigned seed, int k, int n, int (&pick)[M]) {
    const unsigned base = mix32(seed ^ mix32((unsigned)k));
    int sorted[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        const unsigned h = mix32(base + 0x9e3779b9u * (unsigned)(j + 1));
        int r = (int)(((unsigned long long)h * (unsigned long long)(unsigned)(n - j)) >> 32);
#pragma unroll
        for (int i = 0; i < j; i++)
            if (r >= sorted[i]) r++;
        pick[j] = r;
        int v = r;
#pragma unroll
        for (int i = 0; i < j; i++)
            if (sorted[i] > v) {
                const int t = sorted[i];
                sorted[i] = v;
                v = t;
            }
        sorted[j] = v;
    }
}

// The list a workgroup works on: the call's own, or pair blockIdx.y's rows of the batch's match buffer, its counter
// and its positions.
__device__ __forceinline__ const VerifyInput& list_of(const VerifyInput& in) { return in; }
__device__ __forceinline__ VerifyInput list_of(const VerifyBatch& b) {
    const int p = blockIdx.y;
    const VerifyBatchPair& e = b.pair[p];
    return VerifyInput{b.matches + e.row0, b.counts ? b.counts + p : nullptr, e.cap, e.qxy, e.txy, b.qstride, b.tstride,
                       e.nq, e.nt};
}
// A batch's workgroup: its pair, and the pair's first row of the per-match arrays.
__device__ __forceinline__ int pair_of(const VerifyBatch&) { return blockIdx.y; }
__device__ __forceinline__ int row0_of(const VerifyBatch& b) { return b.pair[blockIdx.y].row0; }
template <class List>
constexpr bool kBatched = false;
template <>
constexpr bool kBatched<VerifyBatch> = true;

}  // namespace

// The predicates of match p = (qx, qy, tx, ty) under a hypothesis, e2 = max_error^2.
// Fundamental: the matcher's epipolar gate for the match's own pair, no window (radius = +inf).
struct SampsonPass {
    static __device__ __forceinline__ bool pass(const float (&f)[9], const float4 p, float e2) {
        const EpiQuery q = epi_query(f, p.x, p.y);
        return epi_pass(q, p.z, p.w, epi_row(f, p.z, p.w), e2, INFINITY);
    }
};
// Homography: the forward transfer error, division-free, in front of the camera only.
struct TransferPass {
    static __device__ __forceinline__ bool pass(const float (&h)[9], const float4 p, float e2) {
#pragma clang fp contract(off)
        const float px = (h[0] * p.x + h[1] * p.y) + h[2];
        const float py = (h[3] * p.x + h[4] * p.y) + h[5];
        const float w = (h[6] * p.x + h[7] * p.y) + h[8];
        const float dx = px - p.z * w, dy = py - p.w * w;
        return (w > 0.f) & (dx * dx + dy * dy <= e2 * (w * w));
    }
};
// Affine map and similarity: the transfer error of {m0 .. m5, 0, 0, 1}.  TransferPass on the same nine floats gives
// the same answer (its w is exactly 1); this one does not form w.
struct AffinePass {
    static __device__ __forceinline__ bool pass(const float (&m)[9], const float4 p, float e2) {
#pragma clang fp contract(off)
        const float px = (m[0] * p.x + m[1] * p.y) + m[2];
        const float py = (m[3] * p.x + m[4] * p.y) + m[5];
        const float dx = px - p.z, dy = py - p.w;
        return dx * dx + dy * dy <= e2;
    }
};

}  // namespace sift_amd
