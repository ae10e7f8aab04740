// Match lists for gfx950: the filtered, compacted cv::DMatch records of the
// matcher's top-2 arrays (k_match_select) and the capped radius list of its
// k-NN table (k_knn_select).  The kernels that fill those arrays are match.hip
// and match_knn.hip.
#include "sift_kernels.h"
#include "sift_match.h"

namespace sift_amd {

// ---------------------------------------------------------------------------
// k_match_select: match lists (sift_hip_match_list_*).  The match kernels above
// have written the forward top-2 of every query of every pair, and -- when the
// filter needs it -- the reverse top-2 of every train row (the same kernels
// with the roles swapped), into the matcher's select scratch.  One workgroup
// per pair (1024 threads, 16 waves) walks the pair's queries in chunks of 1024:
// a lane evaluates the keep rule of its query (include/sift_hip.h) -- the
// ratio test of write_match on the forward pair, the distance cap, and for the
// cross check / two-way ratio test a gather of row i1 of the reverse arrays --
// and the kept queries take consecutive slots in query order: a 64-bit ballot
// and popcount inside the wave, the wave totals through LDS, a running base
// across chunks.  No atomics: the slot of a query depends on the keep bits of
// the queries before it only, so the output bytes are the same in every run.
// ---------------------------------------------------------------------------
constexpr int kSelectThreads = 1024, kSelectWaves = kSelectThreads / 64;

__device__ __forceinline__ bool ratio_pass(int a1, float d1, int a2, float d2, float ratio, int ratio_on_squared) {
    if (a1 < 0) return false;
    if (a2 < 0 || !(ratio > 0.f)) return true;
    if (ratio_on_squared) return d1 < ratio * d2;
    return __builtin_sqrtf(d1) < ratio * __builtin_sqrtf(d2);
}

__global__ __launch_bounds__(kSelectThreads) void k_match_select(SelectBatch batch, const int* __restrict__ idx2,
                                                                 const float* __restrict__ d2, MatchFilter f,
                                                                 MatchRecord* __restrict__ out,
                                                                 int* __restrict__ counts) {
    __shared__ int s_wave[kSelectWaves];
    const int p = blockIdx.x;
    const SelectPair pr = batch.pair[p];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const bool reverse = f.cross_check || f.ratio_both_ways;
    const int2* const fi = reinterpret_cast<const int2*>(idx2) + pr.fwd;
    const float2* const fd = reinterpret_cast<const float2*>(d2) + pr.fwd;
    const int2* const ri = reinterpret_cast<const int2*>(idx2) + pr.rev;
    const float2* const rd = reinterpret_cast<const float2*>(d2) + pr.rev;
    MatchRecord* const o = out + pr.out_off;
    int base = 0;
    for (int c0 = 0; c0 < pr.nq; c0 += kSelectThreads) {  // workgroup-uniform
        const int i = c0 + tid;
        bool keep = false;
        MatchRecord rec{i, -1, p, 0.f};
        if (i < pr.nq) {
            const int2 a = fi[i];
            const float2 e = fd[i];
            rec.trainIdx = a.x;
            rec.distance = __builtin_sqrtf(e.x);
            keep = a.x >= 0 && a.x < pr.nt && ratio_pass(a.x, e.x, a.y, e.y, f.ratio, f.ratio_on_squared) &&
                   (!(f.max_distance > 0.f) || rec.distance <= f.max_distance);
            if (keep && reverse) {
                const int2 b = ri[a.x];
                const float2 g = rd[a.x];
                if (f.cross_check) keep = b.x == i;
                if (keep && f.ratio_both_ways) keep = ratio_pass(b.x, g.x, b.y, g.y, f.ratio, f.ratio_on_squared);
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kSelectWaves; k++) {
            const int c = s_wave[k];
            before += k < w ? c : 0;
            total += c;
        }
        if (keep) o[base + before + __popcll(mask & lt_mask)] = rec;
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0) counts[p] = base;
}

void launch_match_select(const SelectBatch& batch, int P, const int* idx2, const float* d2, const MatchFilter& filter,
                         MatchRecord* out, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(k_match_select, dim3(P), dim3(kSelectThreads), 0, s, batch, idx2, d2, filter, out, counts);
}

// k_knn_select: the capped radius list.  One workgroup per pair walks the
// pair's nq k table entries in (query, rank) order, 1024 at a time; an entry is
// kept when it holds a neighbour within max_distance, and the kept entries take
// consecutive slots by the ballot / popcount / LDS prefix of k_match_select.
__global__ __launch_bounds__(kSelectThreads) void k_knn_select(SelectBatch batch, int k, const int* __restrict__ idx,
                                                               const float* __restrict__ d2, float max_distance,
                                                               MatchRecord* __restrict__ out,
                                                               int* __restrict__ counts) {
    __shared__ int s_wave[kSelectWaves];
    const int p = blockIdx.x;
    const SelectPair pr = batch.pair[p];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int* const ti = idx + (size_t)pr.fwd * k;
    const float* const td = d2 + (size_t)pr.fwd * k;
    MatchRecord* const o = out + pr.out_off;
    const int n = pr.nq * k;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += kSelectThreads) {  // workgroup-uniform
        const int e = c0 + tid;
        bool keep = false;
        MatchRecord rec{0, -1, p, 0.f};
        if (e < n) {
            rec.queryIdx = e / k;
            rec.trainIdx = ti[e];
            rec.distance = __builtin_sqrtf(td[e]);
            keep = rec.trainIdx >= 0 && (!(max_distance > 0.f) || rec.distance <= max_distance);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < kSelectWaves; j++) {
            const int c = s_wave[j];
            before += j < w ? c : 0;
            total += c;
        }
        if (keep) o[base + before + __popcll(mask & lt_mask)] = rec;
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0) counts[p] = base;
}

void launch_knn_select(const SelectBatch& batch, int P, int k, const int* idx, const float* d2, float max_distance,
                       MatchRecord* out, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(k_knn_select, dim3(P), dim3(kSelectThreads), 0, s, batch, k, idx, d2, max_distance, out, counts);
}

}  // namespace sift_amd
