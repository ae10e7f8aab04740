// Two-view verification: a fixed-budget RANSAC for the fundamental matrix over
// a match list, on the device (sift_hip_verify_*; the rule -- sampler, solver,
// score, selection -- is written out in include/sift_hip.h and mirrored in
// numpy by sift_amd.cv.ransac_fundamental).
//
//  k_verify_gather      record j -> (qx, qy, tx, ty) in scratch, NaN for a
//                       record whose index lies outside its position array:
//                       the only kernel that reads positions through a record.
//  k_verify_hypotheses  one thread per hypothesis: the counter-based draw of 8
//                       distinct matches and the normalised 8-point solve.
//                       Full pivoting indexes the 8 x 9 system by run-time
//                       row and column, so it lives in LDS laid out
//                       [entry][lane] (a lane's entries are 64 floats apart:
//                       every access of a wave is one conflict-free row).
//  k_verify_score       the hot path, K x n predicate evaluations: one wave
//                       per hypothesis, the workgroup's waves share an
//                       LDS-staged tile of the gathered matches, lanes stride
//                       over it, ballot + popcount count, one store per
//                       hypothesis.  The predicate is sift_epipolar.h's, the
//                       matcher's own.
//  k_verify_select      one 1024-thread workgroup: argmax with the tie rule,
//                       the winner rescored into the mask, and the ordered
//                       compaction of k_match_select (prefix sums, no atomics:
//                       the same bytes in every run).
// Everything is float32 with -ffp-contract=off and correctly rounded division
// and square root: the operation order written here is the one executed.
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

// lowbias32 (the header writes it out).
__device__ __forceinline__ unsigned mix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) < INFINITY; }

// Hartley normalisation of one side of a sample: x, y become the normalised
// coordinates, (s, ox, oy) the similarity x' = s x + ox.
__device__ __forceinline__ void normalise8(float (&x)[8], float (&y)[8], float& s, float& ox, float& oy) {
#pragma clang fp contract(off)
    float sx = x[0], sy = y[0];
#pragma unroll
    for (int i = 1; i < 8; i++) {
        sx = sx + x[i];
        sy = sy + y[i];
    }
    const float mx = sx / 8.0f, my = sy / 8.0f;
    float sd = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        x[i] = x[i] - mx;
        y[i] = y[i] - my;
        const float d = __builtin_sqrtf(x[i] * x[i] + y[i] * y[i]);
        sd = i == 0 ? d : sd + d;
    }
    const float md = sd / 8.0f;
    s = 1.41421354f / md;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        x[i] = x[i] * s;
        y[i] = y[i] * s;
    }
    ox = -(s * mx);
    oy = -(s * my);
}

constexpr int kHypThreads = 64;

}  // namespace

__global__ __launch_bounds__(256) void k_verify_gather(VerifyInput in, float4* __restrict__ pts) {
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

__global__ __launch_bounds__(kHypThreads) void k_verify_hypotheses(VerifyInput in, const float4* __restrict__ pts, int K,
                                                                  unsigned seed, int* __restrict__ samples,
                                                                  float* __restrict__ Fout, int* __restrict__ valid) {
#pragma clang fp contract(off)
    __shared__ float s_a[72 * kHypThreads];  // the 8 x 9 system, entry e = 9 row + col of lane l at [e][l]
    __shared__ float s_y[9 * kHypThreads];   // the solution in pivot order, then in column order
    __shared__ int s_perm[9 * kHypThreads];  // the original column at each position
    const int lane = threadIdx.x;
    const int k = blockIdx.x * kHypThreads + lane;
    if (k >= K) return;  // no barrier below: a lane works on its own LDS column
    const int n = verify_n(in.count, in.cap);
    float* const A = s_a + lane;
    float* const Y = s_y + lane;
    int* const P = s_perm + lane;
#define VA(r, c) A[((r) * 9 + (c)) * kHypThreads]

    bool ok = n >= 8;
    int pick[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pick[j] = -1;
    float g[9];
#pragma unroll
    for (int i = 0; i < 9; i++) g[i] = 0.f;
    float sq = 0.f, oqx = 0.f, oqy = 0.f, st = 0.f, otx = 0.f, oty = 0.f;
    if (ok) {
        // The draw: 8 distinct indices of [0, n), a function of (seed, k, n).
        const unsigned base = mix32(seed ^ mix32((unsigned)k));
        int sorted[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
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
        float qx[8], qy[8], tx[8], ty[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 p = pts[pick[j]];
            qx[j] = p.x, qy[j] = p.y, tx[j] = p.z, ty[j] = p.w;
        }
        normalise8(qx, qy, sq, oqx, oqy);
        normalise8(tx, ty, st, otx, oty);
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
        for (int c = 0; c < 9; c++) P[c * kHypThreads] = c;
        // Gaussian elimination with full pivoting: the largest |entry| of rows and columns >= c, the scan starting at
        // (c, c) in row-major order and moving on a strictly larger value only.
        for (int c = 0; c < 8 && ok; c++) {
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
            ok = p != 0.f && finite_f(p);
            if (!ok) break;
            for (int r = c + 1; r < 8; r++) {
                const float m = VA(r, c) / p;
                for (int j = c + 1; j < 9; j++) VA(r, j) = VA(r, j) - m * VA(c, j);
            }
        }
    }
    if (ok) {
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
        float ss = F[0] * F[0];
#pragma unroll
        for (int i = 1; i < 9; i++) ss = ss + F[i] * F[i];
        const float nrm = __builtin_sqrtf(ss);
#pragma unroll
        for (int i = 0; i < 9; i++) {
            g[i] = F[i] / nrm;
            ok = ok && finite_f(g[i]);
        }
    }
#undef VA
#pragma unroll
    for (int j = 0; j < 8; j++) samples[8 * (size_t)k + j] = pick[j];
#pragma unroll
    for (int i = 0; i < 9; i++) Fout[9 * (size_t)k + i] = ok ? g[i] : 0.f;
    valid[k] = ok ? 1 : 0;
}

// The predicate of match p under a hypothesis: the matcher's epipolar gate for
// the match's own pair, no window (radius = +inf).
__device__ __forceinline__ bool verify_pass(const float (&f)[9], const float4 p, float e2) {
    const EpiQuery q = epi_query(f, p.x, p.y);
    return epi_pass(q, p.z, p.w, epi_row(f, p.z, p.w), e2, INFINITY);
}

constexpr int kScoreWaves = 4;     // hypotheses per workgroup
constexpr int kScoreUnroll = 4;    // matches per lane and loop iteration
constexpr int kScoreTile = 2048;   // matches per LDS tile (32 KiB): 2000 matches are one tile

__global__ __launch_bounds__(64 * kScoreWaves) void k_verify_score(VerifyInput in, const float4* __restrict__ pts,
                                                                   const float* __restrict__ F,
                                                                   const int* __restrict__ valid, int K, float e2,
                                                                   int* __restrict__ counts) {
    __shared__ float4 s_pts[kScoreTile];
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = blockIdx.x * kScoreWaves + __builtin_amdgcn_readfirstlane(tid >> 6);
    // F and the flag are loaded side by side (an invalid hypothesis' row is zero, not garbage).
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
                    pass[u] = (i < m) & verify_pass(f, s_pts[i < m ? i : 0], e2);  // no branch: m >= 1 here
                }
#pragma unroll
                for (int u = 0; u < kScoreUnroll; u++) cnt += __popcll(__ballot(pass[u]));
            }
    }
    if (lane == 0 && k < K) counts[k] = cnt;
}

constexpr int kVSelThreads = 1024, kVSelWaves = kVSelThreads / 64;

__global__ __launch_bounds__(kVSelThreads) void k_verify_select(VerifyInput in, const float4* __restrict__ pts,
                                                                const float* __restrict__ F,
                                                                const int* __restrict__ valid,
                                                                const int* __restrict__ counts, int K, float e2,
                                                                VerifyResult* __restrict__ result,
                                                                MatchRecord* __restrict__ out, int* __restrict__ out_count,
                                                                uint8_t* __restrict__ mask) {
    __shared__ int s_key[kVSelWaves], s_nv[kVSelWaves], s_wave[kVSelWaves];
    const int n = verify_n(in.count, in.cap);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // The winner: most inliers among the valid hypotheses, ties to the lowest k, as the largest key
    // count * 4096 + (4095 - k) (count <= 65536, k < 4096); -1: none.
    int key = -1, nv = 0;
    for (int k = tid; k < K; k += kVSelThreads)
        if (valid[k]) {
            nv++;
            key = max(key, counts[k] * 4096 + (4095 - k));
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
    const int hyp = key < 0 ? -1 : 4095 - (key & 4095);
    float f[9];
#pragma unroll
    for (int i = 0; i < 9; i++) f[i] = hyp < 0 ? 0.f : F[9 * (size_t)hyp + i];
    if (tid == 0) {
        VerifyResult r;
#pragma unroll
        for (int i = 0; i < 9; i++) r.F[i] = f[i];
        r.inliers = key < 0 ? 0 : key >> 12;
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
        const bool keep = hyp >= 0 && j < n && verify_pass(f, pts[j < n ? j : 0], e2);
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

void launch_verify_gather(const VerifyInput& in, float4* pts, hipStream_t s) {
    if (in.cap > 0) hipLaunchKernelGGL(k_verify_gather, dim3((in.cap + 255) / 256), dim3(256), 0, s, in, pts);
}

void launch_verify_hypotheses(const VerifyInput& in, const float4* pts, int K, unsigned seed, int* samples, float* F,
                              int* valid, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_hypotheses, dim3((K + kHypThreads - 1) / kHypThreads), dim3(kHypThreads), 0, s, in, pts, K,
                       seed, samples, F, valid);
}

void launch_verify_score(const VerifyInput& in, const float4* pts, const float* F, const int* valid, int K, float e2,
                         int* counts, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_score, dim3((K + kScoreWaves - 1) / kScoreWaves), dim3(64 * kScoreWaves), 0, s, in, pts, F,
                       valid, K, e2, counts);
}

void launch_verify_select(const VerifyInput& in, const float4* pts, const float* F, const int* valid, const int* counts,
                          int K, float e2, VerifyResult* result, MatchRecord* out, int* out_count, uint8_t* mask,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_verify_select, dim3(1), dim3(kVSelThreads), 0, s, in, pts, F, valid, counts, K, e2, result, out,
                       out_count, mask);
}

}  // namespace sift_amd
