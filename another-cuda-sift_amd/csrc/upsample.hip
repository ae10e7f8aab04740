// 2x bilinear upsample of the frame (firstOctave = -1) and the 8-bit frame
// conversion, for gfx950.
//
// Replaces the reference's sift_cuda/image_func/Resize.cu.  Semantics follow
// OpenCV 4.x; the float operation order is
// the oracle's (oracle/sift_oracle.cpp upsample2x), so planes are bit-exact.
#include <cstring>

#include "sift_kernels.h"
#include "sift_math.h"

namespace sift_amd {

// ---------------------------------------------------------------------------
// 2x bilinear upsample (OpenCV resize INTER_LINEAR on float; firstOctave = -1).
// Reference: Resize.cu:6-64 (half-pixel bilinear, target size ignored).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void up_coeff(int d, int slen, int& s, float& a0, float& a1) {
    // (d + 0.5) * 0.5 - 0.5 = d / 2 - 0.25: exact in float for every d < 2^22,
    // so this is the oracle's double expression to the bit.
    float f = (float)d * 0.5f - 0.25f;
    int si = (int)floorf(f);
    f -= (float)si;
    if (si < 0) { f = 0.f; si = 0; }
    if (si >= slen - 1) { f = 0.f; si = slen - 1; }
    s = si;
    a0 = 1.f - f;
    a1 = f;
}

// One wave per 256 source columns and a run of source rows (rows per wave =
// H / (4 gridDim.y), rounded up): lane l holds columns c, c + 1 for c = base +
// 2l and c = base + 128 + 2l -- one 8-byte load per row and half, 512 B
// contiguous per wave -- and takes its neighbours c - 1, c + 2 from lanes l - 1
// / l + 1 by DPP (lanes 0 / 63 from the other half or one extra load per row).
// Each source row's horizontal interpolation is formed once and kept in a
// 3-row ring; rows 2m, 2m + 1 are then one 16-byte store per half whose 64
// lanes cover 1 KB contiguously.  Away from the left and right borders every
// horizontal output takes the fixed weights (0.25, 0.75) / (0.75, 0.25) --
// up_coeff's values there, in the same operation order; border lanes and every
// vertical step take up_coeff.  (Measured, round 6, per 16-frame 1920x1200
// launch: one output per thread 408 us (1.8 TB/s); 16 outputs per thread with
// two 16-byte stores 32 B apart 330; one wave per row with contiguous stores
// and three loads per window 242 -- 167 of it with the loads removed.)
template <typename T>
__global__ __launch_bounds__(256) void k_upsample2x(const T* __restrict__ src, int spitch, int W, int H,
                                                    float* __restrict__ dst, int dpitch, long sfs, long dfs) {
    src = fptr(src, blockIdx.z * sfs);  // frame blockIdx.z
    dst = fptr(dst, blockIdx.z * dfs);
    const int per = (H + 4 * (int)gridDim.y - 1) / (4 * (int)gridDim.y);  // source rows per wave
    const int m0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * per;
    if (m0 >= H) return;  // wave-uniform
    const int mEnd = min(m0 + per, H);
    const int lane = threadIdx.x & 63, base = blockIdx.x * 256;
    const int c[2] = {base + 2 * lane, base + 128 + 2 * lane};
    const int xe = lane == 0 ? max(base - 1, 0) : min(base + 256, W - 1);  // lanes 0 / 63: outer columns
    const bool vec = sizeof(T) == 4 && (reinterpret_cast<uintptr_t>(src) & 7) == 0 && (spitch & 1) == 0;
    struct Raw {
        float v[2][2], e;
    };
    // Source row y (clamped), columns clamped to the row: every lane's window
    // is src[clamp(c - 1 .. c + 2)].
    auto load = [&](int y, Raw& r) {
        const T* row = src + (size_t)min(max(y, 0), H - 1) * spitch;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (vec && c[h] + 1 < W) {
                const float2 q = *reinterpret_cast<const float2*>(row + c[h]);
                r.v[h][0] = q.x;
                r.v[h][1] = q.y;
            } else {
                r.v[h][0] = (float)row[min(c[h], W - 1)];
                r.v[h][1] = (float)row[min(c[h] + 1, W - 1)];
            }
        }
        r.e = (float)row[xe];
    };
    auto horiz = [&](const Raw& r, float (&hh)[8]) {
        float w[2][4];
        const float a1_63 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.v[0][1]), 63));
        const float b0_0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.v[1][0]), 0));
        w[0][0] = dpp_left_or(r.e, r.v[0][1]);
        w[0][3] = dpp_right_or(b0_0, r.v[0][0]);
        w[1][0] = dpp_left_or(a1_63, r.v[1][1]);
        w[1][3] = dpp_right_or(r.e, r.v[1][0]);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            w[h][1] = r.v[h][0];
            w[h][2] = r.v[h][1];
            if (c[h] >= 1 && c[h] + 2 < W) {
                hh[4 * h] = w[h][0] * 0.25f + w[h][1] * 0.75f;
                hh[4 * h + 1] = w[h][1] * 0.75f + w[h][2] * 0.25f;
                hh[4 * h + 2] = w[h][1] * 0.25f + w[h][2] * 0.75f;
                hh[4 * h + 3] = w[h][2] * 0.75f + w[h][3] * 0.25f;
            } else {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    int sx;
                    float ax0, ax1;
                    up_coeff(min(2 * c[h] + t, 2 * W - 1), W, sx, ax0, ax1);
                    const int k0 = min(max(sx - c[h] + 1, 0), 3), k1 = min(max(min(sx + 1, W - 1) - c[h] + 1, 0), 3);
                    const float s0 = k0 == 0 ? w[h][0] : (k0 == 1 ? w[h][1] : (k0 == 2 ? w[h][2] : w[h][3]));
                    const float s1 = k1 == 0 ? w[h][0] : (k1 == 1 ? w[h][1] : (k1 == 2 ? w[h][2] : w[h][3]));
                    hh[4 * h + t] = s0 * ax0 + s1 * ax1;
                }
            }
        }
    };
    Raw rr;
    float hp[8], hc[8], hn[8];
    load(m0 - 1, rr);
    horiz(rr, hp);
    load(m0, rr);
    horiz(rr, hc);
    load(m0 + 1, rr);
    for (int m = m0; m < mEnd; m++) {
        horiz(rr, hn);                  // source row m + 1
        if (m + 1 < mEnd) load(m + 2, rr);  // one row ahead of the stores
#pragma unroll
        for (int v = 0; v < 2; v++) {
            int sy;
            float ay0, ay1;
            up_coeff(2 * m + v, H, sy, ay0, ay1);  // sy in {m - 1, m}, its successor in {m, m + 1}
            const bool r0c = sy == m, r1c = min(sy + 1, H - 1) == m;
            float o[8];
#pragma unroll
            for (int i = 0; i < 8; i++) o[i] = (r0c ? hc[i] : hp[i]) * ay0 + (r1c ? hc[i] : hn[i]) * ay1;
            float* d = dst + (size_t)(2 * m + v) * dpitch;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (c[h] + 2 <= W) {
                    *reinterpret_cast<float4*>(d + 2 * c[h]) = make_float4(o[4 * h], o[4 * h + 1], o[4 * h + 2], o[4 * h + 3]);
                } else if (c[h] < W) {  // W odd: the row's last two outputs
                    d[2 * c[h]] = o[4 * h];
                    d[2 * c[h] + 1] = o[4 * h + 1];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            hp[i] = hc[i];
            hc[i] = hn[i];
        }
    }
}

// Source rows per wave: 8 for frame batches (fewer, longer-lived waves), 2
// for a single frame (more waves in flight).
dim3 up_grid(int W, int H, int nf) {
    const int per = nf > 1 ? 8 : 2;
    return dim3((W + 255) / 256, (H + 4 * per - 1) / (4 * per), nf);
}

void launch_upsample2x(const float* src, int spitch, int W, int H, float* dst, int dpitch, const Frames& fr, long sfs,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_upsample2x<float>, up_grid(W, H, fr.nf), dim3(256), 0, s, src, spitch, W, H, dst, dpitch, sfs,
                       fr.stride);
}

void launch_upsample2x_u8(const uint8_t* src, int spitch, int W, int H, float* dst, int dpitch, const Frames& fr,
                          long sfs, hipStream_t s) {
    hipLaunchKernelGGL(k_upsample2x<uint8_t>, up_grid(W, H, fr.nf), dim3(256), 0, s, src, spitch, W, H, dst, dpitch, sfs, fr.stride);
}

// The kernel node launch_upsample2x would make (the head node of a captured
// frame graph: head_blur_node, blur.hip).
void head_upsample_node(HeadNode& h, const float* src, int spitch, int W, int H, float* dst, int dpitch,
                        const Frames& fr, long sfs) {
    // k_upsample2x<float>(src, spitch, W, H, dst, dpitch, sfs, dfs): each argument at its own slot.
    unsigned char* a = h.args;
    auto put = [&](int i, const void* v, size_t n) {
        std::memcpy(a + 16 * i, v, n);
        h.argv[i] = a + 16 * i;
    };
    put(0, &src, sizeof src);
    put(1, &spitch, sizeof spitch);
    put(2, &W, sizeof W);
    put(3, &H, sizeof H);
    put(4, &dst, sizeof dst);
    put(5, &dpitch, sizeof dpitch);
    put(6, &sfs, sizeof sfs);
    put(7, &fr.stride, sizeof fr.stride);
    h.p = hipKernelNodeParams{};
    h.p.func = reinterpret_cast<void*>(&k_upsample2x<float>);
    h.p.gridDim = up_grid(W, H, fr.nf);
    h.p.blockDim = dim3(256);
    h.p.sharedMemBytes = 0;
    h.p.kernelParams = h.argv;
    h.p.extra = nullptr;
}

__global__ __launch_bounds__(256) void k_u8_to_f32(const uint8_t* __restrict__ src, int spitch, int W, int H,
                                                   float* __restrict__ dst, int dpitch, long sfs, long dfs) {
    src = fptr(src, blockIdx.z * sfs);
    dst = fptr(dst, blockIdx.z * dfs);
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x < W) dst[(size_t)y * dpitch + x] = (float)src[(size_t)y * spitch + x];
}

void launch_u8_to_f32(const uint8_t* src, int spitch, int W, int H, float* dst, int dpitch, const Frames& fr,
                      long sfs, hipStream_t s) {
    hipLaunchKernelGGL(k_u8_to_f32, dim3((W + 255) / 256, H, fr.nf), dim3(256), 0, s, src, spitch, W, H, dst, dpitch,
                       sfs, fr.stride);
}

}  // namespace sift_amd
