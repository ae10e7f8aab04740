// Pyramid tail for gfx950: every blur of a frame's small octaves in one
// workgroup, planes held in LDS.  The operations and their order are
// blur_tile's (sift_blur_dev.h), so the planes are the same bits.
#include <algorithm>

#include "sift_kernels.h"
#include "sift_math.h"

namespace sift_amd {

// ---------------------------------------------------------------------------
// Pyramid tail: every blur of the small octaves o >= T of a frame in ONE
// workgroup (1024 threads, one per frame), planes held in LDS.  A single
// frame's small octaves were one launch per blur job (752x480, auto octaves:
// 14 launches of 1-2 tiles for octaves 3..6, ~5 us each: the launch and one
// tile's load -> LDS -> passes -> store chain, almost none of it work); here
// octave T's base plane is read once and every plane is blurred LDS -> LDS
// with the operations of blur_tile in the same order (OpenCV's sepFilter2D:
// the row filter, then the symmetric column filter; reflect-101 borders,
// looping for kernels wider than the octave), stored for the keypoint stages,
// and plane L's even rows and columns become the next octave's base (LDS and
// HBM).  Row pass A -> B, column pass B -> A; the LDS rows have an odd pitch:
// the row pass gives consecutive lanes consecutive rows, the column pass
// consecutive columns (conflict-free both ways).  The taps of the plane are
// staged in LDS (wave-uniform reads).  The octaves it takes are bounded by
// work, not LDS: one CU's VALU runs the whole tail (tail_first_octave).
// ---------------------------------------------------------------------------
constexpr int kTailThreads = 1024;
constexpr int kTailRun = 4;     // outputs per thread and run (along the pass)
constexpr int kTailRmax = 16;   // radius bound of the tail's unrolled windows
constexpr int kTailMaxDim = 512;  // octave width / height bound (reflection tables)

__host__ __device__ __forceinline__ int tail_pitch(int W) { return W | 1; }

// HBM stores as global_store (not flat: a flat store counts on lgkmcnt too,
// so the next run's LDS wait would also wait for it).  The tail's barriers
// fence LDS only (lds_barrier): __syncthreads() would wait for every plane
// store to be acknowledged before the next pass (56 us for 752x480's tail);
// the planes are read by later launches only.
__device__ __forceinline__ void gstore(float* p, size_t i, float v) {
    ((__attribute__((address_space(1))) float*)p)[i] = v;
}
__device__ __forceinline__ float gload(const float* p, size_t i) {
    return ((const __attribute__((address_space(1))) float*)p)[i];
}

// One instantiation per radius class RP (the largest radius of the tail's
// planes, rounded up to 4, 8, 13 or 16), every plane's taps zero-padded to
// 2 RP + 1: in these sums every term is >= 0 (non-negative pixels and taps),
// so a zero-weight fma adds a signed zero to a non-negative sum and leaves it
// bit-identical, and a leading one leaves s = +0 until the first real tap --
// the padded chain is OpenCV's chain.  (Per-radius instantiations dispatched
// per plane: 56 us for 752x480's tail, its code cold in the instruction cache
// at every plane.)  The window loads of a run are all issued before its
// first fma.
template <int RP>
__device__ __forceinline__ void tail_row_pass(const float* __restrict__ A, float* __restrict__ B, int W, int H, int P,
                                              bool small, const float* __restrict__ wp, const int* __restrict__ xo) {
    constexpr int NWIN = kTailRun + 2 * RP;
    const int nrx = (W + kTailRun - 1) / kTailRun, nruns = nrx * H;
    for (int r = threadIdx.x; r < nruns; r += kTailThreads) {
        const int y = r % H, xb = (r / H) * kTailRun;  // consecutive lanes: consecutive rows
        const float* row = A + y * P;
        // Source column of window slot k: xb - RP + k (runs at the borders
        // through the reflection table xo[j] = reflect101(j - RP), j = xb + k).
        float win[NWIN];
        if (xb - RP >= 0 && xb + kTailRun - 1 + RP < W) {
#pragma unroll
            for (int k = 0; k < NWIN; k++) win[k] = row[xb - RP + k];
        } else {
            int ix[NWIN];
#pragma unroll
            for (int k = 0; k < NWIN; k++) ix[k] = xo[xb + k];
#pragma unroll
            for (int k = 0; k < NWIN; k++) win[k] = row[ix[k]];
        }
        float s[kTailRun];
        if (!small) {  // RowFilter: s = 0; s = fma(x[k], w[k], s), k = 0..2R
#pragma unroll
            for (int q = 0; q < kTailRun; q++) s[q] = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * RP; k++) {
                const float wk = wp[k];
#pragma unroll
                for (int q = 0; q < kTailRun; q++) s[q] = __fmaf_rn(win[q + k], wk, s[q]);
            }
        } else {  // SymmRowSmall (2R + 1 <= 5): s = x0 w0; s = fma(x[-k] + x[+k], w_k, s)
            const float wc = wp[RP];
#pragma unroll
            for (int q = 0; q < kTailRun; q++) s[q] = win[q + RP] * wc;
#pragma unroll
            for (int k = 1; k <= 2 && k <= RP; k++) {
                const float wk = wp[RP + k];
#pragma unroll
                for (int q = 0; q < kTailRun; q++) s[q] = __fmaf_rn(win[q + RP - k] + win[q + RP + k], wk, s[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < kTailRun; q++)
            if (xb + q < W) B[y * P + xb + q] = s[q];
    }
}

// Column pass (SymmColumnFilter: s = fma(c, w_R, 0); s = fma(down_k + up_k,
// w_{R+k}, s)) B -> A and the plane to HBM; with `dec`, the even rows and
// columns also go to the next octave's base (LDS N and HBM).
template <int RP>
__device__ __forceinline__ void tail_col_pass(const float* __restrict__ B, float* __restrict__ A, int W, int H, int P,
                                              const float* __restrict__ wp, const int* __restrict__ yo,
                                              float* __restrict__ gdst, int gpitch, bool dec, float* __restrict__ N,
                                              int NP, float* __restrict__ gnext, int gnpitch) {
    constexpr int NWIN = kTailRun + 2 * RP;
    const int nry = (H + kTailRun - 1) / kTailRun, nruns = nry * W;
    for (int r = threadIdx.x; r < nruns; r += kTailThreads) {
        const int x = r % W, yb = (r / W) * kTailRun;  // consecutive lanes: consecutive columns
        float win[NWIN];
        if (yb - RP >= 0 && yb + kTailRun - 1 + RP < H) {
#pragma unroll
            for (int k = 0; k < NWIN; k++) win[k] = B[(yb - RP + k) * P + x];
        } else {
            int iy[NWIN];
#pragma unroll
            for (int k = 0; k < NWIN; k++) iy[k] = yo[yb + k];
#pragma unroll
            for (int k = 0; k < NWIN; k++) win[k] = B[iy[k] * P + x];
        }
        float s[kTailRun];
        const float wc = wp[RP];
#pragma unroll
        for (int q = 0; q < kTailRun; q++) s[q] = __fmaf_rn(win[q + RP], wc, 0.f);
#pragma unroll
        for (int k = 1; k <= RP; k++) {
            const float wk = wp[RP + k];
#pragma unroll
            for (int q = 0; q < kTailRun; q++) s[q] = __fmaf_rn(win[q + RP + k] + win[q + RP - k], wk, s[q]);
        }
#pragma unroll
        for (int q = 0; q < kTailRun; q++) {
            const int y = yb + q;
            if (y < H) {
                A[y * P + x] = s[q];
#if !defined(SIFT_TAIL_DIAG) || SIFT_TAIL_DIAG != 4
                gstore(gdst, (size_t)y * gpitch + x, s[q]);
#endif
                if (dec && !((x | y) & 1) && (x >> 1) < (W >> 1) && (y >> 1) < (H >> 1)) {
                    N[(y >> 1) * NP + (x >> 1)] = s[q];
                    gstore(gnext, (size_t)(y >> 1) * gnpitch + (x >> 1), s[q]);
                }
            }
        }
    }
}

template <int RP>
__device__ __forceinline__ void tail_octaves(const TailDesc& T, float* lds, const float (*wall)[2 * kTailRmax + 1],
                                             int* xo, int* yo, long foff) {
    int aOff = 0, nOff = T.regionX;
    const int bOff = T.regionX + T.regionY;
    for (int o = T.o0; o < T.nOct; o++) {
        const OctGeom& g = T.oct[o];
        const OctGeom& gn = T.oct[o + 1 < T.nOct ? o + 1 : o];
        float* base = fptr(g.base, foff);
        const int P = tail_pitch(g.W);
        // Reflection tables for the padded radius (the same for every plane).
        lds_barrier();
        const int t = threadIdx.x;
        if (t < g.W + 2 * RP + kTailRun) xo[t] = reflect101(min(t - RP, g.W - 1 + RP), g.W);
        if (t < g.H + 2 * RP + kTailRun) yo[t] = reflect101(min(t - RP, g.H - 1 + RP), g.H);
        for (int i = 1; i < T.L + 3; i++) {
#if defined(SIFT_TAIL_DIAG) && SIFT_TAIL_DIAG == 5  // timing builds only: s_memtime per plane -> octave 0, plane 0
            if (threadIdx.x == 0) {
                const unsigned long long t0 = __builtin_amdgcn_s_memtime();
                unsigned* st = reinterpret_cast<unsigned*>(fptr(T.oct[0].base, foff));
                const int slot = (o - T.o0) * (T.L + 2) + (i - 1);
                st[2 * slot] = (unsigned)t0;
                st[2 * slot + 1] = (unsigned)(t0 >> 32);
            }
#endif
            const bool small = T.taps[i].n <= 5, dec = o + 1 < T.nOct && i == T.L;
            const float* wp = wall[i];
            lds_barrier();  // A written (load / previous column pass); tables set
#if !defined(SIFT_TAIL_DIAG) || SIFT_TAIL_DIAG != 1  // timing-variant builds only (tools/ab_variant.sh)
            tail_row_pass<RP>(lds + aOff, lds + bOff, g.W, g.H, P, small, wp, xo);
#endif
            lds_barrier();
#if !defined(SIFT_TAIL_DIAG) || SIFT_TAIL_DIAG != 2
            tail_col_pass<RP>(lds + bOff, lds + aOff, g.W, g.H, P, wp, yo, base + (size_t)i * g.planeStride, g.pitch,
                              dec, lds + nOff, tail_pitch(gn.W), dec ? fptr(gn.base, foff) : base, gn.pitch);
#endif
        }
        const int tt = aOff;  // the next octave works on its base; its own next base goes where this plane was
        aOff = nOff;
        nOff = tt;
    }
}

__global__ __launch_bounds__(kTailThreads) void k_blur_tail(TailDesc T, long fs) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float wall[kTailMaxPlanes][2 * kTailRmax + 1];  // every plane's taps, zero-padded to 2 RP + 1
    __shared__ int xo[kTailMaxDim + 2 * kTailRmax + kTailRun], yo[kTailMaxDim + 2 * kTailRmax + kTailRun];
    const long foff = (long)blockIdx.x * fs;
    const int RP = T.rpad;
    // LDS (float offsets into lds, not pointers, so every access stays a
    // ds_*): A = the plane (region X, then the next base's region,
    // alternating), B = the row pass's output, N = the next octave's base.
    {
        // Taps from the kernel arguments, padded: one round of loads here
        // instead of a dependent kernarg load before every plane.
        for (int t = threadIdx.x; t < kTailMaxPlanes * (2 * kTailRmax + 1); t += kTailThreads) {
            const int i = t / (2 * kTailRmax + 1), k = t - i * (2 * kTailRmax + 1);
            float v = 0.f;
            if (i < T.L + 3 && k <= 2 * RP) {
                const int R = T.taps[i].n >> 1, kk = k - RP + R;
                if (kk >= 0 && kk <= 2 * R) v = T.taps[i].w[kk];
            }
            wall[i][k] = v;
        }
        const OctGeom& g = T.oct[T.o0];
        const float* src = fptr(g.base, foff);
        const int P = tail_pitch(g.W);
        for (int i = threadIdx.x; i < g.W * g.H; i += kTailThreads) {
            const int y = i / g.W, x = i - y * g.W;
            lds[y * P + x] = gload(src, (size_t)y * g.pitch + x);
        }
    }
#if defined(SIFT_TAIL_DIAG) && SIFT_TAIL_DIAG == 3
    return;
#endif
    switch (RP) {
        case 4: tail_octaves<4>(T, lds, wall, xo, yo, foff); break;
        case 8: tail_octaves<8>(T, lds, wall, xo, yo, foff); break;
        case 13: tail_octaves<13>(T, lds, wall, xo, yo, foff); break;
        default: tail_octaves<16>(T, lds, wall, xo, yo, foff); break;
    }
}

constexpr long kTailMaxPx = 6000;  // largest octave the tail takes (one CU's VALU: 752x480 octave 3 = 94x60; 1920x1200 octave 4 (120x75) lost 10-20 us)
int tail_first_octave(const PyrDesc& pyr, const Taps* taps, int L) {
    for (int i = 1; i < L + 3; i++)
        if ((taps[i].n >> 1) > kTailRmax) return pyr.nOct;
    int T = pyr.nOct;
    for (int o = pyr.nOct - 1; o >= 0; o--) {
        const OctGeom& g = pyr.oct[o];
        const long px = (long)tail_pitch(g.W) * g.H;
        const long nxt = o + 1 < pyr.nOct ? (long)tail_pitch(pyr.oct[o + 1].W) * pyr.oct[o + 1].H : 0;
        if ((long)g.W * g.H > kTailMaxPx || 2 * px + nxt > kTailLdsFloats || g.W > kTailMaxDim ||
            g.H > kTailMaxDim)
            break;
        T = o;
    }
    return T;
}

hipError_t tail_init() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_blur_tail),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * kTailLdsFloats));
}

void launch_blur_tail(const PyrDesc& pyr, const Taps* taps, int L, int o0, const Frames& fr, hipStream_t s) {
    TailDesc T{};
    T.o0 = o0;
    T.nOct = pyr.nOct;
    T.L = L;
    for (int o = 0; o < pyr.nOct; o++) T.oct[o] = pyr.oct[o];
    for (int i = 0; i < L + 3 && i < kTailMaxPlanes; i++) T.taps[i] = taps[i];
    int rmax = 0;
    for (int i = 1; i < L + 3; i++) rmax = std::max(rmax, taps[i].n >> 1);
    T.rpad = rmax <= 4 ? 4 : rmax <= 8 ? 8 : rmax <= 13 ? 13 : 16;
    T.regionX = tail_pitch(pyr.oct[o0].W) * pyr.oct[o0].H;
    T.regionY = o0 + 1 < pyr.nOct ? tail_pitch(pyr.oct[o0 + 1].W) * pyr.oct[o0 + 1].H : 0;
    const size_t lds = sizeof(float) * (size_t)(2 * T.regionX + T.regionY);
    hipLaunchKernelGGL(k_blur_tail, dim3(fr.nf), dim3(kTailThreads), lds, s, T, fr.stride);
}

}  // namespace sift_amd
