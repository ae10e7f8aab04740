// Gaussian blur of the pyramid planes for gfx950: one blur job per launch
// (k_blur: every radius 1 .. kMaxTaps / 2, and the frame's first blur of an
// 8-bit frame) or two (k_blur2: the radius pairs of the default pyramid).
//
// Replaces the reference's sift_cuda/image_func/Filter.cu.  Semantics follow
// OpenCV 4.x; the float operation order is
// the oracle's (oracle/sift_oracle.cpp gaussianBlur), so planes are bit-exact.
// The tile body is blur_tile (sift_blur_dev.h).
//
// k_blur and k_blur2 share this unit on purpose: compiled apart, the ten
// k_blur<R, float, NW> whose blur_tile<R> a pair kernel also inlines (R = 5, 6,
// 8, 10, 13) come out with other register choices and instruction order than
// the kernels measured in profiles/ (the same arithmetic; blur_tile<R, float,
// NW> then has one caller in its unit instead of five).
#include <array>
#include <cstring>
#include <utility>

#include "sift_blur_dev.h"

namespace sift_amd {

template <int R, typename T, int NW>
__global__ __launch_bounds__(64 * NW) void k_blur(BlurJob J) {
    __shared__ __attribute__((aligned(16))) float in[blur_lds_floats<R>()];
    blur_tile<R, T, NW>(J, blockIdx.x, in);
}

// Two independent blur jobs in one launch (blocks [0, A.ntiles) take A): the
// first blurs of octave o+1 run beside the last blurs of octave o, which they
// do not depend on, so a frame needs fewer launches (each costs ~0.7-1.5 us of
// dispatch) and small-octave tiles fill CUs the larger
// job leaves idle.
template <int RA, int RB, int NW>
__global__ __launch_bounds__(64 * NW) void k_blur2(BlurJob A, BlurJob B) {
    constexpr int NA = blur_lds_floats<RA>(), NB = blur_lds_floats<RB>();
    __shared__ __attribute__((aligned(16))) float in[NA > NB ? NA : NB];
    const int na = A.ntiles * A.nf;
    if ((int)blockIdx.x < na)
        blur_tile<RA, float, NW>(A, blockIdx.x, in);
    else
        blur_tile<RB, float, NW>(B, blockIdx.x - na, in);
}

using BlurLaunch = void (*)(const BlurJob&, hipStream_t);

template <int R>
void blur_launch_r(const BlurJob& j, hipStream_t s) {
    const int tiles = j.ntiles * j.nf;
    if (blur_waves(tiles) == 4)
        hipLaunchKernelGGL((k_blur<R, float, 4>), dim3(tiles), dim3(256), 0, s, j);
    else
        hipLaunchKernelGGL((k_blur<R, float, 8>), dim3(tiles), dim3(512), 0, s, j);
}

template <int... Rs>
constexpr std::array<BlurLaunch, sizeof...(Rs)> blur_table(std::integer_sequence<int, Rs...>) {
    return {&blur_launch_r<Rs + 1>...};
}
static const std::array<BlurLaunch, kMaxTaps / 2> kBlurTable = blur_table(std::make_integer_sequence<int, kMaxTaps / 2>{});

// Pair instantiations: the radii of the default pyramid (sigma 1.6, 3 layers:
// 5, 6, 8, 10, 13), larger radius first.  Other pairs launch separately.
template <int RA, int RB>
void blur2_launch(const BlurJob& a, const BlurJob& b, hipStream_t s) {
    const int tiles = a.ntiles * a.nf + b.ntiles * b.nf;
    if (blur_waves(tiles) == 4)
        hipLaunchKernelGGL((k_blur2<RA, RB, 4>), dim3(tiles), dim3(256), 0, s, a, b);
    else
        hipLaunchKernelGGL((k_blur2<RA, RB, 8>), dim3(tiles), dim3(512), 0, s, a, b);
}
bool launch_blur_pair_jobs(const BlurJob& a, const BlurJob& b, hipStream_t s) {
    const int ra = a.taps.n >> 1, rb = b.taps.n >> 1;
#define SIFT_PAIR(X, Y)                      \
    if (ra == X && rb == Y) {                \
        blur2_launch<X, Y>(a, b, s);         \
        return true;                         \
    }                                        \
    if (ra == Y && rb == X) {                \
        blur2_launch<X, Y>(b, a, s);         \
        return true;                         \
    }
    SIFT_PAIR(6, 5)
    SIFT_PAIR(8, 5)
    SIFT_PAIR(8, 6)
    SIFT_PAIR(10, 5)
    SIFT_PAIR(10, 6)
    SIFT_PAIR(10, 8)
    SIFT_PAIR(13, 5)
    SIFT_PAIR(13, 6)
    SIFT_PAIR(13, 8)
    SIFT_PAIR(13, 10)
#undef SIFT_PAIR
    return false;
}

bool launch_blur_pair(const BlurDesc& a, const BlurDesc& b, const Frames& fr, hipStream_t s) {
    return launch_blur_pair_jobs(make_job(a.src, a.spitch, a.W, a.H, a.dst, a.dpitch, a.dec, *a.taps,
                                          nullptr, nullptr, fr, fr.stride),
                                 make_job(b.src, b.spitch, b.W, b.H, b.dst, b.dpitch, b.dec, *b.taps,
                                          nullptr, nullptr, fr, fr.stride),
                                 s);
}

bool launch_blur_u8(const uint8_t* src, int spitch, int W, int H, float* dst, int dpitch, const Taps& taps,
                    const Frames& fr, long sfs, hipStream_t s, unsigned* range_keys, Counters* zero_ctr) {
    const BlurJob j = make_job(src, spitch, W, H, dst, dpitch, DecOut{}, taps, range_keys, zero_ctr, fr, sfs);
    const int tiles = j.ntiles * j.nf;
    const bool big = blur_waves(tiles) == 4;
    switch (taps.n >> 1) {
        case 5:
            if (big) hipLaunchKernelGGL((k_blur<5, uint8_t, 4>), dim3(tiles), dim3(256), 0, s, j);
            else hipLaunchKernelGGL((k_blur<5, uint8_t, 8>), dim3(tiles), dim3(512), 0, s, j);
            return true;
        case 6:
            if (big) hipLaunchKernelGGL((k_blur<6, uint8_t, 4>), dim3(tiles), dim3(256), 0, s, j);
            else hipLaunchKernelGGL((k_blur<6, uint8_t, 8>), dim3(tiles), dim3(512), 0, s, j);
            return true;
        default: return false;
    }
}

// The kernel node launch_blur (without a decimated output) and
// launch_upsample2x would make, for a captured frame graph whose head node
// is re-pointed at each frame's input (hipGraphExecKernelNodeSetParams).
template <int R>
const void* blur_fn(int nw) {
    return nw == 4 ? reinterpret_cast<const void*>(&k_blur<R, float, 4>)
                   : reinterpret_cast<const void*>(&k_blur<R, float, 8>);
}
template <int... Rs>
constexpr std::array<const void* (*)(int), sizeof...(Rs)> blur_fn_table(std::integer_sequence<int, Rs...>) {
    return {&blur_fn<Rs + 1>...};
}
static const std::array<const void* (*)(int), kMaxTaps / 2> kBlurFnTable =
    blur_fn_table(std::make_integer_sequence<int, kMaxTaps / 2>{});
static_assert(sizeof(BlurJob) <= sizeof(HeadNode::args), "head node argument storage");

void head_blur_node(HeadNode& h, const float* src, int spitch, int W, int H, float* dst, int dpitch, const Taps& taps,
                    const Frames& fr, long sfs, unsigned* range_keys, Counters* zero_ctr) {
    const BlurJob j = make_job(src, spitch, W, H, dst, dpitch, DecOut{}, taps, range_keys, zero_ctr, fr, sfs);
    const int tiles = j.ntiles * j.nf, nw = blur_waves(tiles);
    std::memcpy(h.args, &j, sizeof j);
    h.argv[0] = h.args;
    h.p = hipKernelNodeParams{};
    h.p.func = const_cast<void*>(kBlurFnTable[(taps.n >> 1) - 1](nw));
    h.p.gridDim = dim3(tiles);
    h.p.blockDim = dim3(64 * nw);
    h.p.sharedMemBytes = 0;
    h.p.kernelParams = h.argv;
    h.p.extra = nullptr;
}

void launch_blur(const float* src, int spitch, int W, int H, float* dst, int dpitch, const DecOut& dec,
                 const Taps& taps, const Frames& fr, long sfs, hipStream_t s, unsigned* range_keys,
                 Counters* zero_ctr) {
    const int r = taps.n >> 1;  // 1 .. kMaxTaps/2 (taps.n >= 3 by construction)
    kBlurTable[r - 1](make_job(src, spitch, W, H, dst, dpitch, dec, taps, range_keys, zero_ctr, fr, sfs), s);
}

}  // namespace sift_amd
