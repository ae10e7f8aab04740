// Stand-alone RootSIFT transform of fp16 descriptor rows (sift_hip_rootsift_*):
// rows the detector did not write in SIFT_HIP_NORM_ROOT -- a database's
// descriptors, a frame the caller kept, another extractor's rows.  The rule is
// sift_rootsift.h, the one the descriptor kernels' root epilogue applies.
//
// One wave per row, two entries per lane (one packed dword load and store), a
// grid-stride loop over rows.  A lane reads and writes only its own two
// entries and the wave's sum separates the two, so desc_out == desc_in is safe.
// Traffic is the floor, 512 B per row; small calls are launch-bound.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "detector_state.h"
#include "sift_math.h"
#include "sift_rootsift.h"

namespace sift_amd {

constexpr int kRootWaves = 4;  // rows per workgroup and step

// kPacked: both pointers are 4-byte aligned (every hipMalloc'ed buffer); else
// the two entries move as 16-bit accesses.
template <bool kPacked>
__global__ __launch_bounds__(64 * kRootWaves) void k_rootsift(const uint16_t* in, uint16_t* out, int n) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (long row = (long)blockIdx.x * kRootWaves + w; row < n; row += (long)gridDim.x * kRootWaves) {
        const uint16_t* src = in + row * 128 + 2 * lane;
        uint16_t* dst = out + row * 128 + 2 * lane;
        unsigned pair;
        if (kPacked) pair = *reinterpret_cast<const unsigned*>(src);
        else pair = (unsigned)src[0] | (unsigned)src[1] << 16;
        const int b0 = root_input_byte((float)__builtin_bit_cast(_Float16, (uint16_t)(pair & 0xffffu)));
        const int b1 = root_input_byte((float)__builtin_bit_cast(_Float16, (uint16_t)(pair >> 16)));
        const int s = __builtin_amdgcn_readlane(wave_incl_scan(b0 + b1), 63);
        const _Float16 h0 = (_Float16)(float)root_byte(b0, s), h1 = (_Float16)(float)root_byte(b1, s);
        const unsigned o = (unsigned)__builtin_bit_cast(uint16_t, h0) | (unsigned)__builtin_bit_cast(uint16_t, h1) << 16;
        if (kPacked) {
            *reinterpret_cast<unsigned*>(dst) = o;
        } else {
            dst[0] = (uint16_t)(o & 0xffffu);
            dst[1] = (uint16_t)(o >> 16);
        }
    }
}

namespace {
int check_rows(const uint16_t* in, int n, const uint16_t* out) {
    if (n < 0) return fail(SIFT_HIP_ERR_INVALID, "negative row count");
    if (n == 0) return SIFT_HIP_OK;
    if (!in || !out) return fail(SIFT_HIP_ERR_INVALID, "null descriptor rows");
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, len = (uintptr_t)n * 256;
    if ((a | b) & 1) return fail(SIFT_HIP_ERR_INVALID, "descriptor rows not 2-byte aligned");
    if (a != b && a < b + len && b < a + len)
        return fail(SIFT_HIP_ERR_INVALID, "desc_in and desc_out overlap (in place is desc_out == desc_in)");
    return SIFT_HIP_OK;
}

void launch_rootsift(const uint16_t* in, int n, uint16_t* out, hipStream_t s) {
    // Rows per workgroup step x enough workgroups to fill the chip; larger n loops.
    const int grid = std::min((n + kRootWaves - 1) / kRootWaves, 4096);
    if ((((uintptr_t)in | (uintptr_t)out) & 3) == 0)
        hipLaunchKernelGGL(k_rootsift<true>, dim3(grid), dim3(64 * kRootWaves), 0, s, in, out, n);
    else
        hipLaunchKernelGGL(k_rootsift<false>, dim3(grid), dim3(64 * kRootWaves), 0, s, in, out, n);
}
}  // namespace

}  // namespace sift_amd

extern "C" {

int sift_hip_rootsift_device(const uint16_t* desc_in, int n, uint16_t* desc_out, void* stream) {
    if (int rc = check_rows(desc_in, n, desc_out)) return rc;
    if (n == 0) return SIFT_HIP_OK;
    launch_rootsift(desc_in, n, desc_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

int sift_hip_rootsift_host(const uint16_t* desc_in, int n, uint16_t* desc_out) {
    if (int rc = check_rows(desc_in, n, desc_out)) return rc;
    if (n == 0) return SIFT_HIP_OK;
    const size_t bytes = (size_t)n * 256;
    uint16_t* dev = nullptr;
    if (hipMalloc((void**)&dev, bytes) != hipSuccess) return fail(SIFT_HIP_ERR_NOMEM, "hipMalloc of the descriptor rows failed");
    hipError_t e = hipMemcpy(dev, desc_in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_rootsift(dev, n, dev, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(desc_out, dev, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(SIFT_HIP_ERR_RUNTIME, std::string("sift_hip_rootsift_host: ") + hipGetErrorString(e));
    return SIFT_HIP_OK;
}

}  // extern "C"
