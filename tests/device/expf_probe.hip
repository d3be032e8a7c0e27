// Test-only device probe of ul_expf (uhsdr_amd/csrc/uhsdr_libm_expf.h) for tests/test_gpu_expf.py, built
// by the Makefile with exactly $(HIPFLAGS), the product's flags, into
// tests/build/libuhsdr_expf_probe.so, as libm_probe.hip is: the header's device build, its
// double-precision fma chain and its __constant__ table are then the ones the noise-reduction kernel
// gets.  Nothing here is linked into libuhsdr_amd.so.
//
// One thread per operand; device pointers, a count (at most 2^24 per launch, the test's chunk) and a
// stream; returns the hipError_t of the launch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../uhsdr_amd/csrc/uhsdr_libm_expf.h"

#define PROBE_MAX ((size_t)1 << 24)
#define PROBE_BLOCK 256

__global__ void k_expf(const float* x, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = ul_expf(x[i]);
}

extern "C" int uld_expf(const float* x, float* r, size_t n, hipStream_t stream)
{
    if (n > PROBE_MAX) return (int)hipErrorInvalidValue;
    if (n == 0) return (int)hipSuccess;
    hipLaunchKernelGGL(k_expf, dim3((unsigned)((n + PROBE_BLOCK - 1) / PROBE_BLOCK)), dim3(PROBE_BLOCK), 0, stream, x, r, n);
    return (int)hipGetLastError();
}
