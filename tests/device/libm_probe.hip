// Test-only device probe of uhsdr_amd/csrc/uhsdr_libm.h and of the bare IEEE primitives the
// chain assumes (tests/test_gpu_libm.py).  Built by the Makefile with exactly $(HIPFLAGS), the
// product's flags, into tests/build/libuhsdr_libm_probe.so: the header's device build, the
// compiler's device expansions of binary32 divide and sqrtf, the double-precision fma chain and
// the __constant__ table are then the ones the receive kernels get.  Nothing here is linked into
// libuhsdr_amd.so.
//
// One thread per operand; every entry point takes device pointers, a count (at most 2^24 per
// launch, the test's chunk) and a stream, and returns the hipError_t of the launch.
//
// Probed: ul_sincosf, ul_atan2f, ul_atanf_pos (as built, and once more with the IEEE quotient in
// place of the short division), ul_asinf, sqrtf(a), a / b, and the two mixed-precision
// recursions of the chain (uhsdr_spectrum.hip auto-I/Q low-pass, uhsdr_rx.hip FM squelch average).
// ul_atanf, the signed form, is called by no kernel and is deliberately not probed.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../uhsdr_amd/csrc/uhsdr_libm.h"

// the same header once more with UHSDR_ATAN_SHORTDIV 0, so the test can tell "the short
// division differs" from "the rest of ul_atanf_pos differs"
namespace ieeediv
{
#undef UHSDR_LIBM_H
#undef UHSDR_ATAN_SHORTDIV
#define UHSDR_ATAN_SHORTDIV 0
#include "../../uhsdr_amd/csrc/uhsdr_libm.h"
}

#define PROBE_MAX ((size_t)1 << 24)
#define PROBE_BLOCK 256

__global__ void k_sincosf(const float* y, float* s, float* c, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    float sv, cv;
    ul_sincosf(y[i], &sv, &cv);
    s[i] = sv;
    c[i] = cv;
}

__global__ void k_atan2f(const float* y, const float* x, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = ul_atan2f(y[i], x[i]);
}

__global__ void k_atanf_pos(const float* a, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = ul_atanf_pos(a[i]);
}

__global__ void k_atanf_pos_ieeediv(const float* a, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = ieeediv::ul_atanf_pos(a[i]);
}

__global__ void k_asinf(const float* a, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = ul_asinf(a[i]);
}

__global__ void k_sqrtf(const float* a, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = sqrtf(a[i]);
}

__global__ void k_divf(const float* a, const float* b, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = a[i] / b[i];
}

// uhsdr_spectrum.hip:125-127, one step of the auto-I/Q low-pass with both signs of c0
__global__ void k_iq_lowpass(const float* t, const float* o, float* rneg, float* rpos, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    rneg[i] = (float)(-0.003 * (double)(t[i] / 32.0f) + 0.997 * (double)o[i]);
    rpos[i] = (float)(0.003 * (double)(t[i] / 32.0f) + 0.997 * (double)o[i]);
}

// uhsdr_rx.hip:3184, one step of the FM squelch average
__global__ void k_squelch_avg(const float* t, const float* o, float* r, size_t n)
{
    const size_t i = (size_t)blockIdx.x * PROBE_BLOCK + threadIdx.x;
    if (i < n) r[i] = (float)(((1 - 0.005) * (double)o[i]) + (0.005 * (double)sqrtf(fabsf(t[i]))));
}

#define PROBE_LAUNCH(kernel, ...)                                                              \
    do {                                                                                       \
        if (n > PROBE_MAX) return (int)hipErrorInvalidValue;                                   \
        if (n == 0) return (int)hipSuccess;                                                    \
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + PROBE_BLOCK - 1) / PROBE_BLOCK)),      \
                           dim3(PROBE_BLOCK), 0, stream, __VA_ARGS__, n);                      \
        return (int)hipGetLastError();                                                         \
    } while (0)

extern "C" {

int uld_sincosf(const float* y, float* s, float* c, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_sincosf, y, s, c); }
int uld_atan2f(const float* y, const float* x, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_atan2f, y, x, r); }
int uld_atanf_pos(const float* a, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_atanf_pos, a, r); }
int uld_atanf_pos_ieeediv(const float* a, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_atanf_pos_ieeediv, a, r); }
int uld_asinf(const float* a, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_asinf, a, r); }
int uld_sqrtf(const float* a, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_sqrtf, a, r); }
int uld_divf(const float* a, const float* b, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_divf, a, b, r); }
int uld_iq_lowpass(const float* t, const float* o, float* rneg, float* rpos, size_t n, hipStream_t stream)
{
    PROBE_LAUNCH(k_iq_lowpass, t, o, rneg, rpos);
}
int uld_squelch_avg(const float* t, const float* o, float* r, size_t n, hipStream_t stream) { PROBE_LAUNCH(k_squelch_avg, t, o, r); }

}
