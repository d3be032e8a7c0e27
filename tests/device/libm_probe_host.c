/* Host side of the libm probe (tests/test_gpu_libm.py, tests/test_libm.py): the entry points of
 * libm_probe.hip as loops over arrays, built by the Makefile with exactly $(HOSTCFLAGS) into
 * tests/build/libuhsdr_libm_probe_host.so.
 *   ulh_*  the host build of uhsdr_amd/csrc/uhsdr_libm.h (and the plain C expression for the
 *          primitives and the mixed-precision recursions)
 *   ulg_*  glibc itself: sincosf, atan2f, atanf, asinf, sqrtf called in libm, and '/'
 * plus ul_gen_atan2_pairs, the operand generator of tools/libm_check.c's "atan2" mode with its
 * seed, so the host pin and the device pin see the same pairs.  The loops are in C because a
 * ctypes call per operand is far too slow for tens of millions of operands. */
#define _GNU_SOURCE
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../uhsdr_amd/csrc/uhsdr_libm.h"

/* libm's entry points through volatile pointers: gcc then neither inlines sqrtss nor folds a call */
static void (*volatile g_sincosf)(float, float*, float*) = sincosf;
static float (*volatile g_atan2f)(float, float) = atan2f;
static float (*volatile g_atanf)(float) = atanf;
static float (*volatile g_asinf)(float) = asinf;
static float (*volatile g_sqrtf)(float) = sqrtf;

void ulh_sincosf(const float* y, float* s, float* c, size_t n) { for (size_t i = 0; i < n; ++i) ul_sincosf(y[i], &s[i], &c[i]); }
void ulg_sincosf(const float* y, float* s, float* c, size_t n) { for (size_t i = 0; i < n; ++i) g_sincosf(y[i], &s[i], &c[i]); }

void ulh_atan2f(const float* y, const float* x, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = ul_atan2f(y[i], x[i]); }
void ulg_atan2f(const float* y, const float* x, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = g_atan2f(y[i], x[i]); }

void ulh_atanf_pos(const float* a, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = ul_atanf_pos(a[i]); }
void ulg_atanf_pos(const float* a, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = g_atanf(a[i]); }

void ulh_asinf(const float* a, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = ul_asinf(a[i]); }
void ulg_asinf(const float* a, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = g_asinf(a[i]); }

void ulh_sqrtf(const float* a, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = sqrtf(a[i]); }
void ulg_sqrtf(const float* a, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = g_sqrtf(a[i]); }

void ulh_divf(const float* a, const float* b, float* r, size_t n) { for (size_t i = 0; i < n; ++i) r[i] = a[i] / b[i]; }
void ulg_divf(const float* a, const float* b, float* r, size_t n) { ulh_divf(a, b, r, n); }

/* uhsdr_spectrum.hip:125-127 */
void ulh_iq_lowpass(const float* t, const float* o, float* rneg, float* rpos, size_t n)
{
    for (size_t i = 0; i < n; ++i)
    {
        rneg[i] = (float)(-0.003 * (double)(t[i] / 32.0f) + 0.997 * (double)o[i]);
        rpos[i] = (float)(0.003 * (double)(t[i] / 32.0f) + 0.997 * (double)o[i]);
    }
}
void ulg_iq_lowpass(const float* t, const float* o, float* rneg, float* rpos, size_t n) { ulh_iq_lowpass(t, o, rneg, rpos, n); }

/* uhsdr_rx.hip:3184 */
void ulh_squelch_avg(const float* t, const float* o, float* r, size_t n)
{
    for (size_t i = 0; i < n; ++i) r[i] = (float)(((1 - 0.005) * (double)o[i]) + (0.005 * (double)sqrtf(fabsf(t[i]))));
}
void ulg_squelch_avg(const float* t, const float* o, float* r, size_t n)
{
    for (size_t i = 0; i < n; ++i) r[i] = (float)(((1 - 0.005) * (double)o[i]) + (0.005 * (double)g_sqrtf(fabsf(t[i]))));
}

/* tools/libm_check.c "atan2": the pairs i = 400 .. 400 + count - 1 that follow its 20 x 20 special
 * grid -- any bits when i % 3 == 0, else FM-like products of audio-range samples of similar
 * magnitude -- from the same xorshift64 state */
void ul_gen_atan2_pairs(size_t count, float* y, float* x)
{
    uint64_t rng = 0x9E3779B97F4A7C15ull;
#define NEXT32() (rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17, (uint32_t)(rng >> 16))
    const size_t grid = 20 * 20;
    for (size_t k = 0; k < count; ++k)
    {
        const size_t i = grid + k;
        if (i % 3 == 0)
        {
            y[k] = ul_asfloat(NEXT32());
            x[k] = ul_asfloat(NEXT32());
        }
        else
        {
            const float a = (float)((int32_t)NEXT32()) * 0x1p-31f;
            const float b = (float)((int32_t)NEXT32()) * 0x1p-31f;
            const int e = (int)(NEXT32() % 40) - 20;
            y[k] = ldexpf(a, e);
            x[k] = ldexpf(b, e + (int)(NEXT32() % 9) - 4);
        }
    }
#undef NEXT32
}
