/*
 * glibc-exact expf for host and device, in the style of uhsdr_libm.h (whose helpers it uses).
 * Pinned against the host's libm on all 2^32 operands (tools/libm_check.c "expf 1",
 * tests/golden/expf_pin.txt), on a subset by tests/test_expf.py, and the device build against the
 * host build on the MI355X by tests/test_gpu_expf.py (tests/device/expf_probe.hip).
 */
#ifndef UHSDR_LIBM_EXPF_H
#define UHSDR_LIBM_EXPF_H

#include "uhsdr_libm.h"

/* ---- expf (glibc sysdeps/ieee754/flt-32/e_expf.c + math_config.h exp2f_data, Szabolcs Nagy, ARM
 *      optimized-routines, 2017; the spectral noise reduction's speech-presence probability,
 *      audio_nr.c:2010) ----
 * exp(x) = 2^(k/32) * 2^(r/32) with k = round(x * 32/ln2) through the 0x1.8p52 shift and a cubic
 * in r, all in double, rounded once to binary32.  The x86-64 build dispatches (IFUNC) to the -mfma
 * variant, where gcc fused five of the operations: x * InvLn2N + SHIFT, x * InvLn2N - kd and the
 * three polynomial steps.  They are explicit fma() calls here.  tab[i] is the bit pattern of
 * 2^(i/32) minus i << 47, so that adding k << 47 puts k / 32 into the exponent.
 * A header of its own beside uhsdr_libm.h: a __constant__ table is emitted into every device code
 * object that sees it, used or not, and 256 more bytes of read-only data move the code of the
 * receive kernels, which include uhsdr_libm.h. */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline const uint64_t* ul_exp2f_table(void)
{
#ifdef __HIPCC__
    static __constant__ const uint64_t t[32] = {
#else
    static const uint64_t t[32] = {
#endif
        0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51,
        0x3fef72b83c7d517b, 0x3fef54873168b9aa, 0x3fef387a6e756238, 0x3fef1e9df51fdee1,
        0x3fef06fe0a31b715, 0x3feef1a7373aa9cb, 0x3feedea64c123422, 0x3feece086061892d,
        0x3feebfdad5362a27, 0x3feeb42b569d4f82, 0x3feeab07dd485429, 0x3feea47eb03a5585,
        0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13,
        0x3feeace5422aa0db, 0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d,
        0x3feee89f995ad3ad, 0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069,
        0x3fef5818dcfba487, 0x3fef7c97337b9b5f, 0x3fefa4afa2a490da, 0x3fefd0765b6e4540,
    };
    return t;
}

UHSDR_LIBM_FN float ul_expf(float x)
{
    const double InvLn2N = 0x1.71547652b82fep+5, SHIFT = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-20, C1 = 0x1.ebfce50fac4f3p-13, C2 = 0x1.62e42ff0c52d6p-6;
    const double xd = (double)x;
    const uint32_t abstop = (ul_asuint(x) >> 20) & 0x7ff;
    if (abstop >= 0x42b)                                          /* |x| >= 88 or NaN */
    {
        if (ul_asuint(x) == 0xff800000u) return 0.0f;             /* -inf */
        if (abstop >= 0x7f8) return x + x;                        /* +inf, NaN */
        if (x > 0x1.62e42ep6f) return INFINITY;                   /* __math_oflowf: 2^97 * 2^97 */
        if (x < -0x1.9fe368p6f) return 0.0f;                      /* __math_uflowf: 2^-95 * 2^-95 */
        if (x < -0x1.9d1d9ep6f) return 0x1p-149f;                 /* __math_may_uflowf: 1.25 2^-75 squared */
    }
    double kd = fma(InvLn2N, xd, SHIFT);
    const uint64_t ki = ul_asuint64(kd);
    kd -= SHIFT;
    const double r = fma(InvLn2N, xd, -kd);
    const double s = ul_asdouble(ul_exp2f_table()[ki & 31] + (ki << 47));
    const double z = fma(C0, r, C1);
    const double r2 = r * r;
    double y = fma(C2, r, 1.0);
    y = fma(z, r2, y);
    return (float)(y * s);
}

#endif /* UHSDR_LIBM_EXPF_H */
