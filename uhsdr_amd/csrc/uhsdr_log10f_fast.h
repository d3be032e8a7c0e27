#ifndef UHSDR_LOG10F_FAST_H
#define UHSDR_LOG10F_FAST_H

#include <math.h>

/* Math_log10f_fast, misc/uhsdr_math.c:26-39: the AGC (uhsdr_rx.hip) and the signal meter
   (uhsdr_meter.h) share it.  frexpf and binary32 steps in the order of the C; the build has
   contraction off. */
#ifdef __HIPCC__
__host__ __device__ __forceinline__ float log10f_fast(float X)
#else
static inline __attribute__((always_inline)) float log10f_fast(float X)
#endif
{
    int E;
    const float F = frexpf(fabsf(X), &E);
    float Y = 1.23149591368684f;
    Y *= F;
    Y += -4.11852516267426f;
    Y *= F;
    Y += 6.02197014179219f;
    Y *= F;
    Y += -3.13396450166353f;
    Y += (float)E;
    return (Y * 0.3010299956639812f);
}

#endif
