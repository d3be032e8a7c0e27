/*
 * Spectral noise reduction, the per-bin steps of spectral_noise_reduction_3 (drivers/audio/
 * audio_nr.c:1841-2195), for host and device: the MMSE noise estimate, the Ephraim-Malah gain and
 * the width of the musical-noise smoothing.  The kernel (uhsdr_nr.hip nr_frames) runs them with a
 * lane per bin, the host twin (nr_frame_host, below) in the reference's loops.
 *
 * The C mixes float variables with double literals, so many expressions are evaluated in double and
 * rounded once on assignment.  Every cast below states where the C promotes and where it rounds; the
 * reference build is gcc -O2 without FMA and this code is built with contraction off.  fmin / fmax
 * are restated (nr_fmin / nr_fmax) so that host and device drop a NaN operand the same way.
 */
#ifndef UHSDR_NR_H
#define UHSDR_NR_H

#include <math.h>
#include <stdint.h>
#include "uhsdr_libm_expf.h"

#define NR_FN UHSDR_LIBM_FN

#define NR_FFT 256                      /* nr_params.NR_FFT_L */
#define NR_BINS 128                     /* NR_FFT_L / 2: bins, and samples per frame */

/* per-channel state: NR_F_COUNT rows of NR_BINS floats, then the words */
enum { NR_F_LAST_IN, NR_F_LAST_OUT, NR_F_HK, NR_F_HK_OLD, NR_F_XT, NR_F_PSLP, NR_F_NEST, NR_F_COUNT };
enum { NR_I_FIRST_TIME, NR_I_INIT_COUNTER, NR_I_NN, NR_I_POWER_RATIO, NR_I_COUNT };

/* the handle-wide values spectral_noise_reduction_3 derives at its entry (:1866-1890, :2034-2059) */
typedef struct
{
    float alpha, xih1r, pfac, power_threshold;
    int32_t width, lo, hi;              /* NR2.width, VAD_low, VAD_high after the clamps */
} NrParams;

typedef struct { float hk, hk_old, xt, pslp, nest; } NrBin;

/* glibc's fmin / fmax on doubles: the other operand when one is a NaN */
NR_FN double nr_fmin(double a, double b) { return a <= b ? a : (a > b ? b : (b != b ? a : b)); }
NR_FN double nr_fmax(double a, double b) { return a >= b ? a : (a < b ? b : (b != b ? a : b)); }

/* first_time == 1 (:1923-1933); last_sample_buffer_L is the caller's */
NR_FN void nr_bin_init(NrBin* b)
{
    b->hk = 1.0f;
    b->hk_old = 1.0f;
    b->nest = 0.0f;
    b->pslp = 0.5f;
}

/* first_time == 2, the 20-frame start-up average (:1993-1994) */
NR_FN void nr_bin_startup(NrBin* b, float X)
{
    b->nest = (float)((double)b->nest + 0.05 * (double)X);
    b->xt = 0.5f * b->nest;                                    /* psini */
}

/* speech-presence probability, noise estimate, SNR_post and SNR_prio of a bin (:2010-2031) */
NR_FN void nr_bin_estimate(NrBin* b, float X, const NrParams* p, float* snr_post, float* snr_prio)
{
    const float ax = 0.7405f, ap = 0.8691f, psthr = 0.99f, pnsaf = 0.01f, snr_prio_min = 0.001f;
    float ph1y = (float)(1.0 / (1.0 + (double)(p->pfac * ul_expf(p->xih1r * X / b->xt))));
    b->pslp = (float)((double)(ap * b->pslp) + (1.0 - (double)ap) * (double)ph1y);
    if (b->pslp > psthr) ph1y = (float)(1.0 - (double)pnsaf);
    else ph1y = (float)nr_fmin((double)ph1y, 1.0);
    const float xtr = (float)((1.0 - (double)ph1y) * (double)X + (double)(ph1y * b->xt));
    b->xt = (float)((double)(ax * b->xt) + (1.0 - (double)ax) * (double)xtr);
    const float post = (float)nr_fmax(nr_fmin((double)(X / b->xt), 1000.0), (double)snr_prio_min);
    *snr_post = post;
    *snr_prio = (float)nr_fmax((double)(p->alpha * b->hk_old) + (1.0 - (double)p->alpha) * nr_fmax((double)post - 1.0, 0.0), 0.0);
}

/* Hk and Hk_old of a bin inside the band (:2067-2071) */
NR_FN void nr_bin_gain(NrBin* b, float snr_post, float snr_prio)
{
    const float v = (float)((double)(snr_prio * snr_post) / (1.0 + (double)snr_prio));
    const float root = sqrtf((float)(0.7212 * (double)v + (double)(v * v)));
    b->hk = (float)nr_fmax(1.0 / (double)snr_post * (double)root, 0.001);
    b->hk_old = snr_post * b->hk * b->hk;
}

/* NN from the band's power before and after the gains (:2088-2097).  The C converts a NaN ratio
   (a band without power: 0 / 0) to int, which is undefined; here that frame has NN = 1 and the
   ratio stays NaN. */
NR_FN int nr_smoothing_width(float* power_ratio, float pre_power, float post_power, const NrParams* p)
{
    *power_ratio = post_power / pre_power;
    if (*power_ratio > p->power_threshold)
    {
        *power_ratio = 1.0f;
        return 1;
    }
    if (*power_ratio != *power_ratio) return 1;
    return 1 + 2 * (int)(0.5 + (double)p->width * (1.0 - (double)(*power_ratio / p->power_threshold)));
}

/* The largest NN a width allows: power_ratio >= 0, so the factor of width is at most 1. */
static inline int nr_nn_max(int width) { return 1 + 2 * width; }

/* The smoothing loops (:2099-2137) index Hk and Nest relative to the band.  With NN up to M and a
   band that is not empty, the lower-edge loop reads up to Hk[lo + M/2 + M - 2], the upper-edge loop
   writes Nest[hi - M] and reads down to Hk[hi - 2M + 1]; the middle loop stays inside the band.  An
   empty band (lo >= hi) has no power, so NN = 1 and only Hk[hi - 1] is touched.  Nothing leaves
   0 .. 127 exactly when this holds. */
static inline int nr_band_in_bounds(int lo, int hi, int width)
{
    const int M = nr_nn_max(width);
    if (lo >= hi) return hi >= 1;
    return hi >= 2 * M - 1 && lo + M / 2 + M - 2 <= NR_BINS - 1;
}

/* ---- the 12 ksps stream around the frames (AudioDriver_RxProcessorNoiseReduction,
 *      audio_driver.c:2328-2434) as functions of an element index, for the kernels and the host twin.
 * All channels advance together, so the positions are the handle's: `fill` samples of the frame being
 * collected, P0 results produced and E0 emitted before the call; a channel's queue holds the results
 * E0 .. P0 - 1, at most two frames. ---- */
#define NR_DEC_TAPS 4
#define NR_INT_TAPS 40
#define NR_INT_PHASE 20                 /* arm_fir_interpolate_init_f32: numTaps / L */
#define NR_LATENCY (2 * NR_BINS)        /* the output FIFO hands out a frame once two exist */
#define NR_QUEUE (2 * NR_BINS)

/* arm_fir_decimate_f32, 4 taps, M = 2: output j of this call, from the call's input row and the
   three samples before it */
NR_FN float nr_stream_decimate(const float* in, const float* hist, int j, const float* c)
{
    float acc = 0.0f;
    for (int k = 0; k < NR_DEC_TAPS; k++)
    {
        const int s = 2 * j - (NR_DEC_TAPS - 1) + k;
        acc += (s >= 0 ? in[s] : hist[NR_DEC_TAPS - 1 + s]) * c[k];
    }
    return acc;
}

/* sample i of the work row: the frame being collected, then the call's samples at the frames' rate */
NR_FN float nr_stream_work(const float* in, const float* pend, const float* dec_hist, const float* dc, int decimated, int fill, int i)
{
    if (i < fill) return pend[i];
    return decimated ? nr_stream_decimate(in, dec_hist, i - fill, dc) : in[i - fill];
}

/* result `idx` of the frame stage: still queued from earlier calls, or of this call's frames */
NR_FN float nr_stream_result(const float* queue, const float* y, int64_t idx, int64_t E0, int64_t P0)
{
    return idx < P0 ? queue[idx - E0] : y[idx - P0];
}

/* what the FIFO hands out for sample i of this call, T0 samples after the reset */
NR_FN float nr_stream_emit(const float* queue, const float* y, int64_t T0, int64_t E0, int64_t P0, int i)
{
    const int64_t j = T0 + i;
    return j < NR_LATENCY ? 0.0f : nr_stream_result(queue, y, j - NR_LATENCY, E0, P0);
}

/* arm_fir_interpolate_f32 (40 taps, L = 2) and arm_scale_f32 by 2.0: output o of this call from the
   emitted row z and the 19 samples before it */
NR_FN float nr_stream_interpolate(const float* z, const float* hist, int o, const float* c)
{
    const int i = o >> 1, first = (o & 1) ? 0 : 1;       /* ptr2 = pCoeffs + (L - j), j = 1, 2 */
    float acc = 0.0f;
    for (int t = 0; t < NR_INT_PHASE; t++)
    {
        const int s = i - (NR_INT_PHASE - 1) + t;
        acc += (s >= 0 ? z[s] : hist[NR_INT_PHASE - 1 + s]) * c[first + 2 * t];
    }
    return acc * 2.0f;
}

#endif /* UHSDR_NR_H */
