/*
 * Noise blanker, the steps of alt_noise_blanking (drivers/audio/audio_nr.c:2210-2535), for host and
 * device: an order-10 LPC analysis of the frame, the inverse filter and its matched filter, a
 * threshold on the result, and up to five repairs of seven samples each from the forward and the
 * backward prediction.  The kernel (uhsdr_nb.hip nb_frames) runs this text with a lane per channel
 * over a column of LDS, the host twin over a plain array: `ws` and `tp` are the distances in floats
 * between consecutive samples of the working buffer and of the filtered frame.
 *
 * Every sum is one binary32 accumulator with the products added in index order, as the CMSIS-DSP
 * functions of the reference form them (arm_dot_prod_f32, arm_fir_f32, arm_var_f32, arm_power_f32:
 * their unrolled loops keep the order), and the build has contraction off.  The C promotes to
 * double in three places; the casts below state them.
 *
 * Kept as the reference has them: nothing is clamped.  A silent frame has R[0] = 0, so k = 0 / 0 and
 * the threshold is a NaN; a frame whose autocorrelation overflows ends the same way.  Every
 * comparison with a NaN is false, so nothing is repaired and the samples pass.  The search does not
 * look at the filtered samples 0 .. 12; a hit at filtered sample n repairs the frame's samples
 * n - 13 .. n - 7 (the working buffer's n .. n + 6), and the search goes on at n + 4.  The repairs
 * run in the order found, after the search, and a later one reads what an earlier one wrote; the
 * search reads only the filtered frame, which no repair touches, so finding all places first and
 * repairing then, as here, is the same.
 *
 * The firmware's working_buffer is a static that nothing ever clears, not even a restart of the
 * noise reduction; here create and reset clear it (uhsdr.h says so beside the NR's overlap half).
 */
#ifndef UHSDR_NB_H
#define UHSDR_NB_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define NB_FN __host__ __device__ static inline
#define NB_UNROLL _Pragma("unroll")
#else
#define NB_FN static inline
#define NB_UNROLL
#endif

#define NB_FRAME 128                    /* NR_FFT_SIZE: samples per frame */
#define NB_ORDER 10                     /* order */
#define NB_PL 3                         /* PL */
#define NB_IMPULSE 7                    /* impulse_length */
#define NB_KEEP (2 * NB_ORDER + 2 * NB_PL)      /* floats of working_buffer kept from frame to frame */
#define NB_WB (NB_FRAME + NB_KEEP)      /* working_buffer */
#define NB_LEAD (NB_ORDER + NB_PL)      /* the analysed and returned frame is wb[13 .. 141) */
#define NB_MAX_HITS 5
#define NB_MAX_SETTING 15               /* MAX_NB_SETTING */

/* 8 values of n from n0 on for all 11 lags: R[i] += x[n] x[n + i] while n + i < 128 (:2380-2384).
   `guard`: the block reaches the frame's end (a constant at each call site). */
NB_FN void nb_autocorr_block(const float* wb, int ws, int n0, int guard, float* R)
{
    float x[8 + NB_ORDER];
    NB_UNROLL
    for (int q = 0; q < 8 + NB_ORDER; q++) x[q] = (!guard || n0 + q < NB_FRAME) ? wb[(NB_LEAD + n0 + q) * ws] : 0.0f;
    NB_UNROLL
    for (int q = 0; q < 8; q++)
    {
        NB_UNROLL
        for (int i = 0; i <= NB_ORDER; i++)
            if (!guard || n0 + q + i < NB_FRAME) R[i] += x[q] * x[q + i];
    }
}

NB_FN void nb_autocorr(const float* wb, int ws, float* R)
{
    NB_UNROLL
    for (int i = 0; i <= NB_ORDER; i++) R[i] = 0.0f;
    for (int n0 = 0; n0 < NB_FRAME - 16; n0 += 8) nb_autocorr_block(wb, ws, n0, 0, R);
    nb_autocorr_block(wb, ws, NB_FRAME - 16, 1, R);
    nb_autocorr_block(wb, ws, NB_FRAME - 8, 1, R);
}

/* Levinson-Durbin (:2391-2416); R[0] * (1.0 + 1.0e-9) is a double product rounded on assignment */
NB_FN void nb_levinson(float* R, float* lpcs)
{
    float any[NB_ORDER + 1];
    R[0] = (float)((double)R[0] * (1.0 + 1.0e-9));
    lpcs[0] = 1.0f;
    NB_UNROLL
    for (int i = 1; i <= NB_ORDER; i++) lpcs[i] = 0.0f;
    float alfa = R[0];
    NB_UNROLL
    for (int m = 1; m <= NB_ORDER; m++)
    {
        float s = 0.0f;
        NB_UNROLL
        for (int u = 1; u < m; u++) s = s + lpcs[u] * R[m - u];
        const float k = -(R[m] + s) / alfa;
        NB_UNROLL
        for (int v = 1; v < m; v++) any[v] = lpcs[v] + k * lpcs[m - v];
        NB_UNROLL
        for (int w = 1; w < m; w++) lpcs[w] = any[w];
        lpcs[m] = k;
        alfa = alfa * (1.0f - k * k);
    }
}

/* The two arm_fir_f32 passes (:2423-2430), each from a cleared state, and arm_var_f32 of the result
   (:2433).  Pass 1: t[n] = sum over i of x[n - 10 + i] * lpcs[10 - i], pass 2: y[n] = sum over i of
   t[n - 10 + i] * lpcs[i], oldest sample first, samples before the frame zero.  Eight outputs at a
   time with the ten samples before them carried in registers; pass 1's result is never stored.
   Returns sigma2 by the formula of this CMSIS version. */
NB_FN float nb_filter(const float* wb, int ws, const float* lpcs, float* ts, int tp)
{
    float h1[NB_ORDER], h2[NB_ORDER];
    float sum = 0.0f, sum_sq = 0.0f;
    NB_UNROLL
    for (int q = 0; q < NB_ORDER; q++) h1[q] = h2[q] = 0.0f;
    for (int n0 = 0; n0 < NB_FRAME; n0 += 8)
    {
        float x[8 + NB_ORDER], t[8 + NB_ORDER];
        NB_UNROLL
        for (int q = 0; q < NB_ORDER; q++)
        {
            x[q] = h1[q];
            t[q] = h2[q];
        }
        NB_UNROLL
        for (int q = 0; q < 8; q++) x[NB_ORDER + q] = wb[(NB_LEAD + n0 + q) * ws];
        NB_UNROLL
        for (int q = 0; q < 8; q++)
        {
            float acc = 0.0f;
            NB_UNROLL
            for (int i = 0; i <= NB_ORDER; i++) acc += x[q + i] * lpcs[NB_ORDER - i];
            t[NB_ORDER + q] = acc;
        }
        NB_UNROLL
        for (int q = 0; q < 8; q++)
        {
            float acc = 0.0f;
            NB_UNROLL
            for (int i = 0; i <= NB_ORDER; i++) acc += t[q + i] * lpcs[i];
            ts[(n0 + q) * tp] = acc;
            sum += acc;
            sum_sq += acc * acc;
        }
        NB_UNROLL
        for (int q = 0; q < NB_ORDER; q++)
        {
            h1[q] = x[8 + q];
            h2[q] = t[8 + q];
        }
    }
    const float mean_of_squares = sum_sq / ((float)NB_FRAME - 1.0f);
    const float mean = sum / (float)NB_FRAME;
    const float square_of_mean = (mean * mean) * ((float)NB_FRAME / ((float)NB_FRAME - 1.0f));
    return mean_of_squares - square_of_mean;
}

/* (float32_t)(16 - nb_setting) * 0.5 * sqrtf(sigma2 * lpc_power) (:2435-2438): arm_power_f32 over
   lpcs[0 .. 9], the product with 0.5 in double */
NB_FN float nb_threshold(const float* lpcs, float sigma2, int nb_setting)
{
    float lpc_power = 0.0f;
    NB_UNROLL
    for (int i = 0; i < NB_ORDER; i++) lpc_power += lpcs[i] * lpcs[i];
    return (float)((double)(float)(16 - nb_setting) * 0.5 * (double)sqrtf(sigma2 * lpc_power));
}

/* The search (:2443-2460).  The places found, impulse_positions[], are packed 7 bits each. */
NB_FN int nb_search(const float* ts, int tp, float threshold, uint64_t* places)
{
    int search_pos = NB_LEAD, count = 0;
    uint64_t packed = 0;
    do
    {
        const float v = ts[search_pos * tp];
        if (v > threshold || v < -threshold)
        {
            packed |= (uint64_t)(search_pos - NB_ORDER) << (7 * count);
            count++;
            search_pos += NB_PL;
        }
        search_pos++;
    } while (search_pos < NB_FRAME && count < NB_MAX_HITS);
    *places = packed;
    return count;
}

/* One repair (:2473-2523) at impulse position p: seven samples from wb[10 + p] on, each the forward
   prediction from the ten samples before weighted by Wfw plus the backward prediction from the ten
   samples behind weighted by Wbw; a prediction feeds the next one.  neg[i] = -lpcs[i]. */
NB_FN void nb_repair(float* wb, int ws, int p, const float* neg)
{
    float fw[NB_IMPULSE + NB_ORDER], bw[NB_IMPULSE + NB_ORDER];
    NB_UNROLL
    for (int k = 0; k < NB_ORDER; k++)
    {
        fw[k] = wb[(p + k) * ws];
        bw[NB_IMPULSE + k] = wb[(NB_LEAD + p + NB_PL + k + 1) * ws];
    }
    NB_UNROLL
    for (int i = 0; i < NB_IMPULSE; i++)
    {
        float f = 0.0f, b = 0.0f;
        NB_UNROLL
        for (int t = 0; t < NB_ORDER; t++) f += neg[NB_ORDER - t] * fw[i + t];
        NB_UNROLL
        for (int t = 0; t < NB_ORDER; t++) b += neg[1 + t] * bw[NB_IMPULSE - i + t];
        fw[NB_ORDER + i] = f;
        bw[NB_IMPULSE - i - 1] = b;
    }
    NB_UNROLL
    for (int i = 0; i < NB_IMPULSE; i++)
    {
        const float w_bw = (float)(1.0 * i / (NB_IMPULSE - 1)), w_fw = (float)(1.0 * (NB_IMPULSE - 1 - i) / (NB_IMPULSE - 1));
        wb[(NB_ORDER + p + i) * ws] = w_fw * fw[NB_ORDER + i] + w_bw * bw[i];
    }
}

/* One frame on a working buffer that already holds the new 128 samples behind the 26 kept ones.
   ts: 128 floats of scratch.  Returns the number of places repaired; the caller takes the frame
   from wb[13 .. 141) and moves the last 26 floats to the front. */
NB_FN int nb_frame(float* wb, int ws, float* ts, int tp, int nb_setting)
{
    float R[NB_ORDER + 1], lpcs[NB_ORDER + 1];
    nb_autocorr(wb, ws, R);
    nb_levinson(R, lpcs);
    const float sigma2 = nb_filter(wb, ws, lpcs, ts, tp);
    const float threshold = nb_threshold(lpcs, sigma2, nb_setting);
    uint64_t places;
    const int count = nb_search(ts, tp, threshold, &places);
    NB_UNROLL
    for (int i = 1; i <= NB_ORDER; i++) lpcs[i] = -lpcs[i];
    for (int j = 0; j < count; j++) nb_repair(wb, ws, (int)(places >> (7 * j)) & 127, lpcs);
    return count;
}

#endif /* UHSDR_NB_H */
