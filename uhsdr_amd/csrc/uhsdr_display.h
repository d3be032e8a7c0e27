/*
 * Display stage, the steps of one display frame for host and device: states 4 and 5 of
 * UiSpectrum_RedrawSpectrum (drivers/ui/lcd/ui_spectrum.c:1467-1517) up to the LCD calls, in the
 * firmware's order, once per completed frame:
 *   UiSpectrum_ScaleFFT (:1258-1292)                sd.FFT_AVGData to the row, with the frame's minimum
 *   UiSpectrum_ScaleFFT2SpectrumWidth (:1300-1339)  the row from L to W samples, if W != L
 *   sd.display_offset -= sd.agc_rate * min1 / 5     (:1485)
 *   the height of UiSpectrum_DrawScope (:881) and the byte line of UiSpectrum_DrawWaterfall
 *   (:1104, :1120-1128)
 *
 * A frame is sd.FFT_AVGData in natural bin order, L = fft_len floats, and `edge`, the float the
 * firmware finds at sd.FFT_Samples[L] (below).  What depends on the configuration alone
 * (uhsdr_display_plan, built by uhsdr_display_plan_build in uhsdr_setup.c) is computed once; the walk
 * of the width reduction is among it, since `amount` and idx_old never depend on the data.
 *
 * The parts, so that a wave can work a frame in parallel and the host in loops:
 *   display_scale    one bin of UiSpectrum_ScaleFFTValue before the minimum and the clamp
 *   display_pixel    one output sample of the width reduction from the scaled row
 *   display_height / display_colour   one column of the scope trace / of the waterfall line
 *   display_agc      the offset's update
 *   display_frame    the whole frame, one thread (the host twin)
 *   display_wave_frame  the same frame by one wave over rows in LDS (device only, below)
 * Every expression is binary32 as the C has it: the literals 1 and 5 are integers there, so no
 * expression widens to double except wfall_contrast, formed once in the plan.  The build has
 * contraction off.
 *
 * The width reduction works in place in the firmware: pixel p overwrites samples[p] after having read
 * samples[first[p]] .. samples[first[p] + whole[p]].  The plan builder has checked that no index is
 * read after it was written, so reading the unmodified scaled row gives the same values, and a
 * pixel depends on its predecessor only through for_next, which is (1 - amount[p-1]) times the
 * predecessor's split sample: recomputed here with the same two operations.
 *
 * Kept as the reference has them: min1 starts at 100000 and takes sig only on sig < min1, before the
 * clamp, so a NaN never wins and a frame of NaNs leaves 100000; sig < 1 ? 1 : sig passes a NaN; a NaN
 * height is the limit (the comparison fails); for the widths whose walk ends on samples[L] the last
 * pixel reads that float, `edge` here: in the firmware float L of arm_cfft_f32's output for the same
 * frame, the real part of bin L / 2 (nothing between the transform and state 4 writes past L - 1).
 * Defined here, not kept: the conversions to uint16_t and uint8_t of a NaN or a value outside the
 * target's range, which C leaves undefined (display_to_bits).
 */
#ifndef UHSDR_DISPLAY_H
#define UHSDR_DISPLAY_H

#include <math.h>
#include <stdint.h>

#include "uhsdr_internal.h"
#include "uhsdr_log10f_fast.h"

#ifdef __HIPCC__
#define DISPLAY_FN __host__ __device__ static inline
#else
#define DISPLAY_FN static inline
#endif

#define DISPLAY_OFFSET_INIT (-80.0f)    /* INIT_SPEC_AGC_LEVEL, ui_spectrum.h:160 */
#define DISPLAY_MIN_INIT 100000.0f      /* float32_t min1=100000, :1471 */
#define DISPLAY_COLOURS 64              /* NUMBER_WATERFALL_COLOURS */
#define DISPLAY_STATE_WORDS 2           /* per channel: display_offset, the last min1 */

/* the bin of sd.FFT_AVGData that scan step i of UiSpectrum_ScaleFFT reads (i + L/2, then i - L/2),
   and the row position L - 1 - i it writes */
DISPLAY_FN int display_src(int L, int i) { return (i + L / 2) & (L - 1); }
DISPLAY_FN int display_dst(int L, int i) { return L - 1 - i; }

/* :1260 */
DISPLAY_FN float display_scale(const uhsdr_display_plan* p, float offset, float v)
{
    return offset + log10f_fast(v) * p->db_scale;
}

/* :1268 */
DISPLAY_FN float display_clamp(float sig) { return (sig < 1) ? 1 : sig; }

/* x86's cvttss2si and the low bits of its result, as the recording has them: truncation for a value
   in (-2^31, 2^31), 0 for anything else, a NaN included */
DISPLAY_FN uint32_t display_to_bits(float v)
{
    return (v > -2147483648.0f && v < 2147483648.0f) ? (uint32_t)(int32_t)v : 0u;
}

/* :881 */
DISPLAY_FN uint16_t display_height(const uhsdr_display_plan* p, float v)
{
    const float limit = (float)p->limit;
    return (uint16_t)display_to_bits(v < limit ? v : limit);
}

/* arm_scale_f32 by sd.wfall_contrast (:1104), then :1122-1127 */
DISPLAY_FN uint8_t display_colour(const uhsdr_display_plan* p, float v)
{
    v = v * p->wfall_contrast;
    if (v >= DISPLAY_COLOURS) v = DISPLAY_COLOURS - 1;
    return (uint8_t)display_to_bits(v);
}

/* :1485 */
DISPLAY_FN float display_agc(const uhsdr_display_plan* p, float offset, float min1)
{
    return offset - p->agc_rate * min1 / 5;
}

/* output sample x of UiSpectrum_ScaleFFT2SpectrumWidth (:1316-1338) from the scaled row; sample L
   of the row is `edge` */
DISPLAY_FN float display_pixel(const uhsdr_display_plan* p, const float* row, float edge, int x)
{
    const int L = p->fft_len;
    float value = 0;
    if (x > 0)
    {
        const int s = p->first[x - 1] + p->whole[x - 1];
        value = (1 - p->amount[x - 1]) * (s < L ? row[s] : edge);      /* for_next of the pixel before */
    }
    int idx = p->first[x];
    for (int k = 0; k < p->whole[x]; k++) { value += (idx < L ? row[idx] : edge); idx++; }
    const float at = idx < L ? row[idx] : edge;
    const float for_next = (1 - p->amount[x]) * at;
    value += at - for_next;
    return value;
}

/* one frame, one thread; `row`: L floats of the caller's.  Returns min1; *offset is updated. */
DISPLAY_FN float display_frame(const uhsdr_display_plan* p, float* offset, const float* avg, float edge, float* row,
                               uint16_t* scope, uint8_t* wfall)
{
    const int L = p->fft_len, W = p->width;
    float min1 = DISPLAY_MIN_INIT;
    for (int i = 0; i < L; i++)
    {
        const float sig = display_scale(p, *offset, avg[display_src(L, i)]);
        if (sig < min1) min1 = sig;
        row[display_dst(L, i)] = display_clamp(sig);
    }
    *offset = display_agc(p, *offset, min1);
    for (int x = 0; x < W; x++)
    {
        const float v = p->resample ? display_pixel(p, row, edge, x) : row[x];
        if (scope) scope[x] = display_height(p, v);
        if (wfall) wfall[x] = display_colour(p, v);
    }
    return min1;
}

#ifdef __HIPCC__
/* What a kernel passes around: the plan and the state in device memory, the caller's rows. */
struct DisplayArgs
{
    const uhsdr_display_plan* plan;
    float* state;                       // [DISPLAY_STATE_WORDS][C], field-major: offset, min
    uhsdr_display_io io;                // null: not wanted
    int C, F;
};

/* One frame by one wave.  `avg`: the frame in LDS, natural bin order, complete before the call;
   `row`: L floats of LDS of the wave's own, not overlapping avg; every lane holds the same offset and
   edge and leaves with the same offset and min1.
   The minimum: the sequential scan leaves the smallest sig below 100000, and of several that compare
   equal (only +0 and -0 do without being the same bits) the one scanned first, since a later equal
   value fails the strict <.  Each lane scans its steps i = lane + 64 k in rising order with that same
   strict <, so it holds the first of its own smallest; the six exchanges then keep the smaller value
   and, of values that compare equal, the lower scan step: a total order on (value, step), so every
   lane ends with the pair the sequential scan ends with.  A NaN fails every comparison, so it never
   enters, in a lane or in an exchange; a lane that took nothing holds 100000 with a step behind all
   others, which loses against every taken value (all below 100000) and ties with nothing taken. */
__device__ __forceinline__ float display_wave_frame(const uhsdr_display_plan* __restrict__ p, float& offset, const float* avg,
                                                    float* row, float edge, size_t at, const uhsdr_display_io& io, int lane)
{
    const int L = p->fft_len, W = p->width;
    const int none = 0x7fffffff;
    float best = DISPLAY_MIN_INIT;
    int step = none;
    for (int i = lane; i < L; i += 64)
    {
        const float sig = display_scale(p, offset, avg[display_src(L, i)]);
        if (sig < best) { best = sig; step = i; }
        row[display_dst(L, i)] = display_clamp(sig);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        const float ov = __shfl_xor(best, d, 64);
        const int os = __shfl_xor(step, d, 64);
        if (ov < best || (ov == best && os < step)) { best = ov; step = os; }
    }
    offset = display_agc(p, offset, best);
    wave_sync();                                                    // the row is complete before its readers (uhsdr_dsp.h)
    uint16_t* __restrict__ scope = io.scope ? io.scope + at * W : nullptr;
    uint8_t* __restrict__ wfall = io.wfall ? io.wfall + at * W : nullptr;
    for (int x = lane; x < W; x += 64)
    {
        const float v = p->resample ? display_pixel(p, row, edge, x) : row[x];
        if (scope) scope[x] = display_height(p, v);
        if (wfall) wfall[x] = display_colour(p, v);
    }
    if (lane == 0)
    {
        if (io.offset) io.offset[at] = offset;
        if (io.min) io.min[at] = best;
    }
    return best;
}
#endif

#endif
