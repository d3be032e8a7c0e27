/*
 * Signal meter, the steps of one display frame for host and device: UiSpectrum_CalculateDBm with
 * UiSpectrum_CalculateSnap (drivers/ui/lcd/ui_spectrum.c:1876-2123), the two averagers of
 * RadioManagement_HandleIqGainAndSMeter and the S-unit search of UiDriver_HandleSMeter
 * (drivers/ui/ui_driver.c:4629-4696), in that order, once per completed frame.
 *
 * A frame is sd.FFT_MagData in natural bin order, L = fft_len floats.  The firmware first copies it
 * reversed, with the halves exchanged and times SCOPE_PREAMP_GAIN, into sd.FFT_Samples (:2084-2091);
 * here meter_sample() is that copy as an index map.  What depends on the configuration alone
 * (uhsdr_meter_plan, built by uhsdr_meter_plan_build in uhsdr_setup.c) is computed once.
 *
 * The parts, so that a wave can search the maximum in parallel and the host in a loop:
 *   meter_snap    from maxbin and the three samples around it to snap_carrier_freq and freq_old
 *   meter_level   from the passband's sum to dbm_cur, dbmhz_cur, dbm, dbmhz and s_count
 *   meter_frame   the whole frame in the firmware's own order, one thread (the host twin)
 *   meter_wave_frame  the same frame by one wave over a row in LDS (device only, below): the
 *                 search as a wave reduction, everything else as in meter_frame
 * The sum is one binary32 accumulator from Lbin up to Ubin, as the C has it; it is no tree.  float
 * and double stand where the C has them: a literal like 1.0 or 0.2 makes its expression a double one,
 * and the casts below state every such place.  The build has contraction off.
 *
 * Kept as the reference has them: the search starts from maximum = 0 and maxbin = 1, so a passband
 * without a sample above zero "finds" bin 1, and a NaN never wins (every comparison with it is
 * false); the sum and the interpolation take NaN and infinities as they come; with Lbin == Ubin the
 * dBm/Hz term is 10 log10 of 0, which Math_log10f_fast gives as a finite number (the clamp of Lbin at
 * 0 makes such a passband: tests/golden/meter_cw_onebin.npz); dbm above the table's last entry is
 * S-count 33.
 * Defined here, not kept:
 *  - with maxbin == L - 1 the C reads sd.FFT_Samples[L], a leftover of the transform's complex
 *    output; here bin3 is 0 in that case (DESIGN.md 7 has the CW decoder's read of the same kind);
 *  - snap_carrier_freq is (ulong)help_freq, which C leaves undefined for a NaN, a negative value or
 *    one of 2^32 and above; here those give 0.
 */
#ifndef UHSDR_METER_H
#define UHSDR_METER_H

#include <math.h>
#include <stdint.h>

#include "uhsdr_internal.h"
#include "uhsdr_log10f_fast.h"

#ifdef __HIPCC__
#define METER_FN __host__ __device__ static inline
#else
#define METER_FN static inline
#endif

#define METER_PREAMP 1000               /* SCOPE_PREAMP_GAIN, ui_spectrum.h:158 */
#define METER_FREQ_OLD_INIT 10000000.0f /* static float32_t freq_old = 10000000.0, :1891 */
#define METER_S_SIZE 33                 /* S_Meter_Cal_Size */
#define METER_SNAP_NEVER 0
#define METER_SNAP_ALWAYS 1             /* AM, SAM, DIGI with BPSK */
#define METER_SNAP_CW 2                 /* CW: the frames whose cw_signal is set */

/* a channel's state between frames: the four averages, freq_old, and the outputs as last written */
typedef struct
{
    float attack_dbm, decay_dbm, attack_dbmhz, decay_dbmhz, freq_old;
    float dbm_cur, dbmhz_cur, dbm, dbmhz;
    int32_t s_count;
    uint32_t snap;
} meter_state;
#define METER_STATE_WORDS 11

METER_FN void meter_state_reset(meter_state* s)
{
    s->attack_dbm = s->decay_dbm = s->attack_dbmhz = s->decay_dbmhz = 0.0f;
    s->freq_old = METER_FREQ_OLD_INIT;
    s->dbm_cur = s->dbmhz_cur = s->dbm = s->dbmhz = 0.0f;
    s->s_count = 0;
    s->snap = 0;
}

/* sd.FFT_Samples[j] of the frame `mag` (:2084-2091): j = L - 1 - i takes bin i + L/2 for i < L/2 and
   bin i - L/2 above */
METER_FN int meter_bin(int L, int j) { return (L - 1 - j + L / 2) & (L - 1); }
METER_FN float meter_sample(const float* mag, int L, int j) { return mag[meter_bin(L, j)] * METER_PREAMP; }

/* :1914-1963 from the search's result on; `found`: a sample above zero was seen, else maxbin is the
   initial 1 */
METER_FN void meter_snap(const uhsdr_meter_plan* p, meter_state* s, const float* mag, int found, int maxindex)
{
    const int L = p->fft_len;
    float maxbin = found ? (float)maxindex : 1.0f;
    const float delta1 = (float)((((double)maxbin + 1.0) - (double)(float)p->posbin) * (double)p->bin_bw);
    if (maxbin < 1.0) maxbin = 1.0f;
    const int m = (int)maxbin;
    float bin1 = meter_sample(mag, L, m - 1);
    const float bin2 = meter_sample(mag, L, m);
    const float bin3 = m + 1 < L ? meter_sample(mag, L, m + 1) : 0.0f;
    if (bin1 + bin2 + bin3 == 0.0) bin1 = (float)0.00000001;
    float delta2 = (float)(((double)p->bin_bw * (1.36 * (double)(bin3 - bin1))) / (double)(bin1 + bin2 + bin3));
    if (delta2 > p->bin_bw) delta2 = 0.0f;
    float delta = delta1 + delta2;
    if (p->snap_offset != 0.0f) delta = delta + p->snap_offset;     /* the CW or the BPSK offset (:1939-1955) */
    float help_freq = (float)p->tune_old;
    help_freq = help_freq + delta;
    help_freq = (float)(0.2 * (double)help_freq + 0.8 * (double)s->freq_old);
    s->snap = (help_freq >= 0.0f && help_freq < 4294967296.0f) ? (uint32_t)help_freq : 0u;
    s->freq_old = help_freq;
}

/* :2112-2121, ui_driver.c:4642-4669 and :4688-4696 */
METER_FN void meter_level(const uhsdr_meter_plan* p, meter_state* s, float sum_db)
{
    const float slope = 19.8f;
    if (sum_db > 0)
    {
        s->dbm_cur = slope * log10f_fast(sum_db) + p->cons;
        s->dbmhz_cur = s->dbm_cur - p->dbmhz_term;
    }
    else
    {
        s->dbm_cur = -145.0f;
        s->dbmhz_cur = -145.0f;
    }
    const float aa = p->attack_alpha, da = p->decay_alpha;
    s->attack_dbm = (float)((1.0 - (double)aa) * (double)s->attack_dbm + (double)(aa * s->dbm_cur));
    s->decay_dbm = (float)((1.0 - (double)da) * (double)s->decay_dbm + (double)(da * s->dbm_cur));
    s->attack_dbmhz = (float)((1.0 - (double)aa) * (double)s->attack_dbmhz + (double)(aa * s->dbmhz_cur));
    s->decay_dbmhz = (float)((1.0 - (double)da) * (double)s->decay_dbmhz + (double)(da * s->dbmhz_cur));
    if (s->attack_dbm > s->decay_dbm)
    {
        s->dbm = s->attack_dbm;
        s->decay_dbm = s->attack_dbm;
    }
    else s->dbm = s->decay_dbm;
    if (s->attack_dbmhz > s->decay_dbmhz)
    {
        s->dbmhz = s->attack_dbmhz;
        s->decay_dbmhz = s->attack_dbmhz;
    }
    else s->dbmhz = s->decay_dbmhz;
    int32_t n = 1;
    while (n < METER_S_SIZE && s->dbm >= p->s_cal_dbm[n]) n++;
    s->s_count = n;
}

/* whether SNAP runs on a frame whose ads.CW_signal is `cw_signal` (:2094 and :1886) */
METER_FN int meter_snap_runs(const uhsdr_meter_plan* p, int cw_signal)
{
    return p->snap == METER_SNAP_ALWAYS || (p->snap == METER_SNAP_CW && cw_signal);
}

/* one frame, one thread */
METER_FN void meter_frame(const uhsdr_meter_plan* p, meter_state* s, const float* mag, int cw_signal)
{
    const int L = p->fft_len;
    if (meter_snap_runs(p, cw_signal))
    {
        float maximum = 0.0f;
        int found = 0, maxindex = 0;
        for (int c = p->lbin; c <= p->ubin; c++)
        {
            const float v = meter_sample(mag, L, c);
            if (maximum < v) { maximum = v; maxindex = c; found = 1; }
        }
        meter_snap(p, s, mag, found, maxindex);
    }
    float sum_db = 0.0f;
    for (int c = p->lbin; c <= p->ubin; c++) sum_db = sum_db + meter_sample(mag, L, c);
    meter_level(p, s, sum_db);
}

#ifdef __HIPCC__
/* What a kernel passes around: the plan and the state in device memory, the caller's rows. */
struct MeterArgs
{
    const uhsdr_meter_plan* plan;
    uint32_t* state;                    // [METER_STATE_WORDS][C], field-major
    uhsdr_meter_io io;                  // rows [C][F], null: not wanted
    int C, F;
};

// the state's words in the order of meter_state, each field by itself: an array copied into the structure
// would be a private array to the compiler, which it places in LDS or scratch
__device__ __forceinline__ void meter_state_load(meter_state& s, const uint32_t* st, int C, int c)
{
    const uint32_t* p = st + c;
    const size_t n = (size_t)C;
    s.attack_dbm = __uint_as_float(p[0 * n]); s.decay_dbm = __uint_as_float(p[1 * n]);
    s.attack_dbmhz = __uint_as_float(p[2 * n]); s.decay_dbmhz = __uint_as_float(p[3 * n]);
    s.freq_old = __uint_as_float(p[4 * n]);
    s.dbm_cur = __uint_as_float(p[5 * n]); s.dbmhz_cur = __uint_as_float(p[6 * n]);
    s.dbm = __uint_as_float(p[7 * n]); s.dbmhz = __uint_as_float(p[8 * n]);
    s.s_count = (int32_t)p[9 * n]; s.snap = p[10 * n];
}

__device__ __forceinline__ void meter_state_store(const meter_state& s, uint32_t* st, int C, int c)
{
    uint32_t* p = st + c;
    const size_t n = (size_t)C;
    p[0 * n] = __float_as_uint(s.attack_dbm); p[1 * n] = __float_as_uint(s.decay_dbm);
    p[2 * n] = __float_as_uint(s.attack_dbmhz); p[3 * n] = __float_as_uint(s.decay_dbmhz);
    p[4 * n] = __float_as_uint(s.freq_old);
    p[5 * n] = __float_as_uint(s.dbm_cur); p[6 * n] = __float_as_uint(s.dbmhz_cur);
    p[7 * n] = __float_as_uint(s.dbm); p[8 * n] = __float_as_uint(s.dbmhz);
    p[9 * n] = (uint32_t)s.s_count; p[10 * n] = s.snap;
}

/* One frame by one wave.  `row`: the frame in LDS, natural bin order, complete before the call; every
   lane holds the same state and leaves with the same state.  The search: each lane takes the samples
   lbin + lane + 64 k in rising order with the C's strict <, then six exchanges keep the larger value
   and, of equal values, the lower index: the first maximum of the serial loop.  A NaN never compares
   above anything, so it never enters.  The sum is the serial loop itself, run by all lanes alike (the
   same LDS word in every lane is one broadcast read): its order is the C's. */
__device__ __forceinline__ void meter_wave_frame(const uhsdr_meter_plan* __restrict__ p, meter_state& s, const float* row,
                                                 int cw_signal, int lane)
{
    const int L = p->fft_len, lbin = p->lbin, ubin = p->ubin;
    if (meter_snap_runs(p, cw_signal))
    {
        const int none = 0x7fffffff;
        float best = 0.0f;
        int at = none;
        for (int c = lbin + lane; c <= ubin; c += 64)
        {
            const float v = meter_sample(row, L, c);
            if (best < v) { best = v; at = c; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
        {
            const float ov = __shfl_xor(best, d, 64);
            const int oa = __shfl_xor(at, d, 64);
            if (best < ov || (best == ov && oa < at)) { best = ov; at = oa; }
        }
        meter_snap(p, &s, row, at != none, at);
    }
    float sum_db = 0.0f;
#pragma unroll 8
    for (int c = lbin; c <= ubin; c++) sum_db = sum_db + meter_sample(row, L, c);
    meter_level(p, &s, sum_db);
}

/* lane 0 of the wave writes the frame's outputs: element `at` = c * F + frame of every row wanted */
__device__ __forceinline__ void meter_write(const uhsdr_meter_io& io, const meter_state& s, size_t at)
{
    if (io.dbm_cur) io.dbm_cur[at] = s.dbm_cur;
    if (io.dbmhz_cur) io.dbmhz_cur[at] = s.dbmhz_cur;
    if (io.dbm) io.dbm[at] = s.dbm;
    if (io.dbmhz) io.dbmhz[at] = s.dbmhz;
    if (io.s_count) io.s_count[at] = s.s_count;
    if (io.snap_carrier_freq) io.snap_carrier_freq[at] = s.snap;
}
#endif

#endif
