/*
 * RTTY decoder: one channel's demodulator and Baudot framer, advanced by one 12 ksps sample.
 *
 * Restates what the firmware runs per decimated sample in DEMOD_DIGI with digital_mode RTTY
 * (audio_driver.c:2537-2557 -> Rtty_Demodulator_ProcessSample, drivers/audio/rtty.c:634-711, with
 * the two 4th-order band-passes and the low-pass :238-255, decayavg :450-462, the demodulator with
 * and without automatic threshold correction :466-555, the bit DPLL :558-591, the start-bit search
 * :594-631 and the letters / figures tables :27-39).  The input of a step is a_buffer[0] after
 * biquad_1, the sample the firmware hands its modems.
 *
 * The same function runs on the host (uhsdr_rtty_process_host) and in the rtty_decode kernel: both
 * address one field-major arena, so a channel's state is a column of it.
 *
 * Arithmetic follows the reference's C exactly as gcc -O2 evaluates it with SSE and no
 * contraction: sums left to right with separate multiplies and adds, every division a correctly
 * rounded binary32 division, the decay weights integer expressions of oneBitSampleCount, and the
 * optimal-ATC expression's last subtraction in binary64 (its 0.25 is a double literal) rounded
 * once on the store to float.  The build has -ffp-contract=off.
 *
 * Every function-local static of the reference (the four ATC trackers, phaseChanged, the
 * start-bit search's state and half-bit counter) is per-channel state here and starts at zero.
 * phaseChanged is never cleared there, so the DPLL corrects its phase once per decoder lifetime;
 * DPLLBitPhase is not reset at a start bit.  Both are kept.
 *
 * The demodulator runs on every sample: in the bit state byteResultp stays below 8 and
 * DPLLBitPhase below oneBitSampleCount between samples (the phase grows by at most 1 + count / 32
 * from below count and is then reduced by count), so the two guards of rtty.c:563 and :649 always
 * hold and the filters advance once per sample in either state.  The step below therefore filters
 * first and runs the state machine on the bit.
 */
#ifndef UHSDR_RTTY_H
#define UHSDR_RTTY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RTTY_HD __host__ __device__ inline
#else
#define RTTY_HD inline
#endif

#define RTTY_SHIFT_COUNT 6
#define RTTY_SPEED_COUNT 2
#define RTTY_STOP_COUNT  3
#define RTTY_STOP_2      2       /* stopbits index of two stop bits */
#define RTTY_CODE_FIGS   0x1bu
#define RTTY_CODE_LTRS   0x1fu

/* float state of a channel, rows of RttyArena::fs: the last four inputs and outputs of each
   band-pass, the last two of the low-pass, the ATC envelope and noise trackers */
enum
{
    RTTY_F_SX = 0, RTTY_F_SY = 4, RTTY_F_MX = 8, RTTY_F_MY = 12, RTTY_F_LX = 16, RTTY_F_LY = 18,
    RTTY_F_MARK_ENV = 20, RTTY_F_SPACE_ENV, RTTY_F_MARK_NOISE, RTTY_F_SPACE_NOISE, RTTY_F_COUNT
};
/* integer state, rows of RttyArena::is */
enum
{
    RTTY_I_RUN = 0,      /* 0 waiting for a start bit, 1 reading bits */
    RTTY_I_WFS,          /* wait_for_start_state 0 .. 3 */
    RTTY_I_HALF,         /* wait_for_half */
    RTTY_I_OLDVAL,       /* DPLLOldVal */
    RTTY_I_PHASE,        /* DPLLBitPhase */
    RTTY_I_BYTE,         /* byteResult */
    RTTY_I_BYTEP,        /* byteResultp */
    RTTY_I_FLAGS,        /* bit 0 figures table selected, bit 1 phaseChanged */
    RTTY_I_COUNT
};
enum { RTTY_FLAG_FIGS = 1, RTTY_FLAG_PHASED = 2 };

/* All channels' state, field-major. */
struct RttyArena
{
    int32_t C;
    int32_t text_capacity;
    float* fs;           /* [RTTY_F_COUNT][C] */
    int32_t* is;         /* [RTTY_I_COUNT][C] */
    uint32_t* total;     /* [C] */
    uint8_t* text;       /* [C][text_capacity], character k at k % text_capacity */
};

/* One band-pass or the low-pass: the gain the input is divided by and the feedback coefficients */
struct RttyBpf { float gain, c0, c1, c2, c3; };
struct RttyLpf { float gain, c0, c1; };

/* The launch constants of a decoder (Rtty_Modem_Init) */
struct RttyParams
{
    RttyBpf space, mark;
    RttyLpf lp;
    int32_t one_bit;         /* oneBitSampleCount */
    int32_t stopbits;        /* 0, 1, 2: 1, 1.5 and 2 stop bits */
    int32_t atc_disable;
};

/* 12 ksps, order-2 Butterworth band-passes 100 Hz wide (50 Hz for the 85 Hz shift) at the mark
   frequency 915 Hz and at 915 Hz + shift, and the 50 Hz low-pass: the reference's float32_t values */
inline RttyParams rtty_params(int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx, int32_t atc_disable)
{
    static const RttyBpf space[RTTY_SHIFT_COUNT] = {
        { 5.944465260e+03, -0.9636529842, 3.3693752166, -4.9084595657, 3.4323354886 },   /*  85: 1000 Hz */
        { 1.513364927e+03, -0.9286270861, 3.1900687350, -4.6666321298, 3.3104336142 },   /* 170: 1085 Hz */
        { 1.513364944e+03, -0.9286270861, 3.1576917276, -4.6112830458, 3.2768349860 },   /* 200: 1115 Hz */
        { 1.513365018e+03, -0.9286270862, 2.8906128091, -4.1762457780, 2.9996788796 },   /* 425: 1340 Hz */
        { 1.513365019e+03, -0.9286270861, 2.8583904591, -4.1263569881, 2.9662407442 },   /* 450: 1365 Hz */
        { 1.513365057e+03, -0.9286270862, 2.1190223173, -3.1352567157, 2.1989754113 },   /* 850: 1765 Hz */
    };
    /* double literals rounded to float, as the reference's initialisers are */
    RttyParams p;
    p.space = space[shift_idx];
    p.mark = RttyBpf{ 1.513364755e+03, -0.9286270861, 3.3584472566, -4.9635817596, 3.4851652468 };
    p.lp = RttyLpf{ 5.944465310e+03, -0.9636529842, 1.9629800894 };
    p.one_bit = speed_idx == 0 ? 264 : 240;     /* roundf(12000 / 45.45f), roundf(12000 / 50) */
    p.stopbits = stopbits_idx;
    p.atc_disable = atc_disable != 0;
    return p;
}

/* the letters and figures tables; 0 is the blank, 7 the bell */
RTTY_HD uint8_t rtty_char(uint32_t code, bool figs)
{
    const char* letters = "\0E\nA SIU\rDRJNFCKTZLWHYPQOBG MXV ";
    const char* figures = "\0" "3\n- \a87\r$4',!:(5\")2#6019?& ./; ";
    return (uint8_t)(figs ? figures : letters)[code & 31u];
}

RTTY_HD float rtty_decayavg(float average, float input, int32_t weight)
{
    if (weight <= 1) return input;
    return ((input - average) / (float)weight) + average;
}

/* One channel: its state in registers, the text through the arena row. */
struct RttyChan
{
    float sx[4], sy[4], mx[4], my[4];       /* xv[1 .. 4], yv[1 .. 4] of the space and mark band-passes */
    float lx[2], ly[2];                     /* xv[1 .. 2], yv[1 .. 2] of the low-pass */
    float mark_env, space_env, mark_noise, space_noise;
    int32_t run, wfs, half, oldval, phase, byte, bytep, flags;
    uint32_t total;
    uint8_t* text;
    int32_t text_capacity;

    RTTY_HD void load(const RttyArena& a, int32_t c)
    {
        const size_t n = (size_t)a.C;
        const float* f = a.fs + c;
        for (int k = 0; k < 4; k++)
        {
            sx[k] = f[(RTTY_F_SX + k) * n]; sy[k] = f[(RTTY_F_SY + k) * n];
            mx[k] = f[(RTTY_F_MX + k) * n]; my[k] = f[(RTTY_F_MY + k) * n];
        }
        for (int k = 0; k < 2; k++) { lx[k] = f[(RTTY_F_LX + k) * n]; ly[k] = f[(RTTY_F_LY + k) * n]; }
        mark_env = f[RTTY_F_MARK_ENV * n]; space_env = f[RTTY_F_SPACE_ENV * n];
        mark_noise = f[RTTY_F_MARK_NOISE * n]; space_noise = f[RTTY_F_SPACE_NOISE * n];
        const int32_t* i = a.is + c;
        run = i[RTTY_I_RUN * n]; wfs = i[RTTY_I_WFS * n]; half = i[RTTY_I_HALF * n]; oldval = i[RTTY_I_OLDVAL * n];
        phase = i[RTTY_I_PHASE * n]; byte = i[RTTY_I_BYTE * n]; bytep = i[RTTY_I_BYTEP * n]; flags = i[RTTY_I_FLAGS * n];
        total = a.total[c];
        text = a.text + (size_t)c * a.text_capacity;
        text_capacity = a.text_capacity;
    }

    RTTY_HD void store(const RttyArena& a, int32_t c) const
    {
        const size_t n = (size_t)a.C;
        float* f = a.fs + c;
        for (int k = 0; k < 4; k++)
        {
            f[(RTTY_F_SX + k) * n] = sx[k]; f[(RTTY_F_SY + k) * n] = sy[k];
            f[(RTTY_F_MX + k) * n] = mx[k]; f[(RTTY_F_MY + k) * n] = my[k];
        }
        for (int k = 0; k < 2; k++) { f[(RTTY_F_LX + k) * n] = lx[k]; f[(RTTY_F_LY + k) * n] = ly[k]; }
        f[RTTY_F_MARK_ENV * n] = mark_env; f[RTTY_F_SPACE_ENV * n] = space_env;
        f[RTTY_F_MARK_NOISE * n] = mark_noise; f[RTTY_F_SPACE_NOISE * n] = space_noise;
        int32_t* i = a.is + c;
        i[RTTY_I_RUN * n] = run; i[RTTY_I_WFS * n] = wfs; i[RTTY_I_HALF * n] = half; i[RTTY_I_OLDVAL * n] = oldval;
        i[RTTY_I_PHASE * n] = phase; i[RTTY_I_BYTE * n] = byte; i[RTTY_I_BYTEP * n] = bytep; i[RTTY_I_FLAGS * n] = flags;
        a.total[c] = total;
    }

    /* UiDriver_TextMsgPutChar */
    RTTY_HD void put(uint8_t ch)
    {
        text[total % (uint32_t)text_capacity] = ch;
        ++total;
    }

    /* RttyDecoder_bandPassFreq: x[0 .. 3], y[0 .. 3] are xv[1 .. 4], yv[1 .. 4] before the step's shift,
       that is xv[0 .. 3], yv[0 .. 3] after it */
    RTTY_HD static float bandpass(float in, const RttyBpf& k, float* x, float* y)
    {
        const float x4 = in / k.gain;
        const float y4 = (x[0] + x4) - 2 * x[2] + (k.c0 * y[0]) + (k.c1 * y[1]) + (k.c2 * y[2]) + (k.c3 * y[3]);
        x[0] = x[1]; x[1] = x[2]; x[2] = x[3]; x[3] = x4;
        y[0] = y[1]; y[1] = y[2]; y[2] = y[3]; y[3] = y4;
        return y4;
    }

    /* RttyDecoder_lowPass */
    RTTY_HD float lowpass(float in, const RttyLpf& k)
    {
        const float x2 = in / k.gain;
        const float y2 = (lx[0] + x2) + 2 * lx[1] + (k.c0 * ly[0]) + (k.c1 * ly[1]);
        lx[0] = lx[1]; lx[1] = x2;
        ly[0] = ly[1]; ly[1] = y2;
        return y2;
    }

    /* RttyDecoder_demodulator: the bit of this sample, 1 = mark */
    RTTY_HD int32_t demodulate(float sample, const RttyParams& p)
    {
        float space_mag = bandpass(sample, p.space, sx, sy);
        float mark_mag = bandpass(sample, p.mark, mx, my);
        float v1;
        space_mag *= space_mag;
        mark_mag *= mark_mag;
        if (!p.atc_disable)
        {
            /* the reference swaps the two lines here and names them the other way round from then on */
            const float m = space_mag, s = mark_mag;
            const int32_t fast = p.one_bit / 4, slow = p.one_bit * 16, slower = p.one_bit * 48;
            /* envelopes: fast attack, slow decay; noise: fast fall, slower rise */
            mark_env = rtty_decayavg(mark_env, m, (m > mark_env) ? fast : slow);
            space_env = rtty_decayavg(space_env, s, (s > space_env) ? fast : slow);
            mark_noise = rtty_decayavg(mark_noise, m, (m < mark_noise) ? fast : slower);
            space_noise = rtty_decayavg(space_noise, s, (s < space_noise) ? fast : slower);
            const float noise_floor = (space_noise < mark_noise) ? space_noise : mark_noise;
            float mclipped = m > mark_env ? mark_env : m;
            float sclipped = s > space_env ? space_env : s;
            if (mclipped < noise_floor) mclipped = noise_floor;
            if (sclipped < noise_floor) sclipped = noise_floor;
            /* optimal ATC; the last subtraction is binary64 */
            const float a = (mclipped - noise_floor) * (mark_env - noise_floor) - (sclipped - noise_floor) * (space_env - noise_floor);
            const float b = (mark_env - noise_floor) * (mark_env - noise_floor) - (space_env - noise_floor) * (space_env - noise_floor);
            v1 = (float)((double)a - 0.25 * (double)b);
        }
        else
        {
            mark_mag *= -1;
            v1 = mark_mag + space_mag;
        }
        v1 = lowpass(v1, p.lp);
        return (v1 > 0) ? 0 : 1;
    }

    /* Rtty_Demodulator_ProcessSample */
    RTTY_HD void step(float sample, const RttyParams& p)
    {
        const int32_t bit = demodulate(sample, p);
        if (run == 0)
        {
            /* RttyDecoder_waitForStartBit: a mark, then a space, then still a space half a bit later */
            bool start = false;
            switch (wfs)
            {
            case 0: if (bit != 0) wfs++; break;
            case 1: if (bit != 1) wfs++; break;
            case 2:
                half = p.one_bit / 2;
                wfs++;
                /* fall through */
            default:
                half = (int16_t)(half - 1);
                if (half == 0)
                {
                    start = (bit == 0);
                    wfs = 0;
                }
                break;
            }
            if (start)
            {
                run = 1;
                bytep = 1;
                byte = 0;
            }
            return;
        }
        /* RttyDecoder_getBitDPLL: one phase correction per decoder lifetime, a bit per wrap of the phase */
        if (!(flags & RTTY_FLAG_PHASED) && bit != oldval)
        {
            if (phase < p.one_bit / 2) phase += p.one_bit / 32;
            else phase -= p.one_bit / 32;
            flags |= RTTY_FLAG_PHASED;
        }
        oldval = bit;
        phase++;
        if (phase < p.one_bit) return;
        phase -= p.one_bit;
        if (bytep == 6 || bytep == 7)
        {
            /* stop bits: a space is a framing error; with fewer than two stop bits the second is not awaited */
            if (bit == 0) run = 0;
            if (p.stopbits != RTTY_STOP_2 && bytep == 6) bytep = 7;
        }
        else byte |= bit << (bytep - 1);
        bytep++;
        if (bytep == 8 && run == 1)
        {
            if ((uint32_t)byte == RTTY_CODE_LTRS) flags &= ~RTTY_FLAG_FIGS;
            else if ((uint32_t)byte == RTTY_CODE_FIGS) flags |= RTTY_FLAG_FIGS;
            else put(rtty_char((uint32_t)byte, (flags & RTTY_FLAG_FIGS) != 0));
            run = 0;
        }
    }
};

/* n samples of one channel on the host, or of one lane without staging */
RTTY_HD void rtty_run_channel(const RttyArena& a, int32_t c, const RttyParams& p, const float* row, int32_t n)
{
    RttyChan ch;
    ch.load(a, c);
    for (int32_t i = 0; i < n; i++) ch.step(row[i], p);
    ch.store(a, c);
}

#endif
