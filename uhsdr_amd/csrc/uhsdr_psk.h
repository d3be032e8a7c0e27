/*
 * BPSK decoder (PSK31 / 63 / 125): one channel's demodulator and varicode framer, advanced by one
 * 12 ksps sample.
 *
 * Restates what the firmware runs per decimated sample in DEMOD_DIGI with digital_mode BPSK
 * (audio_driver.c:2547 -> Psk_Demodulator_ProcessSample, drivers/audio/psk.c:606-684, with the
 * 4th-order band-pass :397-412 and :582-599, the bit decision and framer :533-580, the varicode
 * lookup :493-504 and softdds_genIQSingleTone, softdds.c:60-78).  The input of a step is
 * a_buffer[0] after biquad_1, the sample the firmware hands its modems.
 *
 * The same functions run on the host (uhsdr_psk_process_host) and in the psk_decode kernel: both
 * address one field-major arena, so a channel's state is a column of it.
 *
 * Two kinds of state.  The oscillator's accumulator, rx_phase, the ring index rx_idx and
 * rx_symbol_idx never see the input: they are one PskClock per handle, advanced by psk_tick, and
 * every channel of a handle takes the same ticks.  The band-pass, the running sum, its 24-entry
 * product ring, rx_last_symbol, rx_word, rx_last_bit and the text are per channel (PskChan).
 *
 * Arithmetic follows the reference's C as gcc -O2 evaluates it with SSE and no contraction:
 *   - the band-pass accumulates 0 + b0 x0 + b1 x1 - a1 y1 + b2 x2 - a2 y2 + ... in binary32 in that
 *     order, the products of the zero coefficients b1 and b3 included (they turn -0, infinities
 *     and NaN visible), and divides by a[0] = 1;
 *   - the coefficient tables are double literals rounded to float;
 *   - rx_sum_sin += sin_mix - old in binary32 and is never cleared, so rounding residue stays;
 *   - rx_phase += 500.0 / 12000 is a binary64 add rounded to float on the store;
 *   - rx_sum_sin / 24 is a correctly rounded binary32 division and the bit is 0 iff the product
 *     rx_last_symbol * symbol is below 0: the product is not flushed when it is denormal.
 * The build has -ffp-contract=off.
 *
 * Left out, because nothing printed depends on them: the firmware overwrites rx_err_corr with 0
 * before its only use, so rx_err, the rx_scmix ring, the 48-element smax scan and cos_out feed
 * nothing.  cos_out is the only reader of rx_sum_cos, and that of the cos product ring and of the
 * oscillator's cosine, so these are left out as well.  symbol_store is assigned at every strobe
 * and read only at the strobe that decides, so the division runs there only.  rx_phase never falls
 * below 0, so the branch of psk.c:677 is never taken.  The band-pass ring of five is kept as the
 * last four inputs and outputs in the ring's order of use.
 *
 * Every static of the reference starts at zero, as in a fresh process.
 */
#ifndef UHSDR_PSK_H
#define UHSDR_PSK_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PSK_HD __host__ __device__ inline
#else
#define PSK_HD inline
#endif

#define PSK_SPEED_COUNT 3
#define PSK_RING        24              /* PSK_BUF_LEN = 12000 / 500: one period of the 500 Hz carrier */
#define PSK_DDS_STEP    178956970u      /* softdds_stepForSampleRate(500, 12000) = ((500 * 1024) << 22) / 12000 */
#define PSK_SHIFT_DIFF  (1.0 * 500 / 12000)
#define PSK_CODES       4096            /* varicode lookup: codes have at most 12 bits */

/* float state of a channel, rows of PskArena::fs */
enum { PSK_F_X = 0, PSK_F_Y = 4, PSK_F_SUM = 8, PSK_F_SYMBOL, PSK_F_RING, PSK_F_COUNT = PSK_F_RING + PSK_RING };
/* integer state, rows of PskArena::is */
enum { PSK_I_WORD = 0, PSK_I_LAST_BIT, PSK_I_COUNT };

/* All channels' state, field-major, and the two tables (in the memory the state is in). */
struct PskArena
{
    int32_t C;
    int32_t text_capacity;
    const float* sine;       /* [1024] the oscillator's table as floats */
    const uint8_t* chars;    /* [PSK_CODES] varicode -> byte, '*' where no code matches */
    float* fs;               /* [PSK_F_COUNT][C]; row PSK_F_SYMBOL is the symbol output */
    uint32_t* is;            /* [PSK_I_COUNT][C] */
    uint32_t* total;         /* [C] */
    uint8_t* text;           /* [C][text_capacity], character k at k % text_capacity */
};

/* The launch constants of a decoder (Psk_Modem_Init): the band-pass and strobes per bit */
struct PskParams
{
    float b[5], a[5];
    int32_t symbol_len;      /* rx_symbol_len = rate / 24: 16, 8, 4 */
};

/* order-2 Butterworth band-passes around 500 Hz at 12 ksps, as wide as the speed needs */
inline PskParams psk_params(int32_t speed_idx)
{
    /* double literals rounded to float, as the reference's initialisers are */
    static const PskParams speeds[PSK_SPEED_COUNT] = {
        { { 6.6165543533213894e-05, 0.0, -0.00013233108706642779, 0.0, 6.6165543533213894e-05 },
          { 1.0, -3.8414813063247664, 5.6662277107033248, -3.7972899991488904, 0.9771256616899302 }, 16 },
        { { 0.0002616526950658905, 0.0, -0.000523305390131781, 0.0, 0.0002616526950658905 },
          { 1.0, -3.8195192250239174, 5.6013869366249818, -3.7321386869273105, 0.95477455992103932 }, 8 },
        { { 0.0010232176384709002, 0.0, -0.0020464352769418003, 0.0, 0.0010232176384709002 },
          { 1.0, -3.7763786572915334, 5.4745855184361272, -3.6055008493327723, 0.91159449659996006 }, 4 },
    };
    return speeds[speed_idx];
}

/* G3PLX varicode of the ASCII half, byte -> code: every code starts and ends with a 1 bit and has
   no two 0 bits in a row; the shortest codes go to the most frequent characters of English text */
static const uint16_t psk_varicode_ascii[128] = {
    0x2AB, 0x2DB, 0x2ED, 0x377, 0x2EB, 0x35F, 0x2EF, 0x2FD, 0x2FF, 0x0EF, 0x01D, 0x36F, 0x2DD, 0x01F, 0x375, 0x3AB,
    0x2F7, 0x2F5, 0x3AD, 0x3AF, 0x35B, 0x36B, 0x36D, 0x357, 0x37B, 0x37D, 0x3B7, 0x355, 0x35D, 0x3BB, 0x2FB, 0x37F,
    0x001, 0x1FF, 0x15F, 0x1F5, 0x1DB, 0x2D5, 0x2BB, 0x17F, 0x0FB, 0x0F7, 0x16F, 0x1DF, 0x075, 0x035, 0x057, 0x1AF,
    0x0B7, 0x0BD, 0x0ED, 0x0FF, 0x177, 0x15B, 0x16B, 0x1AD, 0x1AB, 0x1B7, 0x0F5, 0x1BD, 0x1ED, 0x055, 0x1D7, 0x2AF,
    0x2BD, 0x07D, 0x0EB, 0x0AD, 0x0B5, 0x077, 0x0DB, 0x0FD, 0x155, 0x07F, 0x1FD, 0x17D, 0x0D7, 0x0BB, 0x0DD, 0x0AB,
    0x0D5, 0x1DD, 0x0AF, 0x06F, 0x06D, 0x157, 0x1B5, 0x15D, 0x175, 0x17B, 0x2AD, 0x1F7, 0x1EF, 0x1FB, 0x2BF, 0x16D,
    0x2DF, 0x00B, 0x05F, 0x02F, 0x02D, 0x003, 0x03D, 0x05B, 0x02B, 0x00D, 0x1EB, 0x0BF, 0x01B, 0x03B, 0x00F, 0x007,
    0x03F, 0x1BF, 0x015, 0x017, 0x005, 0x037, 0x07B, 0x06B, 0x0DF, 0x05D, 0x1D5, 0x2B7, 0x1BB, 0x2B5, 0x2D7, 0x3B5,
};

inline bool psk_varicode_valid(uint32_t code)
{
    if (!(code & 1u)) return false;
    for (uint32_t c = code; c > 1u; c >>= 1) if ((c & 3u) == 0u) return false;
    return true;
}

/* The lookup the decoder uses, code -> byte.  Bytes 128 .. 255 take, in increasing order, the valid
   codes the ASCII half leaves unused.  '*' (also the byte of code 0x16F) where no code matches. */
inline void psk_fill_chars(uint8_t* chars)
{
    for (int k = 0; k < PSK_CODES; k++) chars[k] = (uint8_t)'*';
    bool used[PSK_CODES] = { false };
    for (int k = 0; k < 128; k++) { chars[psk_varicode_ascii[k]] = (uint8_t)k; used[psk_varicode_ascii[k]] = true; }
    int next = 128;
    for (uint32_t code = 1; code < PSK_CODES && next < 256; code++)
        if (psk_varicode_valid(code) && !used[code]) chars[code] = (uint8_t)next++;
}

/* The state no input reaches: the same for every channel of a handle */
struct PskClock
{
    uint32_t acc;        /* psk_rx_dds.acc */
    float phase;         /* rx_phase */
    int32_t idx;         /* rx_idx */
    int32_t sym;         /* rx_symbol_idx */
};

/* What a sample's step needs of the clock */
struct PskTick
{
    uint32_t sine;       /* index of vco_sin in the oscillator's table */
    int32_t slot;        /* rx_idx of this sample */
    bool decide;         /* BpskDecoder_NextSymbol runs and completes a bit */
};

PSK_HD uint32_t psk_sine_index(uint32_t acc) { return (acc >> 22) % 1024u; }

/* one sample of the clock: softdds_nextSampleIndex, the phase counter, the strobe count, rx_idx */
PSK_HD PskTick psk_tick(PskClock& k, int32_t symbol_len)
{
    PskTick t;
    t.sine = psk_sine_index(k.acc);
    k.acc += PSK_DDS_STEP;
    t.slot = k.idx;
    t.decide = false;
    k.phase = (float)((double)k.phase + PSK_SHIFT_DIFF);
    if (k.phase > 1)
    {
        k.phase -= 1;
        k.sym += 1;
        if (k.sym >= symbol_len)
        {
            k.sym = 0;
            t.decide = true;
        }
    }
    k.idx = (k.idx + 1) % PSK_RING;
    return t;
}

/* One channel: its state in registers, the product ring and the text through memory. */
struct PskChan
{
    float x[4], y[4];            /* the band-pass' inputs and outputs of the last four samples, latest first */
    float sum;                   /* rx_sum_sin */
    float last_symbol;           /* rx_last_symbol */
    uint32_t word;               /* rx_word */
    uint32_t last_bit;           /* rx_last_bit */
    uint32_t total;
    uint8_t* text;
    int32_t text_capacity;

    PSK_HD void load(const PskArena& a, int32_t c)
    {
        const size_t n = (size_t)a.C;
        const float* f = a.fs + c;
        for (int k = 0; k < 4; k++) { x[k] = f[(PSK_F_X + k) * n]; y[k] = f[(PSK_F_Y + k) * n]; }
        sum = f[PSK_F_SUM * n];
        last_symbol = f[PSK_F_SYMBOL * n];
        word = a.is[PSK_I_WORD * n + c];
        last_bit = a.is[PSK_I_LAST_BIT * n + c];
        total = a.total[c];
        text = a.text + (size_t)c * a.text_capacity;
        text_capacity = a.text_capacity;
    }

    PSK_HD void store(const PskArena& a, int32_t c) const
    {
        const size_t n = (size_t)a.C;
        float* f = a.fs + c;
        for (int k = 0; k < 4; k++) { f[(PSK_F_X + k) * n] = x[k]; f[(PSK_F_Y + k) * n] = y[k]; }
        f[PSK_F_SUM * n] = sum;
        f[PSK_F_SYMBOL * n] = last_symbol;
        a.is[PSK_I_WORD * n + c] = word;
        a.is[PSK_I_LAST_BIT * n + c] = last_bit;
        a.total[c] = total;
    }

    /* UiDriver_TextMsgPutChar */
    PSK_HD void put(uint8_t ch)
    {
        text[total % (uint32_t)text_capacity] = ch;
        ++total;
    }

    /* BpskDecoder_Bandpass with Psk_IirNext */
    PSK_HD float bandpass(float in, const PskParams& p)
    {
        float resp = 0;
        resp += p.b[0] * in;
        resp += p.b[1] * x[0];
        resp -= p.a[1] * y[0];
        resp += p.b[2] * x[1];
        resp -= p.a[2] * y[1];
        resp += p.b[3] * x[2];
        resp -= p.a[3] * y[2];
        resp += p.b[4] * x[3];
        resp -= p.a[4] * y[3];
        resp = resp / p.a[0];
        x[3] = x[2]; x[2] = x[1]; x[1] = x[0]; x[0] = in;
        y[3] = y[2]; y[2] = y[1]; y[1] = y[0]; y[0] = resp;
        return resp;
    }

    /* Psk_Demodulator_ProcessSample down to the running sum: `old` is rx_sin_prod[rx_idx] as the
       sample finds it, the return value what the sample leaves there */
    PSK_HD float mix(float sample, float vco_sin, float old, const PskParams& p)
    {
        const float fsample = bandpass(sample, p);
        const float sin_mix = vco_sin * fsample;
        sum += sin_mix - old;
        return sin_mix;
    }

    /* BpskDecoder_NextSymbol at the strobe that completes a bit */
    PSK_HD void decide(const uint8_t* chars)
    {
        const float symbol = sum / PSK_RING;
        const uint32_t bit = (last_symbol * symbol < 0) ? 0u : 1u;
        last_symbol = symbol;
        /* two 0 bits in a row after at least one 1 bit end a character; the last 0 is shifted out */
        if (last_bit == 0u && bit == 0u && word != 0u)
        {
            const uint16_t code = (uint16_t)(word >> 1);
            put(code < PSK_CODES ? chars[code] : (uint8_t)'*');
            word = 0;
        }
        else word = (word << 1) | bit;
        last_bit = bit;
    }
};

/* n samples of one channel on the host from the clock `k` (a copy: every channel starts from the
   handle's) */
inline void psk_run_channel(const PskArena& a, int32_t c, const PskParams& p, PskClock k, const float* row, int32_t n)
{
    PskChan ch;
    ch.load(a, c);
    float* ring = a.fs + (size_t)PSK_F_RING * a.C + c;
    for (int32_t i = 0; i < n; i++)
    {
        const PskTick t = psk_tick(k, p.symbol_len);
        float* slot = ring + (size_t)t.slot * a.C;
        *slot = ch.mix(row[i], a.sine[t.sine], *slot, p);
        if (t.decide) ch.decide(a.chars);
    }
    ch.store(a, c);
}

#endif
