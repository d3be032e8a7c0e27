/*
 * RTTY modulator: one channel's Baudot framer and two-tone generator, advanced by one 48 ksps
 * sample.
 *
 * Restates what the firmware runs per transmit sample in DEMOD_DIGI with digital_mode RTTY
 * (tx_processor.c:811-822 -> Rtty_Modulator_GenSample, drivers/audio/rtty.c:806-932, with
 * Rtty_BaudotAdd :748-769, Rtty_Modulator_Code2Bits :771-793, Rtty_Modulator_StartTX :796-802, the
 * Ascii2Baudot table :43-173 and the two oscillators of Rtty_Modem_Init :445-446).  A step returns
 * the int16 the firmware's call returns.  Everything is integer arithmetic: a table look-up per
 * oscillator step, nothing is rounded.
 *
 * The same function runs on the host (uhsdr_rttymod_process_host) and in the rttymod_gen kernel.
 *
 * Kept as the firmware has them:
 *   - a character is a start bit, five code bits from the least significant one and one stop bit
 *     (stopbits 1) or two (1.5 and 2 alike); LTRS or FIGS goes in front only when the set changes;
 *   - the bit word is shifted before the test for an empty word, so after StartTX in the middle of a
 *     character the first bit of the LTRS pair it loads is shifted out unsent;
 *   - StartTX passes the bare LTRS code, whose mode bit says "figures": it loads FIGS, LTRS;
 *   - characters are taken until one has a Baudot code; EOT requests TX-off and the loop goes on;
 *     the byte is masked with 0x7f and code 0 is "none";
 *   - with an empty queue the idle character is LTRS, tagged as a letter;
 *   - the phase-continuous tone change: the old tone runs on until its sine passes from below to
 *     not below zero (mark to space) or until the sample after its positive peak (space to mark);
 *     the new oscillator then takes the old one's accumulator and steps a second time in that
 *     sample; last_value is set to INT16_MIN when the space-to-mark wait begins and assigned the
 *     returned sample at the end of every call;
 *   - StartTX leaves char_bit_samples, the wait state and both accumulators as they are.
 */
#ifndef UHSDR_RTTYMOD_H
#define UHSDR_RTTYMOD_H

#include "uhsdr_digiq.h"

#define RTTYMOD_SHIFT_COUNT 6
#define RTTYMOD_SPEED_COUNT 2
#define RTTYMOD_STOP_COUNT  3
#define RTTYMOD_FIGS        0x1bu       /* RTTY_SYMBOL_CODE */
#define RTTYMOD_LTRS        0x1fu       /* RTTY_LETTER_CODE */
#define RTTYMOD_LETTER      0x20u       /* RTTY_CODE_MODE_LETTER, the mode bit of a table entry */

/* integer state, rows of DigiModArena::is */
enum
{
    RTTYMOD_I_ACC_SPACE = 0, /* tx_dds[0].acc */
    RTTYMOD_I_ACC_MARK,      /* tx_dds[1].acc */
    RTTYMOD_I_BIT_SAMPLES,   /* char_bit_samples */
    RTTYMOD_I_BITS,          /* char_bits, 16 bits */
    RTTYMOD_I_BIT_IDX,       /* char_bit_idx, 8 bits */
    RTTYMOD_I_LAST_BIT,
    RTTYMOD_I_CURRENT_BIT,
    RTTYMOD_I_MSK,           /* msk_state */
    RTTYMOD_I_FIGS,          /* char_mode: 1 figures */
    RTTYMOD_I_LAST_VALUE,    /* int16, sign-extended */
    RTTYMOD_I_COUNT
};
enum { RTTYMOD_MSK_IDLE = 0, RTTYMOD_MSK_WAIT_NEG, RTTYMOD_MSK_WAIT_PLUS, RTTYMOD_MSK_WAIT_PLUSGRAD, RTTYMOD_MSK_WAIT_MAX };

/* The launch constants of a modulator (Rtty_Modem_Init) */
struct RttyModParams
{
    uint32_t step[2];        /* space, mark: softdds_stepForSampleRate(freq, 48000) */
    uint32_t bit_samples;    /* oneBitSampleCount * 4 */
    int32_t one_stop;        /* stopbits 1: a character is 7 bits, else 8 */
};

inline RttyModParams rttymod_params(int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx)
{
    /* the centre of the decoder's space band-pass, 915 Hz + shift; mark is 915 Hz */
    static const float space[RTTYMOD_SHIFT_COUNT] = { 1000, 1085, 1115, 1340, 1365, 1765 };
    RttyModParams p;
    p.step[0] = digi_dds_step(space[shift_idx], 48000);
    p.step[1] = digi_dds_step(915, 48000);
    p.bit_samples = (speed_idx == 0 ? 264u : 240u) * 4u;    /* roundf(12000 / 45.45f), roundf(12000 / 50) */
    p.one_stop = stopbits_idx == 0;
    return p;
}

/* byte & 0x7f -> Baudot code, RTTYMOD_LETTER set for the letters set, 0 where there is none.  The
   figures are the decoder's table read backwards, except that BEL and the apostrophe have changed
   places (the firmware sends 0x0b for BEL and 0x05 for the apostrophe); line feed and carriage
   return count as figures; lower case is sent as upper case. */
inline void rttymod_fill_codes(uint16_t* codes)
{
    /* bytes 32 .. 95 */
    static const uint8_t printable[64] = {
        0x24, 0x0d, 0x11, 0x14, 0x09, 0x00, 0x1a, 0x05, 0x0f, 0x12, 0x00, 0x00, 0x0c, 0x03, 0x1c, 0x1d,
        0x16, 0x17, 0x13, 0x01, 0x0a, 0x10, 0x15, 0x07, 0x06, 0x18, 0x0e, 0x1e, 0x00, 0x00, 0x00, 0x19,
        0x00, 0x23, 0x39, 0x2e, 0x29, 0x21, 0x2d, 0x3a, 0x34, 0x26, 0x2b, 0x2f, 0x32, 0x3c, 0x2c, 0x38,
        0x36, 0x37, 0x2a, 0x25, 0x30, 0x27, 0x3e, 0x33, 0x3d, 0x35, 0x31, 0x00, 0x00, 0x00, 0x00, 0x00,
    };
    for (int k = 0; k < 128; k++) codes[k] = 0;
    codes[7] = 0x0b;
    codes['\n'] = 0x02;
    codes['\r'] = 0x08;
    for (int k = 32; k < 96; k++) codes[k] = printable[k - 32];
    for (int k = 'a'; k <= 'z'; k++) codes[k] = codes[k - 32];
}

/* One channel: its state and its end of the text queue in registers. */
struct RttyModChan
{
    uint32_t acc_space, acc_mark;
    uint32_t bit_samples, bits, bit_idx;
    uint32_t last_bit, current_bit, msk, figs;
    int32_t last_value;
    DigiQueue q;

    DIGI_HD void load(const DigiModArena& a, int32_t c)
    {
        const size_t n = (size_t)a.C;
        const uint32_t* i = a.is + c;
        acc_space = i[RTTYMOD_I_ACC_SPACE * n]; acc_mark = i[RTTYMOD_I_ACC_MARK * n];
        bit_samples = i[RTTYMOD_I_BIT_SAMPLES * n]; bits = i[RTTYMOD_I_BITS * n]; bit_idx = i[RTTYMOD_I_BIT_IDX * n];
        last_bit = i[RTTYMOD_I_LAST_BIT * n]; current_bit = i[RTTYMOD_I_CURRENT_BIT * n];
        msk = i[RTTYMOD_I_MSK * n]; figs = i[RTTYMOD_I_FIGS * n];
        last_value = (int32_t)i[RTTYMOD_I_LAST_VALUE * n];
        q.load(a, c);
    }

    DIGI_HD void store(const DigiModArena& a, int32_t c) const
    {
        const size_t n = (size_t)a.C;
        uint32_t* i = a.is + c;
        i[RTTYMOD_I_ACC_SPACE * n] = acc_space; i[RTTYMOD_I_ACC_MARK * n] = acc_mark;
        i[RTTYMOD_I_BIT_SAMPLES * n] = bit_samples; i[RTTYMOD_I_BITS * n] = bits; i[RTTYMOD_I_BIT_IDX * n] = bit_idx;
        i[RTTYMOD_I_LAST_BIT * n] = last_bit; i[RTTYMOD_I_CURRENT_BIT * n] = current_bit;
        i[RTTYMOD_I_MSK * n] = msk; i[RTTYMOD_I_FIGS * n] = figs;
        i[RTTYMOD_I_LAST_VALUE * n] = (uint32_t)last_value;
        q.store(a, c);
    }

    /* Rtty_BaudotAdd: start bit, code, stop bits, above the bits already in the word */
    DIGI_HD void add(uint32_t code, const RttyModParams& p)
    {
        uint32_t b = (code << 1) & 0xffu;
        b |= p.one_stop ? 0x40u : 0xc0u;
        bits = (bits | (b << bit_idx)) & 0xffffu;
        bit_idx = (bit_idx + (p.one_stop ? 7u : 8u)) & 0xffu;
    }

    /* Rtty_Modulator_Code2Bits */
    DIGI_HD void code2bits(uint32_t info, const RttyModParams& p)
    {
        bits = 0;
        bit_idx = 0;
        const uint32_t want_figs = (info & RTTYMOD_LETTER) ? 0u : 1u;
        if (figs != want_figs)
        {
            figs = want_figs;
            add(want_figs ? RTTYMOD_FIGS : RTTYMOD_LTRS, p);
        }
        add(info & 0xffu & ~RTTYMOD_LETTER, p);
    }

    /* Rtty_Modulator_StartTX */
    DIGI_HD void start_tx(const RttyModParams& p)
    {
        last_bit = 1;
        last_value = INT16_MIN;
        figs = 0;
        code2bits(RTTYMOD_LTRS, p);
    }

    /* the state of a fresh process after Rtty_Modem_Init and Rtty_Modulator_StartTX, the queue empty */
    DIGI_HD void reset(const RttyModParams& p)
    {
        acc_space = acc_mark = 0;
        bit_samples = 0;
        current_bit = 0;
        msk = RTTYMOD_MSK_IDLE;
        q.put = q.consumed = 0;
        q.txoff_at = DIGI_NO_TXOFF;
        start_tx(p);
    }

    /* softdds_nextSample(&tx_dds[bit]) */
    DIGI_HD int16_t tone(const int16_t* sine, const RttyModParams& p, uint32_t bit)
    {
        uint32_t acc = bit ? acc_mark : acc_space;
        const int16_t v = digi_dds_next(sine, acc, bit ? p.step[1] : p.step[0]);
        if (bit) acc_mark = acc; else acc_space = acc;
        return v;
    }

    /* the end of a wait: the new tone goes on from the old one's phase and steps once more */
    DIGI_HD int16_t change_tone(const int16_t* sine, const RttyModParams& p)
    {
        msk = RTTYMOD_MSK_IDLE;
        current_bit = bits & 1u;
        const uint32_t acc = last_bit ? acc_mark : acc_space;
        if (current_bit) acc_mark = acc; else acc_space = acc;
        last_bit = current_bit;
        return tone(sine, p, current_bit);
    }

    /* Rtty_Modulator_GenSample; `t` is the sample's index since reset, `codes` rttymod_fill_codes */
    DIGI_HD int16_t step(const int16_t* sine, const uint16_t* codes, const RttyModParams& p, uint32_t t)
    {
        if (bit_samples == 0)
        {
            bit_samples = p.bit_samples;
            bits >>= 1;
            if (bit_idx == 0)
            {
                bool filled = false;
                while (!filled && q.has_data())
                {
                    const uint8_t ascii = q.remove();
                    if (ascii == DIGI_EOT) q.request_txoff(t);
                    else
                    {
                        const uint32_t baudot = codes[ascii & 0x7f];
                        if (baudot > 0)
                        {
                            code2bits(baudot, p);
                            filled = true;
                        }
                    }
                }
                if (!filled) code2bits(RTTYMOD_LTRS | RTTYMOD_LETTER, p);
            }
            bit_idx = (bit_idx - 1u) & 0xffu;
            current_bit = bits & 1u;
            if (last_bit != current_bit)
            {
                if (last_bit == 1u) msk = RTTYMOD_MSK_WAIT_NEG;
                else
                {
                    msk = RTTYMOD_MSK_WAIT_PLUSGRAD;
                    last_value = INT16_MIN;
                }
                current_bit = last_bit;
            }
        }
        bit_samples--;

        int16_t value = tone(sine, p, current_bit);
        switch (msk)
        {
        case RTTYMOD_MSK_WAIT_NEG:
            if (value < 0) msk = RTTYMOD_MSK_WAIT_PLUS;
            break;
        case RTTYMOD_MSK_WAIT_PLUS:
            if (value >= 0) value = change_tone(sine, p);
            break;
        case RTTYMOD_MSK_WAIT_PLUSGRAD:
            if (value > last_value) msk = RTTYMOD_MSK_WAIT_MAX;
            break;
        case RTTYMOD_MSK_WAIT_MAX:
            if (value >= last_value) last_value = value;
            else if (last_value > 0) value = change_tone(sine, p);
            break;
        default:
            break;
        }
        last_value = value;
        return value;
    }
};

#endif
