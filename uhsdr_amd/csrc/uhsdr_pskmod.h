/*
 * BPSK modulator (PSK31 / 63 / 125): one channel's varicode framer, envelope and carrier, advanced
 * by one 48 ksps sample.
 *
 * Restates what the firmware runs per transmit sample in DEMOD_DIGI with digital_mode BPSK
 * (tx_processor.c:833-845 -> Psk_Modulator_GenSample, drivers/audio/psk.c:686-841, with
 * Psk_Modulator_SetState :860-887, Psk_Modulator_PrepareTx :437-440, Bpsk_FindCharReversed
 * :506-521, Bpsk_ResetWin :431-435 and the oscillators of Psk_Modem_Init :475-490).  A step returns
 * the int16 the firmware's call returns.  Everything is integer arithmetic; the only division is
 * the int32 one by SAMPLE_MAX, truncating as C does.
 *
 * The same function runs on the host (uhsdr_pskmod_process_host) and in the pskmod_gen kernel.
 *
 * Kept as the firmware has them:
 *   - a bit lasts tx_bit_len / 2 samples; it starts at phase tx_bit_len / 4 and the sign changes in
 *     its middle, at phase 0, where the raised envelope restarts from zero;
 *   - the preamble is zeros until their count reaches the speed value (31.25, 62.5, 125: an integer
 *     compared with a float), then the state is ACTIVE; between characters two zeros are sent, and
 *     with an empty queue zeros go on;
 *   - a character's varicode is sent from its most significant bit; the reversal leaves a 0 in
 *     front, so a character is preceded by three zeros in all;
 *   - EOT changes to POSTAMBLE: 16 ones at a time until their count reaches the speed value, then
 *     INACTIVE, one last shaped bit, and OFF in its middle, where TX-off is requested; text that
 *     follows an EOT in the queue is still taken when the 16 ones are out, as the firmware does;
 *   - while OFF a step returns 0 and advances nothing, the carrier's accumulator included;
 *   - PrepareTx restarts the framer and leaves both oscillators' accumulators as they are;
 *   - the product coeff * sign * carrier / 32766 is returned through int16: an envelope of 32767
 *     on a carrier of 32767 wraps, as it does there.
 * QPSK is not built: the reference has no QPSK modulator either.
 */
#ifndef UHSDR_PSKMOD_H
#define UHSDR_PSKMOD_H

#include "uhsdr_digiq.h"

#define PSKMOD_SPEED_COUNT 3
#define PSKMOD_SAMPLE_MAX  32766

enum { PSKMOD_OFF = 0, PSKMOD_PREAMBLE, PSKMOD_ACTIVE, PSKMOD_POSTAMBLE, PSKMOD_INACTIVE };

/* integer state, rows of DigiModArena::is; the modulator state is DigiModArena::state */
enum
{
    PSKMOD_I_ACC = 0,        /* psk_dds.acc, the 500 Hz carrier */
    PSKMOD_I_BIT_ACC,        /* psk_bit_dds.acc, the envelope at half the bit rate */
    PSKMOD_I_BITS,           /* tx_bits, 16 bits */
    PSKMOD_I_PHASE,          /* tx_bit_phase */
    PSKMOD_I_SIGNS,          /* tx_wave_sign_next in the low half, tx_wave_sign_current in the high half, as int16 */
    PSKMOD_I_ZEROS,          /* tx_zeros */
    PSKMOD_I_ONES,           /* tx_ones */
    PSKMOD_I_WIN,            /* tx_win */
    PSKMOD_I_COUNT
};

/* The launch constants of a modulator (Psk_Modem_Init) */
struct PskModParams
{
    uint32_t step, bit_step; /* softdds_stepForSampleRate(500, 48000) and (speed / 2, 48000) */
    uint32_t half_len;       /* tx_bit_len / 2: samples per bit */
    uint32_t quarter_len;    /* tx_bit_len / 4: the phase a bit starts at */
    float speed;             /* psk_speeds[].value */
};

inline PskModParams pskmod_params(int32_t speed_idx)
{
    static const float speeds[PSKMOD_SPEED_COUNT] = { 31.25f, 62.5f, 125.0f };
    PskModParams p;
    p.speed = speeds[speed_idx];
    p.step = digi_dds_step(500, 48000);
    p.bit_step = digi_dds_step((float)(p.speed / 2.0), 48000);
    const uint32_t bit_len = (uint32_t)(48000 / p.speed * 2 + 0.5f);        /* lround: 3072, 1536, 768 */
    p.half_len = bit_len / 2;
    p.quarter_len = bit_len / 4;
    return p;
}

/* One channel: its state and its end of the text queue in registers. */
struct PskModChan
{
    uint32_t acc, bit_acc;
    uint32_t bits, phase;
    int32_t sign_next, sign_current, zeros, ones;
    uint32_t win, state;
    DigiQueue q;

    DIGI_HD void load(const DigiModArena& a, int32_t c)
    {
        const size_t n = (size_t)a.C;
        const uint32_t* i = a.is + c;
        acc = i[PSKMOD_I_ACC * n]; bit_acc = i[PSKMOD_I_BIT_ACC * n];
        bits = i[PSKMOD_I_BITS * n]; phase = i[PSKMOD_I_PHASE * n];
        const uint32_t signs = i[PSKMOD_I_SIGNS * n];
        sign_next = (int16_t)(signs & 0xffffu); sign_current = (int16_t)(signs >> 16);
        zeros = (int32_t)i[PSKMOD_I_ZEROS * n]; ones = (int32_t)i[PSKMOD_I_ONES * n];
        win = i[PSKMOD_I_WIN * n];
        state = a.state[c];
        q.load(a, c);
    }

    DIGI_HD void store(const DigiModArena& a, int32_t c) const
    {
        const size_t n = (size_t)a.C;
        uint32_t* i = a.is + c;
        i[PSKMOD_I_ACC * n] = acc; i[PSKMOD_I_BIT_ACC * n] = bit_acc;
        i[PSKMOD_I_BITS * n] = bits; i[PSKMOD_I_PHASE * n] = phase;
        i[PSKMOD_I_SIGNS * n] = ((uint32_t)sign_next & 0xffffu) | ((uint32_t)sign_current << 16);
        i[PSKMOD_I_ZEROS * n] = (uint32_t)zeros; i[PSKMOD_I_ONES * n] = (uint32_t)ones;
        i[PSKMOD_I_WIN * n] = win;
        a.state[c] = (uint8_t)state;
        q.store(a, c);
    }

    /* Psk_Modulator_PrepareTx: Psk_Modulator_SetState(PSK_MOD_PREAMBLE) */
    DIGI_HD void prepare_tx()
    {
        ones = 0;
        win = 1;
        bits = 0;
        sign_next = 1;
        sign_current = 1;
        phase = 0;
        zeros = 0;
        state = PSKMOD_PREAMBLE;
    }

    /* the state of a fresh process after Psk_Modem_Init and Psk_Modulator_PrepareTx, the queue empty */
    DIGI_HD void reset()
    {
        acc = bit_acc = 0;
        q.put = q.consumed = 0;
        q.txoff_at = DIGI_NO_TXOFF;
        prepare_tx();
    }

    /* Bpsk_FindCharReversed: the code's bits in reverse above a 0 */
    static DIGI_HD uint32_t reversed(uint32_t code)
    {
        uint32_t r = 0;
        while (code > 0)
        {
            r |= code & 1u;
            r = (r << 1) & 0xffffu;
            code >>= 1;
        }
        return r;
    }

    /* Psk_Modulator_GenSample; `t` is the sample's index since reset, `codes` the varicode table */
    DIGI_HD int16_t step(const int16_t* sine, const uint16_t* codes, const PskModParams& p, uint32_t t)
    {
        if (state == PSKMOD_OFF) return 0;
        if (phase == p.quarter_len)
        {
            if (bits == 0)
            {
                if (zeros < 2 || state == PSKMOD_PREAMBLE)
                {
                    zeros = (int16_t)(zeros + 1);
                    if (state == PSKMOD_PREAMBLE && (float)zeros >= p.speed) state = PSKMOD_ACTIVE;
                }
                else if (q.has_data())
                {
                    const uint8_t ch = q.remove();
                    state = PSKMOD_ACTIVE;
                    if (ch == DIGI_EOT) state = PSKMOD_POSTAMBLE;
                    else
                    {
                        bits = reversed(codes[ch]);
                        zeros = 0;
                        ones = 0;
                    }
                }
                if (state == PSKMOD_POSTAMBLE)
                {
                    if ((float)ones < p.speed)
                    {
                        ones = (int16_t)(ones + 16);
                        bits = 0xffffu;
                    }
                    else state = PSKMOD_INACTIVE;
                }
            }
            if ((bits & 1u) == 0 && ones == 0) sign_next = -sign_next;
            win = (sign_next != sign_current || state == PSKMOD_INACTIVE) ? 1u : 0u;
            bits >>= 1;
        }
        if (phase == 0)
        {
            sign_current = sign_next;
            if (win) bit_acc = 0;
            if (state == PSKMOD_INACTIVE)
            {
                q.request_txoff(t);
                state = PSKMOD_OFF;
            }
        }
        int32_t coeff = PSKMOD_SAMPLE_MAX;
        if (win)
        {
            const int32_t e = digi_dds_next(sine, bit_acc, p.bit_step);
            coeff = e < 0 ? -e : e;
        }
        phase = (phase + 1u) % p.half_len;
        const int32_t carrier = digi_dds_next(sine, acc, p.step);
        return (int16_t)((coeff * sign_current * carrier) / PSKMOD_SAMPLE_MAX);
    }
};

#endif
