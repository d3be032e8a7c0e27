/*
 * What the RTTY and BPSK modulators share: the per-channel text queue, the softdds oscillator and
 * the field-major arena both address (uhsdr_rttymod.h, uhsdr_pskmod.h, uhsdr_digimod.hip).
 *
 * The queue models the firmware's ring (drivers/audio/cw/uhsdr_digi_buffer.c): a byte FIFO the
 * modulator takes one character from at a time.  The producer (put, a host call) and the consumer
 * (consumed, the modulator) count characters since reset; character k lies at k % text_capacity and
 * one slot stays free, so put - consumed <= text_capacity - 1.  The counters are 32 bits wide: they
 * would wrap after 2^32 characters, decades of text at the fastest mode.  The firmware's consumer
 * tag (active_consumer) is not modelled, the queue always belongs to the handle's modulator, and
 * the echo of a removed character to UiDriver_TextMsgPutChar is what `consumed` counts.
 */
#ifndef UHSDR_DIGIQ_H
#define UHSDR_DIGIQ_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DIGI_HD __host__ __device__ inline
#else
#define DIGI_HD inline
#endif

#define DIGI_NO_TXOFF 0xffffffffu
#define DIGI_EOT      0x04u

/* All channels' state, field-major, and the two tables (in the memory the state is in). */
struct DigiModArena
{
    int32_t C;
    int32_t text_capacity;
    const int16_t* sine;     /* [1024] the softdds table */
    const uint16_t* codes;   /* RTTY: [128] byte -> Baudot code and mode bit; BPSK: [256] byte -> varicode */
    uint32_t* is;            /* [rows][C], the modulator's own state */
    uint32_t* consumed;      /* [C] characters taken since reset */
    uint32_t* txoff_at;      /* [C] index since reset of the first sample that requested TX-off */
    uint32_t* put;           /* [C] characters put since reset */
    uint8_t* state;          /* [C] the BPSK modulator's state; 0 for RTTY */
    uint8_t* text;           /* [C][text_capacity] */
};

/* softdds_stepForSampleRate (softdds.c:26-32): the product in binary32, truncated to an integer */
inline uint32_t digi_dds_step(float freq, uint32_t samp_rate)
{
    uint64_t f = (uint64_t)(freq * 1024);
    f <<= 22;
    return (uint32_t)(f / samp_rate);
}

/* softdds_nextSample: the table entry of the accumulator as it is, then the step */
DIGI_HD int16_t digi_dds_next(const int16_t* sine, uint32_t& acc, uint32_t step)
{
    const int16_t v = sine[(acc >> 22) % 1024u];
    acc += step;
    return v;
}

/* One channel's end of the queue, in registers over a call */
struct DigiQueue
{
    const uint8_t* text;
    uint32_t capacity;
    uint32_t put, consumed, txoff_at;

    DIGI_HD void load(const DigiModArena& a, int32_t c)
    {
        text = a.text + (size_t)c * a.text_capacity;
        capacity = (uint32_t)a.text_capacity;
        put = a.put[c];
        consumed = a.consumed[c];
        txoff_at = a.txoff_at[c];
    }

    DIGI_HD void store(const DigiModArena& a, int32_t c) const
    {
        a.consumed[c] = consumed;
        a.txoff_at[c] = txoff_at;
    }

    /* DigiModes_TxBufferHasData */
    DIGI_HD bool has_data() const { return put != consumed; }

    /* DigiModes_TxBufferRemove on a queue that has data: the only read of a text byte */
    DIGI_HD uint8_t remove()
    {
        const uint8_t ch = text[consumed % capacity];
        ++consumed;
        return ch;
    }

    /* RadioManagement_Request_TxOff in sample `t` since reset; the first request is kept */
    DIGI_HD void request_txoff(uint32_t t)
    {
        if (txoff_at == DIGI_NO_TXOFF) txoff_at = t;
    }
};

#endif
