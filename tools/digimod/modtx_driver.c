/*
 * Fixture recorder for the DIGI transmit chain (tests/golden/digimod_chain_*.npz).
 *
 * One capture object linked with the reference harness, its own main and the reference's psk.c
 * (digimod.mk, target modtx_driver).  The harness' empty text-ring and TX-off hooks, its
 * Psk_Modulator_GenSample and RadioManagement_IsTxAtZeroIF are re-routed here with -Wl,--wrap; a
 * constructor puts the firmware into digital voice mode with RTTY or BPSK, initialises the
 * modulator and fills the ring before the harness' main configures the rest:
 *
 *   MODTX_KIND     rtty | psk        ts.dvmode = true, ts.digital_mode
 *   MODTX_SHIFT, MODTX_SPEED, MODTX_STOP   rtty_ctrl_config / psk_ctrl_config
 *   MODTX_LSB      ts.digi_lsb
 *   MODTX_CAP      the ring's capacity (one slot stays free)
 *   MODTX_TEXT     hex bytes put into the ring before the first call
 *   MODTX_LOG      file: "consumed txoff_at state" at exit
 *
 * Run as the harness is, with tx=1 mode=6 (DEMOD_DIGI): TxProcessor_Run takes its dvmode branch
 * (tx_processor.c:962-984).  in= is ignored by that branch.  Nothing of this program or its output
 * other than the recorded data is committed.
 */
#include "uhsdr_board.h"
#include "radio_management.h"
#include "rtty.h"
#include "psk.h"
#include "uhsdr_digi_buffer.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern __IO TransceiverState ts;
void Rtty_Modulator_StartTX(void);      /* rtty.c, not in rtty.h */

static uint8_t* ring;
static int capacity = 128, head, tail, psk;
static unsigned long consumed, now, txoff_at = 4294967295ul;

static int env_int(const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }

__attribute__((constructor)) static void modtx_setup(void)
{
    const char* kind = getenv("MODTX_KIND");
    if (!kind) return;
    psk = !strcmp(kind, "psk");
    ts.dvmode = true;
    ts.digital_mode = psk ? DigitalMode_BPSK : DigitalMode_RTTY;
    ts.digi_lsb = env_int("MODTX_LSB", 0);
    capacity = env_int("MODTX_CAP", 128);
    ring = malloc((size_t)capacity);
    if (psk)
    {
        psk_ctrl_config.speed_idx = env_int("MODTX_SPEED", 0);
        Psk_Modem_Init(48000);          /* the renamed one of psk.c */
        Psk_Modulator_PrepareTx();
    }
    else
    {
        /* Rtty_Modem_Init runs again in AudioDriver_Init with these; StartTX needs it to have run */
        rtty_ctrl_config.shift_idx = env_int("MODTX_SHIFT", 1);
        rtty_ctrl_config.speed_idx = env_int("MODTX_SPEED", 0);
        rtty_ctrl_config.stopbits_idx = env_int("MODTX_STOP", 1);
        Rtty_Modem_Init(48000);
        Rtty_Modulator_StartTX();
    }
    unsigned byte;
    for (const char* t = getenv("MODTX_TEXT"); t && sscanf(t, "%2x", &byte) == 1; t += 2)
    {
        const int next = (head + 1) % capacity;
        if (next == tail) break;
        ring[head] = (uint8_t)byte;
        head = next;
    }
}

__attribute__((destructor)) static void modtx_close(void)
{
    const char* log = getenv("MODTX_LOG");
    if (!log || !getenv("MODTX_KIND")) return;
    FILE* f = fopen(log, "w");
    if (f) { fprintf(f, "%lu %lu %d\n", consumed, txoff_at, psk ? (int)Psk_Modulator_GetState() : 0); fclose(f); }
}

/* the chain's call lands here; the name in the body is the renamed modulator of psk.c */
int16_t __wrap_Psk_Modulator_GenSample(void)
{
    const int16_t v = Psk_Modulator_GenSample();
    now++;
    return v;
}

uint8_t __wrap_DigiModes_TxBufferHasData(void) { return (uint8_t)(head != tail); }
uint8_t __wrap_DigiModes_TxBufferHasDataFor(digi_buff_consumer_t consumer) { (void)consumer; return (uint8_t)(head != tail); }

bool __wrap_DigiModes_TxBufferRemove(uint8_t* c_ptr, digi_buff_consumer_t consumer)
{
    (void)consumer;
    if (head == tail) return false;
    *c_ptr = ring[tail];
    tail = (tail + 1) % capacity;
    consumed++;
    return true;
}

/* the sample index of an RTTY request is not counted here (its GenSample is not wrapped): the
   chain fixtures record whether TX-off was requested, the stand-alone ones where */
void __wrap_RadioManagement_Request_TxOff(void)
{
    if (txoff_at == 4294967295ul) txoff_at = psk ? now : 0;
}

/* radio_management.c:587-605: RTTY and BPSK transmit at zero IF */
bool __wrap_RadioManagement_IsTxAtZeroIF(uint8_t dmod_mode, uint8_t digital_mode)
{
    (void)digital_mode;
    return dmod_mode == DEMOD_CW || dmod_mode == DEMOD_DIGI;
}
