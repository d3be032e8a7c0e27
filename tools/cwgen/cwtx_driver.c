/*
 * Fixture recorder for the CW transmit chain (tests/golden/cwgen_chain_*.npz).
 *
 * One capture object linked with the reference harness and its own main (cwgen.mk, target
 * cwtx_driver).  The harness' empty key-line, text-ring, TX-request and text-output hooks and the
 * reference's CwGen_Process and softdds_runIQ are re-routed here with -Wl,--wrap; a constructor sets
 * the keyer's settings and fills the ring before the harness' main configures the rest:
 *
 *   CWTX_MODE, CWTX_SPEED, CWTX_WEIGHT, CWTX_REVERSE, CWTX_RXDELAY, CWTX_SIDETONE   ts.cw_*
 *   CWTX_LSB       ts.cw_lsb
 *   CWTX_CAP       the ring's capacity (one slot stays free)
 *   CWTX_TEXT      hex bytes put into the ring before the first call
 *   CWTX_KEYS      file: one byte per 32-frame call, bit 0 the DIT line, bit 1 the DAH/PTT line
 *   CWTX_LOG       file: "consumed echo-as-hex" at exit
 *   CWTX_FLAGS     file: one byte per call: bit 0 the signal was active (CwGen_Process returned true,
 *                  or TUNE), bit 1 TX-on, bit 2 TX-off requested
 *
 * Run as the harness is, with tx=1 mode=<DEMOD_CW>: TxProcessor_Run takes its CW branch
 * (tx_processor.c:985-988).  in= is ignored by that branch.  CwGen_Init and the sidetone set-up run
 * before the first CwGen_Process, so TUNE (tune=t0:K:1) must begin after call 0.  A call in TUNE
 * does not reach CwGen_Process: it is counted by its softdds_runIQ, and its key byte is not looked at.
 * Nothing of this program or its output other than the recorded data is committed.
 */
#include "uhsdr_board.h"
#include "radio_management.h"
#include "audio_management.h"
#include "cw_gen.h"
#include "uhsdr_digi_buffer.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern __IO TransceiverState ts;
extern struct { uint32_t w[13]; } ps;      /* cw_gen.c's public state: thirteen 32-bit words */

static uint8_t *ring, *keys, *flag_log;
static long calls, key_count;
static int capacity = 128, head, tail, lines, before, inside, started, on;
static unsigned long consumed;
static unsigned flags;
static uint8_t echo[1 << 16];
static int echoed;

static int env_int(const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }

/* the harness' main sets keyer defaults of its own after the constructor: applied again before the first call */
static void cwtx_settings(void)
{
    ts.cw_keyer_mode = (uint8_t)env_int("CWTX_MODE", 0);
    ts.cw_keyer_speed = (uint8_t)env_int("CWTX_SPEED", 20);
    ts.cw_keyer_weight = (uint8_t)env_int("CWTX_WEIGHT", 100);
    ts.cw_paddle_reverse = (uint8_t)env_int("CWTX_REVERSE", 0);
    ts.cw_rx_delay = (uint8_t)env_int("CWTX_RXDELAY", 8);
    ts.cw_sidetone_freq = (uint32_t)env_int("CWTX_SIDETONE", 750);
    ts.cw_lsb = env_int("CWTX_LSB", 0);
    ts.cw_text_entry = false;
}

__attribute__((constructor)) static void cwtx_setup(void)
{
    if (!getenv("CWTX_MODE")) return;
    on = 1;
    cwtx_settings();
    capacity = env_int("CWTX_CAP", 128);
    ring = malloc((size_t)capacity);
    unsigned byte;
    for (const char* t = getenv("CWTX_TEXT"); t && sscanf(t, "%2x", &byte) == 1; t += 2)
    {
        const int next = (head + 1) % capacity;
        if (next == tail) break;
        ring[head] = (uint8_t)byte;
        head = next;
    }
    FILE* f = getenv("CWTX_KEYS") ? fopen(getenv("CWTX_KEYS"), "rb") : NULL;
    if (f)
    {
        fseek(f, 0, SEEK_END);
        key_count = ftell(f);
        fseek(f, 0, SEEK_SET);
        keys = malloc((size_t)key_count + 1);
        if (fread(keys, 1, (size_t)key_count, f) != (size_t)key_count) key_count = 0;
        fclose(f);
    }
    flag_log = calloc((size_t)key_count + 1, 1);
}

__attribute__((destructor)) static void cwtx_close(void)
{
    if (!on) return;
    FILE* f = getenv("CWTX_LOG") ? fopen(getenv("CWTX_LOG"), "w") : NULL;
    if (f)
    {
        fprintf(f, "%lu ", consumed);
        for (int k = 0; k < echoed; k++) fprintf(f, "%02x", echo[k]);
        fprintf(f, "\n");
        fclose(f);
    }
    f = getenv("CWTX_FLAGS") ? fopen(getenv("CWTX_FLAGS"), "wb") : NULL;
    if (f) { fwrite(flag_log, 1, (size_t)(calls < key_count ? calls : key_count), f); fclose(f); }
}

bool __wrap_Board_DitLinePressed(void) { return (lines & 1) != 0; }
bool __wrap_Board_PttDahLinePressed(void) { return (lines & 2) != 0; }
void __wrap_RadioManagement_Request_TxOn(void) { flags |= 2; }
void __wrap_RadioManagement_Request_TxOff(void) { flags |= 4; }
void __wrap_UiDriver_TextMsgPutChar(char ch) { if (echoed < (int)sizeof echo) echo[echoed++] = (uint8_t)ch; }

bool __wrap_DigiModes_TxBufferRemove(uint8_t* c_ptr, digi_buff_consumer_t consumer)
{
    if (consumer != CW || head == tail) return false;
    *c_ptr = ring[tail];
    tail = (tail + 1) % capacity;
    consumed++;
    return true;
}

int32_t __wrap_DigiModes_TxBufferPutChar(uint8_t c, digi_buff_consumer_t source)
{
    (void)source;
    __wrap_UiDriver_TextMsgPutChar((char)c);
    return 0;
}

void __wrap_DigiModes_TxBufferPutSign(const char* s, digi_buff_consumer_t source)
{
    __wrap_DigiModes_TxBufferPutChar('<', source);
    __wrap_DigiModes_TxBufferPutChar((uint8_t)s[0], source);
    __wrap_DigiModes_TxBufferPutChar((uint8_t)s[1], source);
    __wrap_DigiModes_TxBufferPutChar('>', source);
}

void DigiModes_TxBufferReset(void)
{
    consumed += (unsigned long)((head - tail + capacity) % capacity);
    tail = head;
}

static void count_call(unsigned f)
{
    if (calls < key_count) flag_log[calls] = (uint8_t)f;
    calls++;
}

void __real_softdds_runIQ(float32_t* i_buff, float32_t* q_buff, uint16_t size);
void __wrap_softdds_runIQ(float32_t* i_buff, float32_t* q_buff, uint16_t size)
{
    __real_softdds_runIQ(i_buff, q_buff, size);
    if (on && !inside) count_call(1);       /* TUNE */
}

bool __real_CwGen_Process(float32_t* i_buffer, float32_t* q_buffer, uint32_t size);
bool __wrap_CwGen_Process(float32_t* i_buffer, float32_t* q_buffer, uint32_t size)
{
    if (!on) return __real_CwGen_Process(i_buffer, q_buffer, size);
    if (!started)
    {
        started = 1;
        cwtx_settings();
        memset(&ps, 0, sizeof ps);      /* a fresh keyer, whatever the harness' set-up did in RX */
        CwGen_Init();
        AudioManagement_SetSidetoneForDemodMode(ts.dmod_mode, false);
    }
    lines = calls < key_count ? keys[calls] & 3 : 0;
    flags = 0;
    if (lines & ~before) CwGen_DitIRQ();
    before = lines;
    inside = 1;
    const bool active = __real_CwGen_Process(i_buffer, q_buffer, size);
    inside = 0;
    count_call(flags | (active ? 1u : 0u));
    return active;
}
