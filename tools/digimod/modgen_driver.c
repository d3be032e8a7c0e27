/*
 * Fixture recorder for the RTTY and BPSK modulators (tests/golden/digimod_*.npz), stand-alone cases.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them and with its
 * psk.c (digimod.mk), without the harness' main.  The harness' empty digital-mode hooks are
 * re-routed with -Wl,--wrap to the text ring and the TX-off log below, so the reference's
 * Rtty_Modulator_GenSample / Psk_Modulator_GenSample run alone against a queue this program
 * fills.  Nothing of this program or its output other than the recorded data is committed.
 *
 *   modgen_driver rtty shift_idx speed_idx stopbits_idx capacity <ops.txt> <out.s16>
 *   modgen_driver psk speed_idx capacity <ops.txt> <out.s16>
 *
 * The modem is initialised for 48 ksps and StartTX / PrepareTx is called once, then the ops run, one per line:
 *   put <hex bytes>   append to the ring what fits; prints "accepted <k>"
 *   gen <n>           n calls of GenSample, the int16 results appended to <out.s16>; prints
 *                     "gen <consumed> <txoff_at> <state>": characters removed so far, the index of
 *                     the first sample that requested TX-off (4294967295: none), the BPSK state
 *   start             Rtty_Modulator_StartTX / Psk_Modulator_PrepareTx
 *
 * The ring is the firmware's (uhsdr_digi_buffer.c) with the capacity an argument: one slot stays
 * free, no consumer tag.  The modulators' statics never reset: one process per case.
 */
#include "uhsdr_board.h"
#include "rtty.h"
#include "psk.h"
#include "uhsdr_digi_buffer.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void Rtty_Modulator_StartTX(void);      /* rtty.c, not in rtty.h */

static uint8_t* ring;
static int capacity, head, tail;
static unsigned long consumed, now, txoff_at = 4294967295ul;

uint8_t __wrap_DigiModes_TxBufferHasData(void)
{
    const int len = head - tail;
    return (uint8_t)((len < 0 ? len + capacity : len) != 0);
}

uint8_t __wrap_DigiModes_TxBufferHasDataFor(digi_buff_consumer_t consumer) { (void)consumer; return __wrap_DigiModes_TxBufferHasData(); }

bool __wrap_DigiModes_TxBufferRemove(uint8_t* c_ptr, digi_buff_consumer_t consumer)
{
    (void)consumer;
    if (head == tail) return false;
    *c_ptr = ring[tail];
    tail = (tail + 1) % capacity;
    consumed++;
    return true;
}

void __wrap_RadioManagement_Request_TxOff(void)
{
    if (txoff_at == 4294967295ul) txoff_at = now;
}

static int put_char(uint8_t c)
{
    const int next = (head + 1) % capacity;
    if (next == tail) return 0;
    ring[head] = c;
    head = next;
    return 1;
}

int main(int argc, char** argv)
{
    int psk = 0, a = 2;
    if (argc == 8 && !strcmp(argv[1], "rtty"))
    {
        rtty_ctrl_config.shift_idx = atoi(argv[a++]);
        rtty_ctrl_config.speed_idx = atoi(argv[a++]);
        rtty_ctrl_config.stopbits_idx = atoi(argv[a++]);
    }
    else if (argc == 6 && !strcmp(argv[1], "psk"))
    {
        psk = 1;
        psk_ctrl_config.speed_idx = atoi(argv[a++]);
    }
    else { fprintf(stderr, "usage: see the head of modgen_driver.c\n"); return 2; }
    capacity = atoi(argv[a++]);
    ring = malloc((size_t)capacity);
    FILE* ops = fopen(argv[a++], "r");
    FILE* out = fopen(argv[a++], "wb");
    if (!ops || !out || !ring) { perror("modgen_driver"); return 1; }

    if (psk) { Psk_Modem_Init(48000); Psk_Modulator_PrepareTx(); }
    else { Rtty_Modem_Init(48000); Rtty_Modulator_StartTX(); }

    static char line[1 << 16];
    while (fgets(line, sizeof line, ops))
    {
        char* arg = strchr(line, ' ');
        if (arg) *arg++ = 0;
        line[strcspn(line, "\n")] = 0;
        if (!strcmp(line, "put"))
        {
            int k = 0;
            unsigned byte;
            for (; arg && sscanf(arg, "%2x", &byte) == 1; arg += 2) k += put_char((uint8_t)byte);
            printf("accepted %d\n", k);
        }
        else if (!strcmp(line, "gen"))
        {
            for (long n = atol(arg); n > 0; n--, now++)
            {
                const int16_t v = psk ? Psk_Modulator_GenSample() : Rtty_Modulator_GenSample();
                fwrite(&v, sizeof v, 1, out);
            }
            printf("gen %lu %lu %d\n", consumed, txoff_at, psk ? (int)Psk_Modulator_GetState() : 0);
        }
        else if (!strcmp(line, "start"))
        {
            if (psk) Psk_Modulator_PrepareTx(); else Rtty_Modulator_StartTX();
        }
        else if (line[0]) { fprintf(stderr, "unknown op %s\n", line); return 2; }
    }
    fclose(out);
    return 0;
}
