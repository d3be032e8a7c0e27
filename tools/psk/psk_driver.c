/*
 * Fixture recorder for the BPSK decoder (tests/golden/psk_*.npz), stand-alone cases.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them and with its
 * psk.c (psk.mk), without the harness' main and with -Wl,--wrap=UiDriver_TextMsgPutChar, so the
 * characters the reference decoder prints arrive here.  Nothing of this program or its output other
 * than the recorded data is committed.
 *
 *   psk_driver <audio.f32> speed_idx
 *       feeds 12 ksps float audio sample by sample through Psk_Demodulator_ProcessSample and
 *       prints "sample byte" for every byte printed, with the index of the sample that emitted it
 *
 * The demodulator's statics never reset: one process per case.
 */
#include "uhsdr_board.h"
#include "psk.h"
#include <stdio.h>
#include <stdlib.h>

static long now;

void __wrap_UiDriver_TextMsgPutChar(char ch)
{
    printf("%ld %u\n", now, (unsigned)(unsigned char)ch);
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: psk_driver <audio.f32> speed_idx\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(float);
    fseek(f, 0, SEEK_SET);
    float* audio = malloc(sizeof(float) * (size_t)(n + 1));
    if (fread(audio, sizeof(float), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    psk_ctrl_config.speed_idx = atoi(argv[2]);
    Psk_Modem_Init(48000);

    for (now = 0; now < n; now++) Psk_Demodulator_ProcessSample(audio[now]);
    free(audio);
    return 0;
}
