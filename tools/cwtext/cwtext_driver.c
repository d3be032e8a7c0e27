/*
 * Fixture recorder for the CW decoder back end (tests/golden/cwtext_*.npz).
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them (cwtext.mk),
 * without the harness' main and with -Wl,--wrap=UiDriver_TextMsgPutChar, so the characters the
 * reference decoder prints arrive here.  Nothing of this program or its output other than the
 * recorded data is committed.
 *
 *   cwtext_driver run <audio.f32> blocksize thresh noisecancel spikecancel sidetone
 *       feeds 12 ksps float audio, 8 samples at a time, through CwDecode_RxProcessor; after each
 *       completed block prints "state speed c c c ..." (ads.CW_signal, cw_decoder_config.speed,
 *       the bytes printed during that block)
 *   cwtext_driver table
 *       prints "code char" of CwGen_CharacterIdFunc for every code of 0 to 9 elements
 */
#include "uhsdr_board.h"
#include "audio_driver.h"
#include "cw_decoder.h"
#include "cw_gen.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned char emitted[256];
static int n_emitted;

void __wrap_UiDriver_TextMsgPutChar(char ch)
{
    if (n_emitted < (int)sizeof emitted) emitted[n_emitted++] = (unsigned char)ch;
}

static int table(void)
{
    for (int n = 0; n <= 9; n++)
        for (unsigned m = 0; m < (1u << n); m++)
        {
            uint32_t code = 0;
            for (int k = n - 1; k >= 0; k--) code = code * 4 + (((m >> k) & 1u) ? 3 : 2);
            printf("%u %u\n", (unsigned)code, (unsigned)CwGen_CharacterIdFunc(code));
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "table")) return table();
    if (argc != 8 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: see the head of cwtext_driver.c\n"); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(float);
    fseek(f, 0, SEEK_SET);
    float* audio = malloc(sizeof(float) * (size_t)(n + 8));
    if (fread(audio, sizeof(float), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    ts.txrx_mode = TRX_MODE_RX;
    ts.cw_decoder_enable = 1;
    ts.dmod_mode = DEMOD_CW;
    ts.cw_sidetone_freq = atoi(argv[7]);
    cw_decoder_config.blocksize = atoi(argv[3]);
    cw_decoder_config.thresh = atoi(argv[4]);
    cw_decoder_config.noisecancel_enable = atoi(argv[5]);
    cw_decoder_config.spikecancel = atoi(argv[6]);
    CwDecode_Filter_Set();

    int count = 0;      /* CwDecode_RxProcessor's sample_counter */
    for (long i = 0; i + 8 <= n; i += 8)
    {
        CwDecode_RxProcessor(audio + i, 8);
        count += 8;
        if (count >= cw_decoder_config.blocksize)
        {
            count = 0;
            printf("%d %u", ads.CW_signal ? 1 : 0, (unsigned)cw_decoder_config.speed);
            for (int k = 0; k < n_emitted; k++) printf(" %u", (unsigned)emitted[k]);
            printf("\n");
            n_emitted = 0;
        }
    }
    free(audio);
    return 0;
}
