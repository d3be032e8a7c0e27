/*
 * Fixture recorder for the noise blanker (tests/golden/nb_*.npz), the frame stage alone.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them (nr.mk, nb.mk),
 * without the harness' main.  The reference's audio_nr.c is included below, where it lies, the way
 * tools/nr/nr_driver.c does: AudioNr_RunNoiseReduction and alt_noise_blanking are private to that
 * file.  Nothing of this program or its output other than the recorded data is committed.
 *
 *   nb_driver frames <in.f32> <out.f32> nb_setting
 *       feeds 128-sample frames through AudioNr_RunNoiseReduction with the blanker on and the noise
 *       reduction off, the firmware's own call of alt_noise_blanking (three arguments to a
 *       definition of four), and writes the 128 output samples of every frame
 *
 * is_dsp_nb_active is compiled as NbRec_active (nb.mk), defined here; the harness' is_dsp_nr reads
 * ts.dsp.active, where DSP_NR_ENABLE stays clear.
 */
#include "audio_nr.c"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

bool NbRec_active(void) { return ts.dsp.nb_setting > 0; }

int main(int argc, char** argv)
{
    if (argc != 5 || strcmp(argv[1], "frames"))
    {
        fprintf(stderr, "usage: nb_driver frames <in.f32> <out.f32> nb_setting\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(float);
    fseek(f, 0, SEEK_SET);
    float* x = malloc(sizeof(float) * (size_t)(n + 1));
    if (fread(x, sizeof(float), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);
    FILE* o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 1; }
    ts.dsp.active &= ~DSP_NR_ENABLE;
    ts.dsp.nb_setting = atoi(argv[4]);
    for (long k = 0; (k + 1) * 128 <= n; k++)
    {
        float frame[128], result[128];
        memcpy(frame, x + k * 128, sizeof frame);
        AudioNr_RunNoiseReduction(frame, result);
        fwrite(result, sizeof(float), 128, o);
    }
    fclose(o);
    free(x);
    return 0;
}
