/*
 * Fixture recorder for the spectral noise reduction (tests/golden/nr_*.npz), the frame stage alone.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them (nr.mk), without
 * the harness' main.  The reference's audio_nr.c is included below, where it lies, the way
 * oracle/ref/ref_audio_driver_tu.c includes audio_driver.c: spectral_noise_reduction_3 and its
 * buffers are private to that file.  Nothing of this program or its output other than the recorded
 * data is committed.
 *
 *   nr_driver tables <out.bin>
 *       SQRT_von_Hann_256 as the compiled reference holds it, 256 binary32
 *   nr_driver icfft <in.f32> <out.f32>
 *       arm_cfft_f32(&arm_cfft_sR_f32_len256, x, 1, 1) on every 512 floats of the input
 *   nr_driver frames <in.f32> <out.bin> alpha_bits asnr width threshold_int width_hz offset_hz rate [reset_frame]
 *       feeds 128-sample frames through spectral_noise_reduction_3 and writes per frame the 128
 *       output samples, Hk[128], NN, power_ratio and first_time (after the frame).  alpha_bits: the
 *       binary32 pattern of nr_params.alpha.  rate 6000: nr_params.NR_decimation_active.  Before
 *       frame reset_frame the noise reduction is restarted as a fresh one (first_time 1 and the
 *       carried overlap cleared; the other statics are rewritten by the start-up itself).
 *
 * arm_cfft_f32 calls arm_bitreversal_32, which the reference has as ARM assembly only: nr_bitrev.c.
 * The filter table audio_nr.c reads is nr_filter.c's (nr.mk renames it here), one entry whose
 * width the case sets.
 */
#include "audio_nr.c"
#include "audio_filter.h"
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void nr_set_filter_width(uint16_t width);

static float* read_floats(const char* path, long* n)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(1); }
    fseek(f, 0, SEEK_END);
    *n = ftell(f) / (long)sizeof(float);
    fseek(f, 0, SEEK_SET);
    float* x = malloc(sizeof(float) * (size_t)(*n + 1));
    if (fread(x, sizeof(float), (size_t)*n, f) != (size_t)*n) { fprintf(stderr, "short read\n"); exit(1); }
    fclose(f);
    return x;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "tables"))
    {
        FILE* o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 1; }
        fwrite(SQRT_von_Hann_256, sizeof(float), 256, o);
        fclose(o);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "icfft"))
    {
        long n;
        float* x = read_floats(argv[2], &n);
        for (long k = 0; k + 512 <= n; k += 512) arm_cfft_f32(&arm_cfft_sR_f32_len256, x + k, 1, 1);
        FILE* o = fopen(argv[3], "wb");
        if (!o) { perror(argv[3]); return 1; }
        fwrite(x, sizeof(float), (size_t)(n / 512 * 512), o);
        fclose(o);
        return 0;
    }
    if (argc < 11 || strcmp(argv[1], "frames"))
    {
        fprintf(stderr, "usage: nr_driver tables|icfft|frames ... (see the source)\n");
        return 2;
    }
    long n;
    float* x = read_floats(argv[2], &n);
    FILE* o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 1; }
    const long reset_frame = argc > 11 ? atol(argv[11]) : -1;

    static char path_mem[sizeof(FilterPathDescriptor)];
    FilterPathDescriptor* path = (FilterPathDescriptor*)path_mem;
    const uint16_t offset = (uint16_t)atoi(argv[9]);
    memcpy((char*)path + offsetof(FilterPathDescriptor, offset), &offset, sizeof offset);
    ts.filters_p = path;                           /* id 0 */
    nr_set_filter_width((uint16_t)atoi(argv[8]));

    NR_Init();
    const uint32_t alpha_bits = (uint32_t)strtoul(argv[4], NULL, 0);
    memcpy(&nr_params.alpha, &alpha_bits, 4);
    NR2.asnr = (int16_t)atoi(argv[5]);
    NR2.width = (int16_t)atoi(argv[6]);
    NR2.power_threshold_int = (int16_t)atoi(argv[7]);
    nr_params.NR_decimation_active = atoi(argv[10]) == 6000;

    for (long f = 0; (f + 1) * 128 <= n; f++)
    {
        if (f == reset_frame)
        {
            nr_params.first_time = 1;
            memset(NR.last_iFFT_result, 0, sizeof NR.last_iFFT_result);
        }
        float frame[128];
        memcpy(frame, x + f * 128, sizeof frame);
        spectral_noise_reduction_3(frame);
        const int32_t nn = NR2.NN, ft = nr_params.first_time;
        fwrite(frame, sizeof(float), 128, o);
        fwrite(NR2.Hk, sizeof(float), 128, o);
        fwrite(&nn, 4, 1, o);
        fwrite(&NR2.power_ratio, 4, 1, o);
        fwrite(&ft, 4, 1, o);
    }
    fclose(o);
    free(x);
    return 0;
}
