/*
 * Fixture recorder for the 12 ksps stream with the noise blanker (tests/golden/nb_stream_*.npz):
 * tools/nr/nr_stream.c with the two settings, the blanker's and whether the noise reduction runs.
 *
 * A translation unit that includes the reference's audio_driver.c where it lies
 * (AudioDriver_RxProcessorNoiseReduction, its decimator and interpolator are private to that file),
 * linked with the reference's audio_nr.c compiled with is_dsp_nb_active renamed to NbRec_active
 * (nb.mk), which is defined here.  Nothing of this program or its output other than the recorded
 * data is committed.
 *
 *   nb_stream run <in.f32> <out.f32> alpha_bits asnr width threshold_int width_hz offset_hz nb_setting nr_on
 *       feeds 12 ksps audio in the firmware's blocks of 8 samples through
 *       AudioDriver_RxProcessorNoiseReduction and runs AudioNr_HandleNoiseReduction once after every
 *       block.  nr_on 0: the blanker alone (DSP_NR_ENABLE clear), 1: the blanker, then the noise
 *       reduction.
 *
 * The DWT page is mapped as in nr_stream.c: the noise reduction's profiling reads it.
 */
#include "uhsdr_board_config.h"
#undef USE_PENDSV_FOR_HIGHPRIO_TASKS
#include "audio_driver.c"
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>

void nr_set_filter_width(uint16_t width);

bool NbRec_active(void) { return ts.dsp.nb_setting > 0; }

int main(int argc, char** argv)
{
    if (argc != 12 || strcmp(argv[1], "run"))
    {
        fprintf(stderr, "usage: nb_stream run ... (see the source)\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(float);
    fseek(f, 0, SEEK_SET);
    float* x = malloc(sizeof(float) * (size_t)(n + 8));
    if (fread(x, sizeof(float), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);

    static char path_mem[sizeof(FilterPathDescriptor)];
    FilterPathDescriptor* path = (FilterPathDescriptor*)path_mem;
    const uint16_t offset = (uint16_t)atoi(argv[9]);
    memcpy((char*)path + offsetof(FilterPathDescriptor, offset), &offset, sizeof offset);
    ts.filters_p = path;                           /* id 0 */
    nr_set_filter_width((uint16_t)atoi(argv[8]));

    if (mmap((void*)0xE0001000ul, 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED, -1, 0) == MAP_FAILED)
    { perror("mmap of the DWT page"); return 1; }
    if (atoi(argv[11])) ts.dsp.active |= DSP_NR_ENABLE;
    else ts.dsp.active &= ~DSP_NR_ENABLE;
    ts.dsp.nb_setting = atoi(argv[10]);
    NR_Init();
    AudioNr_Prepare();
    const uint32_t alpha_bits = (uint32_t)strtoul(argv[4], NULL, 0);
    memcpy(&nr_params.alpha, &alpha_bits, 4);
    NR2.asnr = (int16_t)atoi(argv[5]);
    NR2.width = (int16_t)atoi(argv[6]);
    NR2.power_threshold_int = (int16_t)atoi(argv[7]);
    /* the two instances as the driver's init sets them up (audio_driver.c:649-653) */
    arm_fir_decimate_init_f32(&DECIMATE_NR, 4, 2, NR_decimate_coeffs, decimNRState, FIR_RXAUDIO_BLOCK_SIZE);
    arm_fir_interpolate_init_f32(&INTERPOLATE_NR, 2, NR_INTERPOLATE_NO_TAPS, NR_interpolate_coeffs, interplNRState, FIR_RXAUDIO_BLOCK_SIZE);

    FILE* o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 1; }
    for (long b = 0; b + 8 <= n; b += 8)
    {
        float block[8];
        memcpy(block, x + b, sizeof block);
        AudioDriver_RxProcessorNoiseReduction(8, block);
        fwrite(block, sizeof(float), 8, o);
        AudioNr_HandleNoiseReduction();
    }
    fclose(o);
    free(x);
    return 0;
}
