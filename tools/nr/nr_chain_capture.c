/*
 * Fixture recorder for the noise reduction and blanker inside the receive chain
 * (tests/golden/nrchain_*.npz).
 *
 * One capture object linked with the reference harness and its own main (nr_chain.mk, target
 * nr_chain), the harness' audio-driver translation unit compiled with is_dsp_nb_active changed to
 * NrChain_enter, the reference's audio_nr.c with it changed to NrChain_nb_active, and
 * -Wl,--wrap=arm_scale_f32,--wrap=UiDriver_Callback_AudioISR,--wrap=Rtty_Demodulator_ProcessSample:
 *
 *   NrChain_enter        the driver asks it once per 32-frame block, in the condition right in front of
 *                        AudioDriver_RxProcessorNoiseReduction(blockSizeDecim, a_buffer[0])
 *                        (audio_driver.c:2501): a_buffer[0] holds the block that enters, which is logged
 *                        when the answer (or DSP NR) lets it enter
 *   arm_scale_f32        the post-AGC scale of a_buffer[0] (audio_driver.c:2524) is the first thing
 *                        after the stage: its source is the block that left, which is logged.  With the
 *                        2:1 decimation the stage itself scales the same buffer once before
 *                        (audio_driver.c:2426), which is passed over
 *   UiDriver_Callback_AudioISR   the end of AudioDriver_I2SCallback: AudioNr_HandleNoiseReduction runs
 *                        once after every 32-frame block, a main loop that never falls behind
 *   Rtty_Demodulator_ProcessSample   the sample handed to the modem (mode=6 with NRC_RTTY=1)
 *
 * A constructor sets what the harness' main leaves alone, from the environment:
 *
 *   NRC_NB_SETTING       ts.dsp.nb_setting (0: no blanker); DSP NR itself is the harness' dsp=1
 *   NRC_STRENGTH         ts.dsp.nr_strength, from which AudioDriver_SetProcessingChain sets alpha
 *   NRC_ASNR NRC_WIDTH NRC_THRESHOLD   NR2.asnr, NR2.width, NR2.power_threshold_int, set before the
 *                        first block (NR_Init, which the driver's init calls, sets its own first)
 *   NRC_RTTY             1: ts.digital_mode = RTTY with the default rtty_ctrl_config
 *   NRC_IN_LOG NRC_OUT_LOG NRC_TAP_LOG   files: float32, 8 per block
 *   NRC_INFO_LOG         file: "width offset", FilterInfo[ts.filters_p->id].width and ts.filters_p->offset as
 *                        the stage finds them at its first block (what a host states in uhsdr_nr_config)
 *
 * AudioNr_RunNoiseReduction reads the Cortex-M DWT counter at 0xE0001004 for its profiling; the page is
 * mapped as plain memory here, as in nr_stream.c.  Nothing of this program or its output other than
 * the recorded data is committed.
 */
#include "uhsdr_board.h"
#include "audio_driver.h"
#include "audio_nr.h"
#include "audio_filter.h"
#include "radio_management.h"
#include "rtty.h"
#include <stdio.h>
#include <stdlib.h>
#include <sys/mman.h>

extern __IO TransceiverState ts;
extern AudioDriverBuffer adb;
bool is_dsp_nr(void);
void __real_arm_scale_f32(float32_t* pSrc, float32_t scale, float32_t* pDst, uint32_t blockSize);
void __real_UiDriver_Callback_AudioISR(void);
void __real_Rtty_Demodulator_ProcessSample(float32_t sample);

static FILE *in_log, *out_log, *tap_log;
static int prepared, inside, scaled;

static int env_int(const char* name, int dflt)
{
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

static FILE* env_file(const char* name)
{
    const char* v = getenv(name);
    FILE* f = v ? fopen(v, "wb") : NULL;
    if (v && !f) { perror(v); exit(1); }
    return f;
}

__attribute__((constructor)) static void capture_setup(void)
{
    if (mmap((void*)0xE0001000ul, 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED, -1, 0) == MAP_FAILED)
    { perror("mmap of the DWT page"); exit(1); }
    ts.dsp.nb_setting = env_int("NRC_NB_SETTING", 0);
    ts.dsp.nr_strength = env_int("NRC_STRENGTH", 50);
    if (env_int("NRC_RTTY", 0))
    {
        ts.digital_mode = DigitalMode_RTTY;
        rtty_ctrl_config.shift_idx = 1;
        rtty_ctrl_config.speed_idx = 0;
        rtty_ctrl_config.stopbits_idx = 1;
        rtty_ctrl_config.atc_disable = false;
    }
    in_log = env_file("NRC_IN_LOG");
    out_log = env_file("NRC_OUT_LOG");
    tap_log = env_file("NRC_TAP_LOG");
}

__attribute__((destructor)) static void capture_close(void)
{
    if (in_log) fclose(in_log);
    if (out_log) fclose(out_log);
    if (tap_log) fclose(tap_log);
}

/* is_dsp_nb_active as audio_nr.c asks it (ui_driver.c:405-408, the blanker's menu bit left out) */
bool NrChain_nb_active(void) { return ts.dsp.nb_setting > 0; }

/* is_dsp_nb_active as the driver asks it, in front of the stage */
bool NrChain_enter(void)
{
    const bool nb = NrChain_nb_active();
    if (!nb && !is_dsp_nr()) return nb;
    if (!prepared)
    {
        prepared = 1;
        AudioNr_Prepare();
        NR2.asnr = (int16_t)env_int("NRC_ASNR", 30);
        NR2.width = (int16_t)env_int("NRC_WIDTH", 4);
        NR2.power_threshold_int = (int16_t)env_int("NRC_THRESHOLD", 40);
        FILE* info = env_file("NRC_INFO_LOG");
        if (info)
        {
            fprintf(info, "%u %u\n", (unsigned)FilterInfo[ts.filters_p->id].width, (unsigned)ts.filters_p->offset);
            fclose(info);
        }
    }
    if (in_log) fwrite(adb.a_buffer[0], sizeof(float32_t), 8, in_log);
    inside = 1;
    scaled = 0;
    return nb;
}

void __wrap_arm_scale_f32(float32_t* pSrc, float32_t scale, float32_t* pDst, uint32_t blockSize)
{
    if (inside && pSrc == adb.a_buffer[0] && pDst == pSrc && blockSize == 8)
    {
        if (nr_params.NR_decimation_active && !scaled) scaled = 1;      /* the interpolator's factor 2 */
        else
        {
            if (out_log) fwrite(pSrc, sizeof(float32_t), 8, out_log);
            inside = 0;
        }
    }
    __real_arm_scale_f32(pSrc, scale, pDst, blockSize);
}

void __wrap_UiDriver_Callback_AudioISR(void)
{
    __real_UiDriver_Callback_AudioISR();
    if (prepared) AudioNr_HandleNoiseReduction();
}

void __wrap_Rtty_Demodulator_ProcessSample(float32_t sample)
{
    if (tap_log) fwrite(&sample, sizeof sample, 1, tap_log);
    __real_Rtty_Demodulator_ProcessSample(sample);
}
