/*
 * Fixture recorder for the RTTY decoder inside the receive chain (tests/golden/rtty_chain_*.npz).
 *
 * One capture object linked with the reference harness and its own main (rtty.mk, target
 * rtty_chain), with -Wl,--wrap=Rtty_Demodulator_ProcessSample,--wrap=UiDriver_TextMsgPutChar.
 * A constructor puts the firmware into RTTY before the harness' main configures the rest:
 *
 *   RTTY_SHIFT RTTY_SPEED RTTY_STOPBITS RTTY_ATC_DISABLE    rtty_ctrl_config (indices)
 *   RTTY_TAP_LOG    file: every sample the chain hands the demodulator, float32
 *   RTTY_CHAR_LOG   file: "sample byte" per byte printed, sample = the index of the tap sample
 *
 * Run as the harness is, with mode=6 (DEMOD_DIGI) on a 12 ksps path.  Nothing of this program or
 * its output other than the recorded data is committed.
 */
#include "uhsdr_board.h"
#include "radio_management.h"
#include "rtty.h"
#include <stdio.h>
#include <stdlib.h>

extern __IO TransceiverState ts;
void __real_Rtty_Demodulator_ProcessSample(float32_t sample);

static FILE *tap_log, *char_log;
static long now = -1;

static int env_int(const char* name, int dflt)
{
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

__attribute__((constructor)) static void capture_setup(void)
{
    ts.digital_mode = DigitalMode_RTTY;
    rtty_ctrl_config.shift_idx = env_int("RTTY_SHIFT", 1);
    rtty_ctrl_config.speed_idx = env_int("RTTY_SPEED", 0);
    rtty_ctrl_config.stopbits_idx = env_int("RTTY_STOPBITS", 1);
    rtty_ctrl_config.atc_disable = env_int("RTTY_ATC_DISABLE", 0) != 0;
    if (getenv("RTTY_TAP_LOG")) tap_log = fopen(getenv("RTTY_TAP_LOG"), "wb");
    if (getenv("RTTY_CHAR_LOG")) char_log = fopen(getenv("RTTY_CHAR_LOG"), "w");
}

__attribute__((destructor)) static void capture_close(void)
{
    if (tap_log) fclose(tap_log);
    if (char_log) fclose(char_log);
}

void __wrap_Rtty_Demodulator_ProcessSample(float32_t sample)
{
    ++now;
    if (tap_log) fwrite(&sample, sizeof sample, 1, tap_log);
    __real_Rtty_Demodulator_ProcessSample(sample);
}

void __wrap_UiDriver_TextMsgPutChar(char ch)
{
    if (char_log) fprintf(char_log, "%ld %u\n", now, (unsigned)(unsigned char)ch);
}
