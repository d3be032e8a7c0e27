/*
 * Fixture recorder for the BPSK decoder inside the receive chain (tests/golden/psk_chain_*.npz).
 *
 * One capture object linked with the reference harness, its own main and the reference's psk.c
 * (psk.mk, target psk_chain), with -Wl,--wrap=Psk_Demodulator_ProcessSample,
 * --wrap=UiDriver_TextMsgPutChar.  The harness has an empty Psk_Demodulator_ProcessSample; psk.c is
 * compiled with the function renamed (psk.mk), and the wrapper below, which the chain's call
 * reaches, forwards to it.  A constructor puts the firmware into BPSK before the harness' main
 * configures the rest:
 *
 *   PSK_SPEED      psk_ctrl_config.speed_idx
 *   PSK_TAP_LOG    file: every sample the chain hands the demodulator, float32
 *   PSK_CHAR_LOG   file: "sample byte" per byte printed, sample = the index of the tap sample
 *
 * Run as the harness is, with mode=6 (DEMOD_DIGI) on a 12 ksps path.  Nothing of this program or
 * its output other than the recorded data is committed.
 */
#include "uhsdr_board.h"
#include "radio_management.h"
#include "psk.h"
#include <stdio.h>
#include <stdlib.h>

extern __IO TransceiverState ts;

static FILE *tap_log, *char_log;
static long now = -1;

__attribute__((constructor)) static void capture_setup(void)
{
    ts.digital_mode = DigitalMode_BPSK;
    psk_ctrl_config.speed_idx = getenv("PSK_SPEED") ? atoi(getenv("PSK_SPEED")) : 0;
    Psk_Modem_Init(48000);       /* the renamed one of psk.c */
    if (getenv("PSK_TAP_LOG")) tap_log = fopen(getenv("PSK_TAP_LOG"), "wb");
    if (getenv("PSK_CHAR_LOG")) char_log = fopen(getenv("PSK_CHAR_LOG"), "w");
}

__attribute__((destructor)) static void capture_close(void)
{
    if (tap_log) fclose(tap_log);
    if (char_log) fclose(char_log);
}

/* the chain's call lands here; the name in the body is the renamed decoder of psk.c */
void __wrap_Psk_Demodulator_ProcessSample(float32_t sample)
{
    ++now;
    if (tap_log) fwrite(&sample, sizeof sample, 1, tap_log);
    Psk_Demodulator_ProcessSample(sample);
}

void __wrap_UiDriver_TextMsgPutChar(char ch)
{
    if (char_log) fprintf(char_log, "%ld %u\n", now, (unsigned)(unsigned char)ch);
}
