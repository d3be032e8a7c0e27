/*
 * Fixture recorder for the signal meter (tests/golden/meter_*.npz), second translation unit: the
 * reference's ui_driver.c, included where it lies, for RadioManagement_HandleIqGainAndSMeter and
 * the static UiDriver_HandleSMeter, and the program.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them (meter.mk),
 * without the harness' main, and with meter_spectrum_tu.c.  ui_driver.c's forward declarations say
 * ulong and ushort, which the firmware has as 32 and 16 bits, so both are defined after the
 * headers.  The LCD calls the three functions reach and the codec-gain servo are empty here; what
 * the link leaves unresolved beyond them is never called (meter.mk).  Nothing of this program or
 * its output other than the recorded data is committed.
 *
 *   meter_driver run <case.bin> <out.bin>
 *       case.bin: int32 fft_iq_len, magnify, iq_freq_mode, dmod_mode, filter_path, sam_sideband,
 *                 cw_lsb, digi_lsb, bpsk, cw_sidetone_freq, dbm_constant, attack_alpha, decay_alpha,
 *                 snap_enable, tune_old, frames; then per frame int32 cw_signal and fft_iq_len / 2
 *                 floats of sd.FFT_MagData
 *       out.bin:  per frame float sm.dbm_cur, sm.dbmhz_cur, sm.dbm, sm.dbmhz, int32 sm.s_count,
 *                 uint32 ads.snap_carrier_freq; then int32 Lbin, Ubin, posbin of the last frame
 *   meter_driver tables <out.bin>
 *       S_Meter_Cal_dbm (33 floats), then per filter path uint16 FilterInfo[id].width and offset
 *
 * One process per channel: the averages, freq_old and the tune helper's state are statics.
 */
#include <sys/types.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <malloc.h>
#include "uhsdr_board.h"
#include "arm_math.h"
#undef __DSB
#define __DSB() ((void)0)
/* every header with a ulong in a structure first, so that the structures keep the layout the other
   objects have; only ui_driver.c's own text then reads the two names as the firmware's widths */
#include "audio_driver.h"
#include "radio_management.h"
#include "ui_spectrum.h"
#include "ui_rotary.h"
#include "ui_lcd_hy28.h"
#include "osc_interface.h"
#include "softdds.h"
#include "cw_decoder.h"
#define ulong uint32_t
#define ushort uint16_t
#include "ui_driver.c"

extern int MeterRec_bins[3];
void MeterRec_CalculateDBm(void);

DialFrequency df;
void RadioManagement_HandleRxIQSignalCodecGain(void) {}
/* the drawing the three functions reach: SNAP's tune helper, the S-meter's bar and the dBm text */
void UiLcdHy28_DrawStraightLine(uint16_t x, uint16_t y, uint16_t length, uint8_t direction, uint16_t color) {}
void UiLcdHy28_DrawStraightLineDouble(uint16_t x, uint16_t y, uint16_t length, uint8_t direction, uint16_t color) {}
void UiLcdHy28_DrawStraightLineTriple(uint16_t x, uint16_t y, uint16_t length, uint8_t direction, uint16_t color) {}
void UiLcdHy28_DrawFullRect(uint16_t x, uint16_t y, uint16_t height, uint16_t width, uint16_t color) {}
void UiLcdHy28_DrawEmptyRect(uint16_t x, uint16_t y, uint16_t height, uint16_t width, uint16_t color) {}
uint16_t UiLcdHy28_PrintText(uint16_t x, uint16_t y, const char* str, const uint32_t color, const uint32_t bk, uint8_t font) { return x; }
uint16_t UiLcdHy28_PrintTextRight(uint16_t x, uint16_t y, const char* str, const uint32_t color, const uint32_t bk, uint8_t font) { return x; }
uint16_t UiLcdHy28_PrintTextCentered(const uint16_t x, const uint16_t y, const uint16_t w, const char* txt, uint32_t fg, uint32_t bg, uint8_t font) { return x; }
uint16_t UiLcdHy28_TextWidth(const char* str, uint8_t font) { return 0; }
uint16_t UiLcdHy28_TextHeight(uint8_t font) { return 0; }
void UiMenu_MapColors(uint32_t color, char* options, volatile uint32_t* clr_ptr) { if (clr_ptr) *clr_ptr = 0; }

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "tables"))
    {
        FILE* o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 1; }
        fwrite(S_Meter_Cal_dbm, sizeof(float), S_Meter_Cal_Size, o);
        for (int p = 0; p < AUDIO_FILTER_PATH_NUM; p++)
        {
            const uint16_t w[2] = { FilterInfo[FilterPathInfo[p].id].width, FilterPathInfo[p].offset };
            fwrite(w, sizeof(uint16_t), 2, o);
        }
        fclose(o);
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "run"))
    {
        fprintf(stderr, "usage: meter_driver run <case.bin> <out.bin> | tables <out.bin>\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    int32_t h[16];
    if (fread(h, 4, 16, f) != 16) { fprintf(stderr, "short head\n"); return 1; }
    static LcdLayout layout;
    ts.Layout = &layout;
    ts.txrx_mode = TRX_MODE_RX;
    sd.fft_iq_len = h[0];
    sd.spec_len = h[0] / 2;
    sd.magnify = h[1];
    ts.iq_freq_mode = h[2];
    ts.dmod_mode = h[3];
    ts.filters_p = &FilterPathInfo[h[4]];
    ads.sam_sideband = h[5];
    ts.cw_lsb = h[6];
    ts.digi_lsb = h[7];
    ts.digital_mode = h[8] ? DigitalMode_BPSK : DigitalMode_None;
    ts.cw_sidetone_freq = h[9];
    ts.dbm_constant = h[10];
    sm.config.alphaSplit.AttackAlpha = h[11];
    sm.config.alphaSplit.DecayAlpha = h[12];
    cw_decoder_config.snap_enable = h[13];
    df.tune_old = (uint32_t)h[14];
    const int frames = h[15], L = h[0] / 2;
    if (L < 1 || L > (int)(sizeof sd.FFT_MagData / sizeof sd.FFT_MagData[0])) { fprintf(stderr, "fft_iq_len %d\n", h[0]); return 1; }
    FILE* o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 1; }
    for (int k = 0; k < frames; k++)
    {
        int32_t cw = 0;
        float mag[1024];
        if (fread(&cw, 4, 1, f) != 1 || fread(mag, 4, L, f) != (size_t)L) { fprintf(stderr, "short frame %d\n", k); return 1; }
        for (int i = 0; i < L; i++) sd.FFT_MagData[i] = mag[i];
        ads.CW_signal = cw != 0;
        MeterRec_CalculateDBm();
        RadioManagement_HandleIqGainAndSMeter();
        UiDriver_HandleSMeter();
        const float v[4] = { sm.dbm_cur, sm.dbmhz_cur, sm.dbm, sm.dbmhz };
        const int32_t s = (int32_t)sm.s_count;
        const uint32_t snap = (uint32_t)ads.snap_carrier_freq;
        fwrite(v, 4, 4, o);
        fwrite(&s, 4, 1, o);
        fwrite(&snap, 4, 1, o);
    }
    fwrite(MeterRec_bins, 4, 3, o);
    fclose(o);
    fclose(f);
    return 0;
}
