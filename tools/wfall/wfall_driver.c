/*
 * Fixture recorder for the waterfall image (tests/golden/wfall_*.npz), second translation unit: the
 * program, and the LCD and menu calls UiSpectrum_DrawWaterfall reaches.  UiLcdHy28_BulkPixel_PutBuffer
 * appends each row it is handed to the frame's record, so the record holds the rows in the order the
 * firmware sends them to the panel; UiMenu_MapColors hands back the case's marker colour; the dial
 * frequencies are the case's.
 *
 * Linked like display_driver (wfall.mk): the reference firmware's objects, wfall_spectrum_tu.c, and
 * the harness with its main renamed, whose spectrum run `spec` below drives.  Nothing of this program
 * or its output other than the recorded data is committed.
 *
 *   wfall_driver run <case.bin> <out.bin>
 *       case.bin: int32 width, height, color_scheme, vert_step_size, marker_colour, magnify,
 *                 iq_freq_mode, dmod_mode, digital_mode (0 none, 1 RTTY, 2 BPSK), cw_lsb, digi_lsb,
 *                 cw_sidetone_freq, rtty_shift_idx, psk_speed_idx, tx_minus_rx_hz, frames; then per
 *                 frame uint32 sd.FFT_frequency and width bytes.  A byte b goes to sd.FFT_Samples as
 *                 the float b below 64 and b - 256 from 64 on (the negative sample whose conversion
 *                 gives that byte), with ts.waterfall.contrast 100, so UiSpectrum_DrawWaterfall
 *                 itself scales, clips, converts and stores it.
 *   wfall_driver spec <out.bin> <fft_len> <width> <db_scale> <agc_rate> <contrast> <height> <color_scheme> <vert_step_size> <marker_colour> <harness arguments...>
 *       the harness' spectrum run; per display frame states 4 and 5 of UiSpectrum_RedrawSpectrum on its
 *       average, waterfall only
 *   out.bin:  per frame uint32 sd.FFT_frequency, int32 the ring line written, width bytes of that
 *             line after the frame, int32 rows put (0 or height), then rows * width uint16;
 *             then the tail: int32 wfall_size, repeat, marker_num; float hz_per_pixel, rx_carrier_pos,
 *             marker_pos[3]; uint16 colours[65] and one uint16 0; int32 sd.magnify, ts.iq_freq_mode,
 *             ts.dmod_mode, sd.wfall_line, sd.wfall_line_update
 *   wfall_driver tables <out.bin>
 *       int32 palettes, then per palette 64 uint16
 *
 * One process per channel: the ring, the counters and doubleLineStart are globals or statics.
 */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "uhsdr_board.h"
#include "arm_math.h"
#include "audio_driver.h"
#include "audio_filter.h"
#include "radio_management.h"
#include "ui_spectrum.h"
#include "ui_lcd_hy28.h"
#include "ui_lcd_layouts.h"
#include "rtty.h"
#include "psk.h"

const uint16_t* WfallRec_palette(int k);
int WfallRec_palette_num(void);
void WfallRec_init(int width, int height, int scope_h);
void WfallRec_draw(void);
int WfallRec_states_4_5(void);
void WfallRec_plan(int32_t* ints, float* floats, uint16_t* colours);
uint32_t WfallRec_line(void);
const uint8_t* WfallRec_ring(uint32_t line);
uint32_t WfallRec_counter(int k);
int WfallRec_ref_main(int argc, char** argv);
void ref_spec_frame(int L, int spectrum_filter, const float* ring, float* mag, float* avg);
void ref_spec_window(int L, float* x);
void ref_cfft(int L, float* p);

enum { WIDTH, HEIGHT, SCHEME, STEP, MARKER_COLOUR, MAGNIFY, IQ_FREQ_MODE, DMOD_MODE, DIGITAL_MODE, CW_LSB, DIGI_LSB, CW_SIDETONE, RTTY_SHIFT,
       PSK_SPEED, TX_MINUS_RX, FRAMES, HEAD };

static int32_t g_case[HEAD];
static uint16_t* g_rows;        /* the rows of the frame under way */
static int g_put;
static FILE* g_out;
static int g_ready, g_spec_cfg[4];      /* fft_len, db_scale, agc_rate, contrast */

disp_resolution_t disp_resolution;
void UiLcdHy28_DrawStraightLine(uint16_t x, uint16_t y, uint16_t length, uint8_t direction, uint16_t color) {}
void UiLcdHy28_DrawColorPoint(uint16_t x, uint16_t y, uint16_t color) {}
void UiLcdHy28_DrawFullRect(uint16_t x, uint16_t y, uint16_t height, uint16_t width, uint16_t color) {}
void UiLcdHy28_BulkPixel_OpenWrite(ushort x, ushort width, ushort y, ushort height) {}
void UiLcdHy28_BulkPixel_CloseWrite(void) {}
void UiLcdHy28_BulkPixel_Put(uint16_t pixel) {}
void UiLcdHy28_BulkPixel_Puts(uint16_t pixel, uint32_t len) {}
void UiLcdHy28_BulkPixel_PutBuffer(uint16_t* pixel_buffer, uint32_t len)
{
    if ((int)len != g_case[WIDTH] || g_put >= g_case[HEIGHT]) { fprintf(stderr, "row %d of %u pixels\n", g_put, len); exit(1); }
    memcpy(g_rows + (size_t)g_put * len, pixel_buffer, 2 * len);
    g_put++;
}
void UiMenu_MapColors(uint32_t color, char* options, volatile uint32_t* clr_ptr) { if (clr_ptr) *clr_ptr = (uint32_t)g_case[MARKER_COLOUR]; }
uint32_t RadioManagement_GetRXDialFrequency(void) { return 7100000; }
uint32_t RadioManagement_GetTXDialFrequency(void) { return (uint32_t)(7100000 + g_case[TX_MINUS_RX]); }

static void panel_init(int scope_h)
{
    ts.waterfall.vert_step_size = g_case[STEP];
    ts.waterfall.color_scheme = g_case[SCHEME];
    ts.flags1 |= FLAGS1_SCOPE_ENABLED | FLAGS1_WFALL_ENABLED;
    ts.txrx_mode = TRX_MODE_RX;
    ts.ptt_req = false;
    ts.menu_mode = false;
    if (!ts.filters_p) ts.filters_p = &FilterPathInfo[48];
    WfallRec_init(g_case[WIDTH], g_case[HEIGHT], scope_h);
    g_rows = malloc(2 * (size_t)g_case[WIDTH] * g_case[HEIGHT]);
    g_ready = 1;
}

/* `draw`: the call that reaches UiSpectrum_DrawWaterfall */
static void record_frame(int states)
{
    const int W = g_case[WIDTH];
    const uint32_t hz = sd.FFT_frequency;
    const int32_t at = (int32_t)WfallRec_line();
    g_put = 0;
    if (states) { if (WfallRec_states_4_5()) { fprintf(stderr, "state 4 did not run\n"); exit(1); } }
    else WfallRec_draw();
    if (g_put != 0 && g_put != g_case[HEIGHT]) { fprintf(stderr, "%d rows put\n", g_put); exit(1); }
    const int32_t put = g_put;
    fwrite(&hz, 4, 1, g_out);
    fwrite(&at, 4, 1, g_out);
    fwrite(WfallRec_ring((uint32_t)at), 1, W, g_out);
    fwrite(&put, 4, 1, g_out);
    fwrite(g_rows, 2, (size_t)put * W, g_out);
}

static void finish(void)
{
    int32_t ints[3];
    float floats[5];
    uint16_t colours[66] = { 0 };
    WfallRec_plan(ints, floats, colours);
    const int32_t echo[5] = { sd.magnify, ts.iq_freq_mode, ts.dmod_mode, (int32_t)WfallRec_counter(0), (int32_t)WfallRec_counter(1) };
    fwrite(ints, 4, 3, g_out);
    fwrite(floats, 4, 5, g_out);
    fwrite(colours, 2, 66, g_out);
    fwrite(echo, 4, 5, g_out);
    fclose(g_out);
}

/* the harness' frame, then states 4 and 5 on what it left (as display_driver's) */
void WfallRec_spec_frame(int L, int spectrum_filter, const float* ring, float* mag, float* avg)
{
    static float buf[2048];
    if (!g_ready)
    {
        ts.spectrum_db_scale = g_spec_cfg[1];
        ts.spectrum_agc_rate = g_spec_cfg[2];
        ts.waterfall.contrast = g_spec_cfg[3];
        panel_init(L == 256 ? 21 : 64);
    }
    if (L != g_spec_cfg[0] || L != sd.spec_len) { fprintf(stderr, "spec=%d against fft_len %d\n", L, g_spec_cfg[0]); exit(1); }
    ref_spec_frame(L, spectrum_filter, ring, mag, avg);
    memcpy(buf, ring, sizeof(float) * 2 * L);
    ref_spec_window(L, buf);
    ref_cfft(L, buf);
    memcpy(sd.FFT_Samples, buf, sizeof(float) * 2 * L);
    memcpy(sd.FFT_MagData, mag, sizeof(float) * L);
    memcpy(sd.FFT_AVGData, avg, sizeof(float) * L);
    record_frame(1);
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "tables"))
    {
        FILE* o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 1; }
        const int32_t n = WfallRec_palette_num();
        fwrite(&n, 4, 1, o);
        for (int k = 0; k < n; k++) fwrite(WfallRec_palette(k), 2, NUMBER_WATERFALL_COLOURS, o);
        fclose(o);
        return 0;
    }
    if (argc >= 13 && !strcmp(argv[1], "spec"))
    {
        g_out = fopen(argv[2], "wb");
        if (!g_out) { perror(argv[2]); return 1; }
        g_spec_cfg[0] = atoi(argv[3]);
        g_case[WIDTH] = atoi(argv[4]);
        for (int k = 0; k < 3; k++) g_spec_cfg[1 + k] = atoi(argv[5 + k]);
        g_case[HEIGHT] = atoi(argv[8]);
        g_case[SCHEME] = atoi(argv[9]);
        g_case[STEP] = atoi(argv[10]);
        g_case[MARKER_COLOUR] = atoi(argv[11]);
        argv[11] = argv[0];
        const int rc = WfallRec_ref_main(argc - 11, argv + 11);
        if (rc || !g_ready) { fprintf(stderr, "harness run failed (%d)\n", rc); return 1; }
        finish();
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "run"))
    {
        fprintf(stderr, "usage: wfall_driver run <case.bin> <out.bin> | spec <out.bin> <nine settings> <harness arguments> | tables <out.bin>\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    if (fread(g_case, 4, HEAD, f) != HEAD) { fprintf(stderr, "short head\n"); return 1; }
    const int W = g_case[WIDTH];
    if (W < 1 || W > SPECTRUM_WIDTH_MAX || g_case[HEIGHT] < 1 || g_case[HEIGHT] > 255) { fprintf(stderr, "width %d height %d\n", W, g_case[HEIGHT]); return 1; }
    g_out = fopen(argv[3], "wb");
    if (!g_out) { perror(argv[3]); return 1; }
    sd.magnify = g_case[MAGNIFY];
    ts.iq_freq_mode = g_case[IQ_FREQ_MODE];
    ts.dmod_mode = g_case[DMOD_MODE];
    ts.digital_mode = g_case[DIGITAL_MODE] == 1 ? DigitalMode_RTTY : g_case[DIGITAL_MODE] == 2 ? DigitalMode_BPSK : DigitalMode_None;
    ts.cw_lsb = g_case[CW_LSB];
    ts.digi_lsb = g_case[DIGI_LSB];
    ts.cw_sidetone_freq = g_case[CW_SIDETONE];
    rtty_ctrl_config.shift_idx = g_case[RTTY_SHIFT];
    psk_ctrl_config.speed_idx = g_case[PSK_SPEED];
    ts.waterfall.contrast = 100;
    panel_init(32);
    uint8_t line[SPECTRUM_WIDTH_MAX];
    for (int k = 0; k < g_case[FRAMES]; k++)
    {
        uint32_t hz;
        if (fread(&hz, 4, 1, f) != 1 || fread(line, 1, W, f) != (size_t)W) { fprintf(stderr, "short frame %d\n", k); return 1; }
        memset(sd.FFT_Samples, 0, sizeof sd.FFT_Samples);
        for (int i = 0; i < W; i++) sd.FFT_Samples[i] = line[i] < NUMBER_WATERFALL_COLOURS ? (float)line[i] : (float)(line[i] - 256);
        sd.FFT_frequency = hz;
        record_frame(0);
    }
    finish();
    fclose(f);
    return 0;
}
