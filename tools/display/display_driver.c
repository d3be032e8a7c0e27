/*
 * Fixture recorder for the display stage (tests/golden/display_*.npz), second translation unit: the
 * program, and the LCD and menu calls that UiSpectrum_DrawScope and UiSpectrum_DrawWaterfall reach,
 * defined empty.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them (display.mk), with
 * display_spectrum_tu.c, and with the harness, whose ref_main.c is compiled a second time with its
 * main and its call of ref_spec_frame renamed: `spec` below runs that harness program unchanged, so
 * the firmware's own receive path fills sd.FFT_RingBuffer from the I/Q file, and every display frame
 * it then forms comes through DisplayRec_spec_frame here.  Nothing of this program or its output
 * other than the recorded data is committed.
 *
 *   display_driver run <case.bin> <out.bin>
 *       case.bin: int32 fft_len, width, spectrum_db_scale, spectrum_agc_rate, waterfall_contrast,
 *                 scope_h, frames; then per frame float edge (what sd.FFT_Samples[fft_len] holds) and
 *                 fft_len floats of sd.FFT_AVGData
 *   display_driver spec <out.bin> <fft_len> <width> <db_scale> <agc_rate> <contrast> <scope_h> <harness arguments...>
 *       the harness' spectrum run (spec=, in=, n=, out_mag=, out_avg= ...); per frame the harness'
 *       window and arm_cfft_f32 stages on the ring snapshot go to sd.FFT_Samples, its magnitude and
 *       average to sd.FFT_MagData and sd.FFT_AVGData, then states 4 and 5 run
 *       out.bin:  per frame width uint16 heights, width uint8 waterfall bytes, float
 *                 sd.display_offset after the frame, float min1, float sd.FFT_Samples[fft_len] as the
 *                 frame found it; then float sd.db_scale, sd.agc_rate, sd.wfall_contrast
 *   display_driver tables <out.bin>
 *       int32 SCOPE_SCALE_NUM, then that many floats scope_scaling_factors[].value
 *
 * One process per channel: sd.display_offset and the drawing's memory are globals.
 */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "uhsdr_board.h"
#include "arm_math.h"
#include "audio_driver.h"
#include "audio_filter.h"
#include "ui_spectrum.h"
#include "ui_lcd_hy28.h"
#include "ui_lcd_layouts.h"

float DisplayRec_scaling_factor(int k);
int DisplayRec_scale_num(void);
void DisplayRec_init(int fft_len, int width, int scope_h);
float DisplayRec_frame(uint16_t* heights, uint8_t* line);
int DisplayRec_ref_main(int argc, char** argv);
void ref_spec_frame(int L, int spectrum_filter, const float* ring, float* mag, float* avg);
void ref_spec_window(int L, float* x);
void ref_cfft(int L, float* p);

disp_resolution_t disp_resolution;
/* what the two drawing functions reach of the LCD, the menu and the dial */
void UiLcdHy28_DrawStraightLine(uint16_t x, uint16_t y, uint16_t length, uint8_t direction, uint16_t color) {}
void UiLcdHy28_DrawColorPoint(uint16_t x, uint16_t y, uint16_t color) {}
void UiLcdHy28_DrawFullRect(uint16_t x, uint16_t y, uint16_t height, uint16_t width, uint16_t color) {}
void UiLcdHy28_BulkPixel_OpenWrite(ushort x, ushort width, ushort y, ushort height) {}
void UiLcdHy28_BulkPixel_CloseWrite(void) {}
void UiLcdHy28_BulkPixel_PutBuffer(uint16_t* pixel_buffer, uint32_t len) {}
void UiLcdHy28_BulkPixel_Put(uint16_t pixel) {}
void UiLcdHy28_BulkPixel_Puts(uint16_t pixel, uint32_t len) {}
void UiMenu_MapColors(uint32_t color, char* options, volatile uint32_t* clr_ptr) { if (clr_ptr) *clr_ptr = 0; }
uint32_t RadioManagement_GetTXDialFrequency(void) { return 7100000; }
uint32_t RadioManagement_GetRXDialFrequency(void) { return 7100000; }

static int g_cfg[6];        /* fft_len, width, db_scale, agc_rate, contrast, scope_h */
static int g_ready;
static FILE* g_out;

static void panel_init(void)
{
    ts.spectrum_db_scale = g_cfg[2];
    ts.spectrum_agc_rate = g_cfg[3];
    ts.waterfall.contrast = g_cfg[4];
    ts.waterfall.vert_step_size = 1;
    ts.waterfall.color_scheme = WFALL_GRAY;
    ts.flags1 |= FLAGS1_SCOPE_ENABLED | FLAGS1_WFALL_ENABLED;
    ts.txrx_mode = TRX_MODE_RX;
    if (!ts.filters_p) ts.filters_p = &FilterPathInfo[48];
    DisplayRec_init(g_cfg[0], g_cfg[1], g_cfg[5]);
    g_ready = 1;
}

static int record_frame(void)
{
    const int L = g_cfg[0], W = g_cfg[1];
    uint16_t heights[1024];
    uint8_t line[1024];
    const float edge = sd.FFT_Samples[L];
    const float min1 = DisplayRec_frame(heights, line);
    if (isnan(min1) && sd.state != 0) { fprintf(stderr, "state 4 did not run\n"); return 1; }
    const float tail[3] = { sd.display_offset, min1, edge };
    fwrite(heights, 2, W, g_out);
    fwrite(line, 1, W, g_out);
    fwrite(tail, 4, 3, g_out);
    return 0;
}

/* the harness' frame, then the display's on what it left */
void DisplayRec_spec_frame(int L, int spectrum_filter, const float* ring, float* mag, float* avg)
{
    static float buf[2048];
    if (!g_ready) panel_init();
    if (L != g_cfg[0] || L != sd.spec_len) { fprintf(stderr, "spec=%d against fft_len %d\n", L, g_cfg[0]); exit(1); }
    ref_spec_frame(L, spectrum_filter, ring, mag, avg);
    memcpy(buf, ring, sizeof(float) * 2 * L);
    ref_spec_window(L, buf);
    ref_cfft(L, buf);
    memcpy(sd.FFT_Samples, buf, sizeof(float) * 2 * L);       /* state 1's result */
    memcpy(sd.FFT_MagData, mag, sizeof(float) * L);           /* state 2's */
    /* state 3 leaves the scaled magnitudes in the first L floats of sd.FFT_Samples; state 4 overwrites them */
    memcpy(sd.FFT_AVGData, avg, sizeof(float) * L);
    if (record_frame()) exit(1);
}

static void finish(void)
{
    const float plan[3] = { sd.db_scale, sd.agc_rate, sd.wfall_contrast };
    fwrite(plan, 4, 3, g_out);
    fclose(g_out);
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "tables"))
    {
        FILE* o = fopen(argv[2], "wb");
        if (!o) { perror(argv[2]); return 1; }
        const int32_t n = DisplayRec_scale_num();
        fwrite(&n, 4, 1, o);
        for (int k = 0; k < n; k++) { const float v = DisplayRec_scaling_factor(k); fwrite(&v, 4, 1, o); }
        fclose(o);
        return 0;
    }
    if (argc >= 10 && !strcmp(argv[1], "spec"))
    {
        g_out = fopen(argv[2], "wb");
        if (!g_out) { perror(argv[2]); return 1; }
        for (int k = 0; k < 6; k++) g_cfg[k] = atoi(argv[3 + k]);
        argv[8] = argv[0];
        const int rc = DisplayRec_ref_main(argc - 8, argv + 8);
        if (rc || !g_ready) { fprintf(stderr, "harness run failed (%d)\n", rc); return 1; }
        finish();
        return 0;
    }
    if (argc != 4 || strcmp(argv[1], "run"))
    {
        fprintf(stderr, "usage: display_driver run <case.bin> <out.bin> | spec <out.bin> <six settings> <harness arguments> | tables <out.bin>\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    int32_t h[7];
    if (fread(h, 4, 7, f) != 7) { fprintf(stderr, "short head\n"); return 1; }
    memcpy(g_cfg, h, sizeof g_cfg);
    const int L = h[0], frames = h[6];
    if ((L != 256 && L != 512) || h[1] < 1 || h[1] > L) { fprintf(stderr, "fft_len %d width %d\n", L, h[1]); return 1; }
    g_out = fopen(argv[3], "wb");
    if (!g_out) { perror(argv[3]); return 1; }
    panel_init();
    for (int k = 0; k < frames; k++)
    {
        float edge, avg[512];
        if (fread(&edge, 4, 1, f) != 1 || fread(avg, 4, L, f) != (size_t)L) { fprintf(stderr, "short frame %d\n", k); return 1; }
        memset(sd.FFT_Samples, 0, sizeof sd.FFT_Samples);
        sd.FFT_Samples[L] = edge;
        memcpy(sd.FFT_AVGData, avg, sizeof(float) * L);
        if (record_frame()) return 1;
    }
    finish();
    fclose(f);
    return 0;
}
