/*
 * Fixture recorder for the display stage, first of two translation units: the reference's
 * ui_spectrum.c, included where it lies, for its static functions UiSpectrum_InitSpectrumDisplayData,
 * UiSpectrum_ScaleFFT, UiSpectrum_ScaleFFT2SpectrumWidth, UiSpectrum_DrawScope and
 * UiSpectrum_DrawWaterfall, its scope_scaling_factors table and its slayout.
 *
 * The file assembles on x86 once __DSB is empty.  Nothing of a function is restated: the wrappers
 * below only call them.  DisplayRec_frame sets sd.state to 4 and calls UiSpectrum_RedrawSpectrum twice
 * (:1467-1517), with both redraw types wanted, so states 4 and 5 run as the firmware has them.
 * The heights are read back from sd.Old_PosData, where UiSpectrum_DrawScope leaves spec_top_y minus
 * the height of every column (:886-891); the byte line from sd.waterfall at the line
 * UiSpectrum_DrawWaterfall wrote (:1118).  Nothing of this program or its output other than the
 * recorded data is committed.
 */
#include <math.h>
#include <string.h>
#include "uhsdr_board.h"
#include "arm_math.h"
#undef __DSB
#define __DSB() ((void)0)
#include "ui_spectrum.h"

#include "ui_spectrum.c"

float DisplayRec_scaling_factor(int k) { return scope_scaling_factors[k].value; }
int DisplayRec_scale_num(void) { return SCOPE_SCALE_NUM; }

/* A width above SPECTRUM_WIDTH_MAX (480; no panel of the firmware is wider) overruns sd.Old_PosData,
   which has that many entries, into the fields of sd behind it, up to fft_iq_len.  The width
   reduction itself knows no such limit, so such a width is recorded all the same, around the array:
   UiSpectrum_InitSpectrumDisplayData runs once at SPECTRUM_WIDTH_MAX, the fields its loop over
   Old_PosData would overrun are kept from that run (none of them depends on the width), and
   UiSpectrum_DrawScope, which takes its column memory as an argument, gets an array long enough. */
static uint16_t DisplayRec_old_pos[FFT_IQ_BUFF_LEN];
static int DisplayRec_wide;

/* the panel: fft_len 256 is the 320 x 240 resolution, 512 the 480 x 320 one (:967-985) */
void DisplayRec_init(int fft_len, int width, int scope_h)
{
    disp_resolution = fft_len == 256 ? RESOLUTION_320_240 : RESOLUTION_480_320;
    memset(&slayout, 0, sizeof slayout);
    sd.Slayout = &slayout;
    slayout.scope.h = scope_h;
    slayout.wfall.h = 1;                    /* one line of sd.waterfall: every frame writes line 0 */
    DisplayRec_wide = width > SPECTRUM_WIDTH_MAX;
    if (DisplayRec_wide)
    {
        char keep[(char*)&sd.cfft_instance - (char*)&sd.samp_ptr];
        slayout.scope.w = slayout.wfall.w = SPECTRUM_WIDTH_MAX;
        UiSpectrum_InitSpectrumDisplayData();
        memcpy(keep, &sd.samp_ptr, sizeof keep);
        slayout.scope.w = slayout.wfall.w = width;
        UiSpectrum_InitSpectrumDisplayData();
        memcpy(&sd.samp_ptr, keep, sizeof keep);
    }
    else
    {
        slayout.scope.w = slayout.wfall.w = width;
        UiSpectrum_InitSpectrumDisplayData();
    }
    sd.vert_grid = width / SPECTRUM_SCOPE_GRID_VERT_COUNT;    /* the grid's spacing as :632 sets it; UiSpectrum_DrawScope divides by it */
    sd.display_offset = INIT_SPEC_AGC_LEVEL;
    sd.wfall_line = 0;
}

/* States 4 and 5 of UiSpectrum_RedrawSpectrum itself on sd.FFT_AVGData and sd.FFT_Samples as they
   stand, scope and waterfall both due.  min1 is a local of state 4, so it is taken from a call of
   UiSpectrum_ScaleFFT of its own into a row that nothing reads, with the offset state 4 will see.
   A width above SPECTRUM_WIDTH_MAX: the calls of the two states (:1471-1501), in their order, with
   the longer column memory. */
float DisplayRec_frame(uint16_t* heights, uint8_t* line)
{
    static float32_t unused[FFT_IQ_BUFF_LEN];
    float32_t min1 = 100000;
    const uint32_t at = sd.wfall_line % sd.wfall_size;
    uint16_t* old_pos = sd.Old_PosData;
    if (DisplayRec_wide)
    {
        old_pos = DisplayRec_old_pos;
        UiSpectrum_ScaleFFT(sd.FFT_Samples, sd.FFT_AVGData, &min1);
        UiSpectrum_ScaleFFT2SpectrumWidth(sd.FFT_Samples, sd.spec_len, slayout.scope.w);
        sd.display_offset -= sd.agc_rate * min1 / 5;
        UiSpectrum_DrawScope(old_pos, sd.FFT_Samples);
        UiSpectrum_DrawWaterfall();
    }
    else
    {
        UiSpectrum_ScaleFFT(unused, sd.FFT_AVGData, &min1);
        sd.RedrawType = Redraw_SCOPE | Redraw_WATERFALL;
        sd.state = 4;
        UiSpectrum_RedrawSpectrum();
        if (sd.state != 5) return NAN;
        UiSpectrum_RedrawSpectrum();
    }
    const uint16_t spec_top_y = sd.scope_ystart + sd.scope_size;
    for (int i = 0; i < slayout.scope.w; i++) heights[i] = (uint16_t)(spec_top_y - old_pos[i]);
    memcpy(line, &sd.waterfall[at * slayout.wfall.w], slayout.wfall.w);
    return min1;
}
