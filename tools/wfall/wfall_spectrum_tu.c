/*
 * Fixture recorder for the waterfall image (tests/golden/wfall_*.npz), first of two translation
 * units: the reference's ui_spectrum.c, included where it lies, for its static functions
 * UiSpectrum_InitSpectrumDisplayData, UiSpectrum_UpdateSpectrumPixelParameters (reached through
 * UiSpectrum_DrawWaterfall), UiSpectrum_DrawWaterfall and UiSpectrum_RedrawSpectrum, its slayout and
 * the five palettes of waterfall_colours.h.
 *
 * The file assembles on x86 once __DSB is empty.  Nothing of a function is restated: the wrappers
 * below only set the panel, call the functions and read sd back.  Nothing of this program or its
 * output other than the recorded data is committed.
 */
#include <math.h>
#include <string.h>
#include "uhsdr_board.h"
#include "arm_math.h"
#undef __DSB
#define __DSB() ((void)0)
#include "ui_spectrum.h"

#include "ui_spectrum.c"

/* palette k in the order of ts.waterfall.color_scheme (:997-1015) */
const uint16_t* WfallRec_palette(int k)
{
    switch (k)
    {
    case WFALL_HOT_COLD: return waterfall_cold_hot;
    case WFALL_RAINBOW: return waterfall_rainbow;
    case WFALL_BLUE: return waterfall_blue;
    case WFALL_GRAY_INVERSE: return waterfall_grey_inverse;
    default: return waterfall_grey;
    }
}
int WfallRec_palette_num(void) { return WFALL_COLOR_NUM; }

/* the panel: a spectrum of 256 bins for widths up to 256, of 512 above (:967-985); the ring and its
   frequencies cleared as UiSpectrum_InitSpectrum does (UiSpectrum_WaterfallClearData) */
void WfallRec_init(int width, int height, int scope_h)
{
    disp_resolution = width <= 256 ? RESOLUTION_320_240 : RESOLUTION_480_320;
    memset(&slayout, 0, sizeof slayout);
    sd.Slayout = &slayout;
    slayout.scope.w = slayout.wfall.w = width;
    slayout.scope.h = scope_h;
    slayout.wfall.h = height;
    UiSpectrum_InitSpectrumDisplayData();
    UiSpectrum_WaterfallClearData();
    sd.vert_grid = width / SPECTRUM_SCOPE_GRID_VERT_COUNT;
    sd.display_offset = INIT_SPEC_AGC_LEVEL;
    sd.wfall_line = 0;
}

/* one call of UiSpectrum_DrawWaterfall on sd.FFT_Samples as it stands */
void WfallRec_draw(void) { UiSpectrum_DrawWaterfall(); }

/* states 4 and 5 of UiSpectrum_RedrawSpectrum on sd.FFT_AVGData, waterfall only; 0 if both ran */
int WfallRec_states_4_5(void)
{
    sd.RedrawType = Redraw_WATERFALL;
    sd.state = 4;
    UiSpectrum_RedrawSpectrum();
    if (sd.state != 5) return 1;
    sd.RedrawType = Redraw_WATERFALL;
    UiSpectrum_RedrawSpectrum();
    return 0;
}

/* what UiSpectrum_InitSpectrumDisplayData and UiSpectrum_UpdateSpectrumPixelParameters left:
   int32 wfall_size, repeat, marker_num, then float hz_per_pixel, rx_carrier_pos and the marker
   positions, then the 65 colours */
void WfallRec_plan(int32_t* ints, float* floats, uint16_t* colours)
{
    ints[0] = sd.wfall_size;
    ints[1] = sd.repeatWaterfallLine;
    ints[2] = sd.marker_num;
    floats[0] = sd.hz_per_pixel;
    floats[1] = sd.rx_carrier_pos;
    for (int k = 0; k < SPECTRUM_MAX_MARKER; k++) floats[2 + k] = sd.marker_pos[k];
    memcpy(colours, sd.waterfall_colours, sizeof sd.waterfall_colours);
}

/* the ring line the next frame writes, and that line after the frame */
uint32_t WfallRec_line(void) { return sd.wfall_line % sd.wfall_size; }
const uint8_t* WfallRec_ring(uint32_t line) { return &sd.waterfall[line * slayout.wfall.w]; }
uint32_t WfallRec_counter(int k) { return k == 0 ? sd.wfall_line : sd.wfall_line_update; }
