/*
 * Waterfall image, the steps for host and device: the rest of UiSpectrum_DrawWaterfall
 * (drivers/ui/lcd/ui_spectrum.c:1099-1256) behind the byte line of the display stage.
 *
 *   wfall_advance        the counters of one frame (:1101, :1131-1152): which ring line the frame
 *                        writes, whether it draws, and where the drawing starts
 *   wfall_row_line       which ring line a row of a drawing shows (:1165, :1237-1248)
 *   wfall_offset_pixel   a ring line's shift against the frame that draws (:1173-1188)
 *   wfall_pixel          one pixel of a shifted line through the palette (:1189-1224)
 *   wfall_markers, wfall_marked   the markers' columns, and whether a column is one (:1226-1233)
 *   wfall_describe       a whole call's counters in one pass: the descriptor the kernels take
 *   wfall_channel_host   one channel, frame after frame as the firmware runs them (the host twin)
 *
 * The counters never look at the data: wfall_line, doubleLineStart and wfall_line_update are the same
 * for every channel, so the host advances them once per call and the descriptor (WfallCall) tells
 * the kernels, per image row, which line it shows and whether a frame of this call or an earlier
 * call wrote that line last, and per ring line which frame of the call it keeps.  No kernel walks
 * the frames.
 *
 * Kept as the reference has them: with a frame that does not advance wfall_line the drawing starts
 * at the line BEFORE the one just written (lptr = wfall_line - 1, :1150), so that frame's own line
 * shows only after a later frame has advanced; a ring line is written repeat + 1 times and keeps the
 * last; |offset_pixel| >= width gives width - 1 of left padding for either sign; the subtraction of
 * the two frequencies is the int32 one and wraps; offset_pixel is the binary32 quotient truncated.
 * Defined here, not kept: a ring byte above 64 is colour 0 (the firmware reads behind its palette).
 */
#ifndef UHSDR_WFALL_H
#define UHSDR_WFALL_H

#include <stdint.h>
#include <string.h>

#include "uhsdr_internal.h"

#ifdef __HIPCC__
#define WFALL_FN __host__ __device__ static inline
#else
#define WFALL_FN static inline
#endif

#define WFALL_MARKER_ENTRY 64               /* NUMBER_WATERFALL_COLOURS: the palette entry of the markers */
#define WFALL_BLACK 0                       /* Black, ui_lcd_hy28.h */
#define WFALL_MAX_HEIGHT 255

/* the handle's counters: sd.wfall_line, the function static doubleLineStart, sd.wfall_line_update */
typedef struct wfall_counters
{
    uint32_t line;
    uint32_t dls;                           /* a uint8_t in the firmware: 0 .. repeat */
    uint32_t update;
} wfall_counters;

/* One frame.  Returns the ring line the frame writes; *draws: the frame draws; *lptr: the ring line
   of the drawing's first row (meaningful for every frame, used when it draws). */
WFALL_FN uint32_t wfall_advance(const uhsdr_wfall_plan* p, wfall_counters* k, int* draws, uint32_t* lptr)
{
    const uint32_t size = (uint32_t)p->wfall_size;
    k->line %= size;                                            /* :1101 */
    const uint32_t at = k->line;
    if (k->dls == 0) { k->dls = (uint32_t)p->repeat; k->line++; }   /* doubleLineStart-- wraps to 0xff, :1134-1139 */
    else k->dls--;
    k->update = (k->update + 1) % (uint32_t)p->vert_step_size;  /* :1143-1144 */
    *draws = k->update == 0;
    uint32_t l = k->line;
    l = l ? l - 1 : size - 1;                                   /* :1150-1152 */
    *lptr = l % size;
    return at;
}

/* the ring line row r of a drawing shows: the first line is put repeat + 1 - dls times, every other
   repeat + 1 times, walking back from lptr around the ring */
WFALL_FN uint32_t wfall_row_line(const uhsdr_wfall_plan* p, uint32_t lptr, uint32_t dls, int r)
{
    const int per = p->repeat + 1, head = per - (int)dls;
    const int back = r < head ? 0 : 1 + (r - head) / per;
    const int size = p->wfall_size;
    return (uint32_t)((((int)lptr - back) % size + size) % size);
}

/* :1173-1188 */
WFALL_FN int32_t wfall_offset_pixel(const uhsdr_wfall_plan* p, uint32_t line_hz, uint32_t cur_hz)
{
    const int32_t diff_centers = (int32_t)(line_hz - cur_hz);
    int32_t offset_pixel = (int32_t)((float)diff_centers / p->hz_per_pixel);
    if (offset_pixel >= p->width || offset_pixel <= -p->width) offset_pixel = p->width - 1;
    return offset_pixel;
}

/* the palette entry of a ring byte */
WFALL_FN uint16_t wfall_colour(const uint16_t* colours, uint8_t b)
{
    return colours[b <= WFALL_MARKER_ENTRY ? b : 0];
}

/* column x of a line moved right by offset_pixel: black where nothing comes (:1189-1224) */
WFALL_FN uint16_t wfall_pixel(const uint16_t* colours, const uint8_t* line, int W, int32_t offset_pixel, int x)
{
    const int s = x - offset_pixel;
    return (s < 0 || s >= W) ? (uint16_t)WFALL_BLACK : wfall_colour(colours, line[s]);
}

/* :1110-1114, :1226-1233: the columns of the markers in use; an unused one gets -1, which no column equals */
WFALL_FN void wfall_markers(const uhsdr_wfall_plan* p, int* mk)
{
    for (int m = 0; m < UHSDR_WFALL_MAX_MARKER; m++) mk[m] = m < p->marker_num ? (int)p->marker_pixel[m] : -1;
}

WFALL_FN int wfall_marked(const int* mk, int x)
{
    int hit = 0;
    for (int m = 0; m < UHSDR_WFALL_MAX_MARKER; m++) hit |= mk[m] == x;
    return hit;
}

/* What a call of F frames does, from the counters alone. */
typedef struct WfallCall
{
    int32_t frames;
    int32_t draw_frame;                     /* the last frame of the call that draws; -1: none does */
    int32_t update0;                        /* wfall_line_update before the call */
    int32_t step;                           /* vert_step_size */
    /* per image row of that drawing: the frame of this call whose line the row shows (the last one
       up to draw_frame that wrote its ring line), or -1 - ring line where an earlier call wrote it */
    int32_t row_src[WFALL_MAX_HEIGHT];
    /* per ring line: the last frame of the call that writes it; -1: none */
    int32_t last[UHSDR_WFALL_MAX_LINES];
} WfallCall;

/* Fills *call for `frames` frames from counters *k, which it advances.  Two passes over the frames'
   counters: the first finds the last drawing, the second the last writers up to it and up to the end. */
static inline void wfall_describe(const uhsdr_wfall_plan* p, wfall_counters* k, int32_t frames, WfallCall* call)
{
    wfall_counters probe = *k;
    int draws;
    uint32_t lptr, draw_lptr = 0, draw_dls = 0;
    call->frames = frames;
    call->draw_frame = -1;
    call->update0 = (int32_t)k->update;
    call->step = p->vert_step_size;
    for (int r = 0; r < WFALL_MAX_HEIGHT; r++) call->row_src[r] = -1;
    for (int l = 0; l < UHSDR_WFALL_MAX_LINES; l++) call->last[l] = -1;
    for (int32_t f = 0; f < frames; f++)
    {
        wfall_advance(p, &probe, &draws, &lptr);
        if (draws) { call->draw_frame = f; draw_lptr = lptr; draw_dls = probe.dls; }
    }
    for (int32_t f = 0; f < frames; f++)
    {
        call->last[wfall_advance(p, k, &draws, &lptr)] = f;
        if (f == call->draw_frame)
            for (int r = 0; r < p->height; r++)
            {
                const uint32_t l = wfall_row_line(p, draw_lptr, draw_dls, r);
                call->row_src[r] = call->last[l] >= 0 ? call->last[l] : -1 - (int32_t)l;
            }
    }
}

/* One channel on the CPU, frame after frame: the line and its frequency into the ring, the counters,
   and the whole drawing of every frame that draws (a later drawing overwrites an earlier one's
   image, as the panel's).  ring: wfall_size * width bytes; freq: wfall_size words; lines: [frames][width];
   center_hz: [frames] or null (0); image: [height][width] or null; drawn: [frames] or null. */
static inline void wfall_channel_host(const uhsdr_wfall_plan* p, wfall_counters k, uint8_t* ring, uint32_t* freq, const uint8_t* lines,
                                      const uint32_t* center_hz, int32_t frames, uint16_t* image, uint8_t* drawn)
{
    const int W = p->width;
    int mk[UHSDR_WFALL_MAX_MARKER];
    wfall_markers(p, mk);
    for (int32_t f = 0; f < frames; f++)
    {
        int draws;
        uint32_t lptr;
        const uint32_t cur_hz = center_hz ? center_hz[f] : 0;
        const uint32_t at = wfall_advance(p, &k, &draws, &lptr);
        memcpy(ring + (size_t)at * W, lines + (size_t)f * W, (size_t)W);
        freq[at] = cur_hz;
        if (drawn) drawn[f] = (uint8_t)draws;
        if (!draws || !image) continue;
        for (int r = 0; r < p->height; r++)
        {
            const uint32_t l = wfall_row_line(p, lptr, k.dls, r);
            const int32_t offset_pixel = wfall_offset_pixel(p, freq[l], cur_hz);
            for (int x = 0; x < W; x++)
                image[(size_t)r * W + x] = wfall_marked(mk, x) ? p->colours[WFALL_MARKER_ENTRY] : wfall_pixel(p->colours, ring + (size_t)l * W, W, offset_pixel, x);
        }
    }
}

#endif
