/*
 * Stand-alone driver of the waterfall image's host step functions (uhsdr_amd/csrc/uhsdr_wfall.h, the
 * text the wfall_image and wfall_commit kernels run) for a host sanitizer build; plain C, no device
 * call:
 *
 *   make sanitize          (tools/sanitize.mk: builds wfall_sanitize and runs it on what dump_cases.py writes)
 *
 * File: see dump_cases.py.  Every channel of every case runs twice, from heap blocks of exactly the
 * sizes the library allocates (so a read or write outside them is seen):
 *   frame by frame through wfall_channel_host, the image compared with the recording after every
 *     frame that drew;
 *   in calls of 1, 2, 3, 5 and all frames through the call's descriptor (wfall_describe) the way the
 *     kernels use it: each image row from the line of the call or the ring line the descriptor names,
 *     then the ring's lines from their last writers; image and ring compared with the first run's
 *     after every call.
 * Then descriptors of long calls over every ring geometry: each entry must name a frame of the call
 * or a ring line, and agree with a walk over the frames.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr_wfall.h"

/* one call as the kernels run it */
static void call_by_descriptor(const uhsdr_wfall_plan* p, wfall_counters* k, uint8_t* ring, uint32_t* freq, const uint8_t* lines,
                               const uint32_t* center_hz, int32_t frames, uint16_t* image)
{
    const int W = p->width;
    WfallCall call;
    int mk[UHSDR_WFALL_MAX_MARKER];
    wfall_markers(p, mk);
    wfall_describe(p, k, frames, &call);
    if (call.draw_frame >= 0)
        for (int r = 0; r < p->height; r++)
        {
            const int32_t src = call.row_src[r];
            const uint8_t* line = src >= 0 ? lines + (size_t)src * W : ring + (size_t)(-1 - src) * W;
            const uint32_t line_hz = src >= 0 ? center_hz[src] : freq[-1 - src];
            const int32_t offset_pixel = wfall_offset_pixel(p, line_hz, center_hz[call.draw_frame]);
            for (int x = 0; x < W; x++)
                image[(size_t)r * W + x] = wfall_marked(mk, x) ? p->colours[WFALL_MARKER_ENTRY] : wfall_pixel(p->colours, line, W, offset_pixel, x);
        }
    for (int l = 0; l < p->wfall_size; l++)
        if (call.last[l] >= 0)
        {
            memcpy(ring + (size_t)l * W, lines + (size_t)call.last[l] * W, (size_t)W);
            freq[l] = center_hz[call.last[l]];
        }
}

static int geometries(void)
{
    long calls = 0;
    for (int W = 128; W <= 512; W += 64)
        for (int H = 1; H <= 255; H += (H < 12 ? 1 : 9))
            for (int step = 1; step <= 5; step++)
            {
                uhsdr_wfall_plan p;
                memset(&p, 0, sizeof p);
                int size = H;
                if (size * W > UHSDR_WFALL_RING_BYTES) size = size / 2 * W > UHSDR_WFALL_RING_BYTES ? UHSDR_WFALL_RING_BYTES / W : size / 2;
                if (size > UHSDR_WFALL_MAX_LINES) continue;
                p.width = W; p.height = H; p.wfall_size = size; p.repeat = H / size; p.vert_step_size = step;
                wfall_counters k = { 0, 0, 0 }, walk = { 0, 0, 0 };
                for (int n = 1; n < 700; n = n * 2 + 1)
                {
                    WfallCall* call = malloc(sizeof *call);
                    int* last = malloc(sizeof(int) * (size_t)size);
                    for (int l = 0; l < size; l++) last[l] = -1;
                    wfall_describe(&p, &k, n, call);
                    int draws, drew = -1;
                    uint32_t lptr, dl = 0, dd = 0;
                    int* at_draw = malloc(sizeof(int) * (size_t)size);
                    for (int f = 0; f < n; f++)
                    {
                        last[wfall_advance(&p, &walk, &draws, &lptr)] = f;
                        if (draws) { drew = f; dl = lptr; dd = walk.dls; memcpy(at_draw, last, sizeof(int) * (size_t)size); }
                    }
                    int bad = drew != call->draw_frame || walk.line != k.line || walk.dls != k.dls || walk.update != k.update;
                    for (int l = 0; l < size; l++) bad |= last[l] != call->last[l];
                    for (int r = 0; drew >= 0 && r < H; r++)
                    {
                        const uint32_t l = wfall_row_line(&p, dl, dd, r);
                        bad |= l >= (uint32_t)size || call->row_src[r] != (at_draw[l] >= 0 ? at_draw[l] : -1 - (int)l);
                        bad |= call->row_src[r] >= n || call->row_src[r] < -size;
                    }
                    free(call); free(last); free(at_draw);
                    if (bad) { printf("descriptor: %d x %d step %d call of %d frames\n", W, H, step, n); return 1; }
                    calls++;
                }
            }
    printf("descriptors: %ld calls agree with the walk over their frames\n", calls);
    return 0;
}

int main(int argc, char** argv)
{
    static const int call_sizes[5] = { 1, 2, 3, 5, 1 << 30 };
    if (argc != 2) { fprintf(stderr, "usage: wfall_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    static uhsdr_wfall_plan plan;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t head[5];
        if (fread(head, 4, 5, f) != 5) return 1;
        const int C = head[1], F = head[2], W = head[3], H = head[4];
        if (head[0] != (int32_t)sizeof plan || fread(&plan, sizeof plan, 1, f) != 1 || W != plan.width || H != plan.height)
        { fprintf(stderr, "case %d: plan\n", k); return 1; }
        const size_t n = (size_t)C * F, px = (size_t)H * W, S = (size_t)plan.wfall_size;
        uint8_t* lines = malloc(n * W);
        uint32_t* hz = malloc(4 * n);
        uint8_t* drawn = malloc(n);
        uint16_t* want = malloc(2 * n * px);
        if (fread(lines, 1, n * W, f) != n * W || fread(hz, 4, n, f) != n || fread(drawn, 1, n, f) != n || fread(want, 2, n * px, f) != n * px) return 1;
        long wrong = 0;
        for (int c = 0; c < C; c++)
        {
            /* frame by frame, against the recording; the ring after every frame kept for the second run */
            uint8_t* ring = calloc(S, W);
            uint32_t* freq = calloc(S, 4);
            uint16_t* image = calloc(px, 2);
            uint8_t* rings = malloc((size_t)F * S * W);
            uint16_t* images = malloc((size_t)F * px * 2);
            wfall_counters kc = { 0, 0, 0 };
            for (int fr = 0; fr < F; fr++)
            {
                uint8_t* line = malloc(W);
                uint8_t got = 2;
                int draws;
                uint32_t lptr;
                memcpy(line, lines + ((size_t)c * F + fr) * W, W);
                wfall_channel_host(&plan, kc, ring, freq, line, &hz[(size_t)c * F + fr], 1, image, &got);
                wfall_advance(&plan, &kc, &draws, &lptr);
                wrong += got != drawn[(size_t)c * F + fr] || got != draws;
                if (got) wrong += memcmp(image, want + ((size_t)c * F + fr) * px, px * 2) != 0;
                memcpy(rings + (size_t)fr * S * W, ring, S * W);
                memcpy(images + (size_t)fr * px, image, px * 2);
                free(line);
            }
            free(ring); free(freq); free(image);
            for (int s = 0; s < 5; s++)
            {
                ring = calloc(S, W);
                freq = calloc(S, 4);
                image = calloc(px, 2);
                wfall_counters kd = { 0, 0, 0 };
                for (int first = 0; first < F; first += call_sizes[s])
                {
                    const int m = F - first < call_sizes[s] ? F - first : call_sizes[s];
                    uint8_t* part = malloc((size_t)m * W);
                    uint32_t* part_hz = malloc(4 * (size_t)m);
                    memcpy(part, lines + ((size_t)c * F + first) * W, (size_t)m * W);
                    memcpy(part_hz, hz + (size_t)c * F + first, 4 * (size_t)m);
                    call_by_descriptor(&plan, &kd, ring, freq, part, part_hz, m, image);
                    wrong += memcmp(ring, rings + (size_t)(first + m - 1) * S * W, S * W) != 0;
                    wrong += memcmp(image, images + (size_t)(first + m - 1) * px, px * 2) != 0;
                    free(part); free(part_hz);
                }
                wrong += kd.line != kc.line || kd.dls != kc.dls || kd.update != kc.update;
                free(ring); free(freq); free(image);
            }
            free(rings); free(images);
        }
        printf("case %d: %d channels x %d frames of %d x %d: %s\n", k, C, F, W, H, wrong ? "MISMATCH" : "ok");
        bad |= wrong != 0;
        free(lines); free(hz); free(drawn); free(want);
    }
    fclose(f);
    if (cases < 1) return 1;
    bad |= geometries();
    return bad;
}
