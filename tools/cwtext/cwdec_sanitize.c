/*
 * Stand-alone driver of uhsdr_cwdec_process_host for a host sanitizer build (no device call):
 *
 *   make sanitize          (tools/sanitize.mk: builds cwdec_sanitize and runs it on what dump_states.py writes)
 *
 * File: int32 cases; per case int32 blocksize, spikecancel, blocks, nchars, then the state bytes
 * and the expected characters.  Every case runs in one piece and in calls of 1 and 97 blocks, alone
 * and as one of three channels; the text is compared as well.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr.h"

static int run(const uint8_t* state, int blocks, int blocksize, int spikecancel, const uint8_t* chars, int nchars, int per_call,
               int channels)
{
    uhsdr_cwdec_handle h;
    const int cap = 4096;
    if (uhsdr_cwdec_create_host(channels, blocksize, spikecancel, cap, &h) != UHSDR_OK) return 1;
    uint8_t* rows = malloc((size_t)channels * per_call);
    for (int b = 0; b < blocks; b += per_call)
    {
        const int n = blocks - b < per_call ? blocks - b : per_call;
        for (int c = 0; c < channels; c++) memcpy(rows + (size_t)c * n, state + b, n);     /* exact-size rows */
        if (uhsdr_cwdec_process_host(h, rows, n, n) != UHSDR_OK) return 1;
    }
    free(rows);
    uint8_t* text; uint32_t* total; uint8_t* wpm;
    uhsdr_cwdec_outputs(h, &text, &total, &wpm);
    int bad = 0;
    for (int c = 0; c < channels; c++)
        bad |= (int)total[c] != nchars || memcmp(text + (size_t)c * cap, chars, nchars) != 0;
    uhsdr_cwdec_destroy(h);
    return bad;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: cwdec_sanitize <states.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t hd[4];
        if (fread(hd, 4, 4, f) != 4) return 1;
        uint8_t* state = malloc(hd[2] ? hd[2] : 1);
        uint8_t* chars = malloc(hd[3] ? hd[3] : 1);
        if (fread(state, 1, hd[2], f) != (size_t)hd[2] || fread(chars, 1, hd[3], f) != (size_t)hd[3]) return 1;
        const int b1 = run(state, hd[2], hd[0], hd[1], chars, hd[3], hd[2], 1);
        const int b2 = run(state, hd[2], hd[0], hd[1], chars, hd[3], 97, 3);
        const int b3 = run(state, hd[2], hd[0], hd[1], chars, hd[3], 1, 1);
        printf("case %d: blocksize %d spikecancel %d, %d blocks, %d chars: %s\n", k, hd[0], hd[1], hd[2], hd[3],
               b1 | b2 | b3 ? "MISMATCH" : "ok");
        bad |= b1 | b2 | b3;
        free(state);
        free(chars);
    }
    fclose(f);
    return bad;
}
