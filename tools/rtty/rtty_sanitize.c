/*
 * Stand-alone driver of uhsdr_rtty_process_host for a host sanitizer build (no device call):
 *
 *   make sanitize          (tools/sanitize.mk: builds rtty_sanitize and runs it on what dump_streams.py writes)
 *
 * File: see dump_streams.py.  Every case runs in one piece and in calls of 1 and 97 samples, alone
 * and as one of three channels, on exact-size rows, and the text is compared.  Then every
 * configuration runs over pseudo-random input with NaN, infinities and huge samples in it, with
 * the smallest text ring.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr.h"

static int run(const float* audio, int samples, const int32_t* cfg, const uint8_t* chars, int nchars, int per_call, int channels)
{
    uhsdr_rtty_handle h;
    const int cap = 4096;
    if (uhsdr_rtty_create_host(channels, cfg[0], cfg[1], cfg[2], cfg[3], cap, &h) != UHSDR_OK) return 1;
    float* rows = malloc(sizeof(float) * (size_t)channels * per_call);
    for (int b = 0; b < samples; b += per_call)
    {
        const int n = samples - b < per_call ? samples - b : per_call;
        for (int c = 0; c < channels; c++) memcpy(rows + (size_t)c * n, audio + b, sizeof(float) * n);     /* exact-size rows */
        if (uhsdr_rtty_process_host(h, rows, n, n) != UHSDR_OK) return 1;
    }
    free(rows);
    uint8_t* text; uint32_t* total;
    uhsdr_rtty_outputs(h, &text, &total);
    int bad = 0;
    for (int c = 0; c < channels; c++)
        bad |= (int)total[c] != nchars || memcmp(text + (size_t)c * cap, chars, nchars) != 0;
    uhsdr_rtty_destroy(h);
    return bad;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(void)
{
    const int C = 5, n = 20000;
    float* x = malloc(sizeof(float) * C * n);
    unsigned long chars = 0;
    for (int shift = 0; shift < 6; shift++)
        for (int speed = 0; speed < 2; speed++)
            for (int stop = 0; stop < 3; stop++)
                for (int atc = 0; atc < 2; atc++)
                {
                    for (int i = 0; i < C * n; i++)
                    {
                        const uint32_t r = rng();
                        float v = ((int32_t)r / 2147483648.0f) * powf(10.0f, (float)(r % 39));
                        if (r % 997 == 0) v = NAN;
                        if (r % 991 == 1) v = (r & 8) ? INFINITY : -INFINITY;
                        if (r % 983 == 2) v = 3.4e38f;
                        if (i / n == 4) v = 1000.0f * sinf(0.479f * (float)(i % n)) * (float)((i / 264) & 1);
                        x[i] = v;
                    }
                    uhsdr_rtty_handle h;
                    if (uhsdr_rtty_create_host(C, shift, speed, stop, atc, 8, &h) != UHSDR_OK) return 1;
                    if (uhsdr_rtty_process_host(h, x, n, n) != UHSDR_OK) return 1;
                    if (uhsdr_rtty_reset(h) != UHSDR_OK) return 1;
                    for (int b = 0; b + 333 <= n; b += 333)
                        if (uhsdr_rtty_process_host(h, x + b, 333, n) != UHSDR_OK) return 1;
                    uint8_t* text; uint32_t* total;
                    uhsdr_rtty_outputs(h, &text, &total);
                    for (int c = 0; c < C; c++) chars += total[c];
                    uhsdr_rtty_destroy(h);
                }
    free(x);
    printf("wild input: 72 configurations, %lu characters\n", chars);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: rtty_sanitize <streams.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t hd[6];
        if (fread(hd, 4, 6, f) != 6) return 1;
        float* audio = malloc(sizeof(float) * (hd[4] ? hd[4] : 1));
        uint8_t* chars = malloc(hd[5] ? hd[5] : 1);
        if (fread(audio, 4, hd[4], f) != (size_t)hd[4] || fread(chars, 1, hd[5], f) != (size_t)hd[5]) return 1;
        const int b1 = run(audio, hd[4], hd, chars, hd[5], hd[4] ? hd[4] : 1, 1);
        const int b2 = run(audio, hd[4], hd, chars, hd[5], 97, 3);
        const int b3 = run(audio, hd[4], hd, chars, hd[5], 1, 1);
        printf("case %d: shift %d speed %d stop %d atc_disable %d, %d samples, %d chars: %s\n", k, hd[0], hd[1], hd[2], hd[3], hd[4],
               hd[5], b1 | b2 | b3 ? "MISMATCH" : "ok");
        bad |= b1 | b2 | b3;
        free(audio);
        free(chars);
    }
    fclose(f);
    bad |= wild();
    return bad;
}
