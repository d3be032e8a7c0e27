/*
 * Stand-alone driver of uhsdr_psk_process_host for a host sanitizer build (no device call):
 *
 *   make sanitize          (tools/sanitize.mk: builds psk_sanitize and runs it on what dump_streams.py writes)
 *
 * File: see dump_streams.py.  Every case runs in one piece and in calls of 1, 23 and 97 samples,
 * alone and as one of three channels, on exact-size rows, and the text is compared.  Then every
 * speed runs over the kind of rows the device tests use: BPSK with gaps of zeros, pseudo-random
 * input over 38 decades with NaN, infinities and a 3e38 run in it, and a 1e-26 row, with the
 * smallest text ring, in one piece and after a reset in calls of 333.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr.h"

static int run(const float* audio, int samples, int speed, const uint8_t* chars, int nchars, int per_call, int channels)
{
    uhsdr_psk_handle h;
    const int cap = 4096;
    if (uhsdr_psk_create_host(channels, speed, cap, &h) != UHSDR_OK) return 1;
    float* rows = malloc(sizeof(float) * (size_t)channels * per_call);
    for (int b = 0; b < samples; b += per_call)
    {
        const int n = samples - b < per_call ? samples - b : per_call;
        for (int c = 0; c < channels; c++) memcpy(rows + (size_t)c * n, audio + b, sizeof(float) * n);     /* exact-size rows */
        if (uhsdr_psk_process_host(h, rows, n, n) != UHSDR_OK) return 1;
    }
    free(rows);
    uint8_t* text; uint32_t* total; float* symbol;
    uhsdr_psk_outputs(h, &text, &total, &symbol);
    int bad = 0;
    for (int c = 0; c < channels; c++)
        bad |= (int)total[c] != nchars || memcmp(text + (size_t)c * cap, chars, nchars) != 0 ||
               memcmp(symbol + c, symbol, sizeof(float)) != 0;
    uhsdr_psk_destroy(h);
    return bad;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(void)
{
    const int C = 6, n = 24000;
    float* x = malloc(sizeof(float) * C * n);
    unsigned long chars = 0;
    for (int speed = 0; speed < 3; speed++)
    {
        for (int i = 0; i < C * n; i++)
        {
            const uint32_t r = rng();
            const int c = i / n, s = i % n;
            float v = ((int32_t)r / 2147483648.0f) * powf(10.0f, (float)(r % 39));
            if (r % 997 == 0) v = NAN;
            if (r % 991 == 1) v = (r & 8) ? INFINITY : -INFINITY;
            if (r % 983 == 2) v = 3.4e38f;
            /* rows 3 .. 5: a 500 Hz carrier reversed every 96 samples, with a gap of zeros; a 3e38 run; at 1e-26 */
            const float bpsk = sinf(6.2831853f * 500.0f / 12000.0f * (float)s) * (float)(1 - 2 * ((s / 96) % 3 == 0));
            if (c == 3) v = (s >= 15000 && s < 21000) ? 0.0f : 1000.0f * bpsk;
            if (c == 4) v = (s >= 5000 && s < 5100) ? 3.0e38f : 1000.0f * bpsk;
            if (c == 5) v = 1e-26f * bpsk;
            x[i] = v;
        }
        uhsdr_psk_handle h;
        if (uhsdr_psk_create_host(C, speed, 8, &h) != UHSDR_OK) return 1;
        if (uhsdr_psk_process_host(h, x, n, n) != UHSDR_OK) return 1;
        if (uhsdr_psk_reset(h) != UHSDR_OK) return 1;
        for (int b = 0; b + 333 <= n; b += 333)
            if (uhsdr_psk_process_host(h, x + b, 333, n) != UHSDR_OK) return 1;
        uint8_t* text; uint32_t* total;
        uhsdr_psk_outputs(h, &text, &total, NULL);
        for (int c = 0; c < C; c++) chars += total[c];
        uhsdr_psk_destroy(h);
    }
    free(x);
    printf("wild input: 3 speeds, %lu characters\n", chars);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: psk_sanitize <streams.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t hd[3];
        if (fread(hd, 4, 3, f) != 3) return 1;
        float* audio = malloc(sizeof(float) * (hd[1] ? hd[1] : 1));
        uint8_t* chars = malloc(hd[2] ? hd[2] : 1);
        if (fread(audio, 4, hd[1], f) != (size_t)hd[1] || fread(chars, 1, hd[2], f) != (size_t)hd[2]) return 1;
        const int b1 = run(audio, hd[1], hd[0], chars, hd[2], hd[1] ? hd[1] : 1, 1);
        const int b2 = run(audio, hd[1], hd[0], chars, hd[2], 97, 3);
        const int b3 = run(audio, hd[1], hd[0], chars, hd[2], 23, 1);
        const int b4 = hd[1] <= 70000 ? run(audio, hd[1], hd[0], chars, hd[2], 1, 1) : 0;
        printf("case %d: speed %d, %d samples, %d chars: %s\n", k, hd[0], hd[1], hd[2], b1 | b2 | b3 | b4 ? "MISMATCH" : "ok");
        bad |= b1 | b2 | b3 | b4;
        free(audio);
        free(chars);
    }
    fclose(f);
    bad |= wild();
    return bad;
}
