/*
 * Stand-alone driver of the signal meter's host step functions (uhsdr_amd/csrc/uhsdr_meter.h, the
 * text the meter_frames kernel and the spectrum kernel's epilogue run) for a host sanitizer build;
 * plain C, no device call:
 *
 *   make sanitize          (tools/sanitize.mk: builds meter_sanitize and runs it on what dump_cases.py writes)
 *
 * File: see dump_cases.py.  Every frame of every case runs from a heap block of exactly fft_len
 * floats (so a read outside the frame is seen) and the six outputs are compared with the recording,
 * a NaN equal to a NaN.  Then wild input: passbands at both ends of the frame and over all of it,
 * with SNAP on every frame, over pseudo-random magnitudes of 38 decades with NaN, infinities,
 * negative values and zeros in them, and the maximum forced into the first and the last bin.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr_meter.h"

static int same32(const void* a, const void* b, int is_float)
{
    if (!memcmp(a, b, 4)) return 1;
    if (!is_float) return 0;
    float x, y;
    memcpy(&x, a, 4);
    memcpy(&y, b, 4);
    return x != x && y != y;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(const uhsdr_meter_plan* base)
{
    static const int band[][2] = { { 0, 0 }, { 0, 1 }, { 0, -1 }, { -1, -1 }, { -2, -1 }, { 5, 5 }, { 100, 140 } };
    long frames = 0;
    for (int L = 256; L <= 512; L *= 2)
        for (unsigned b = 0; b < sizeof band / sizeof band[0]; b++)
        {
            uhsdr_meter_plan p = *base;
            p.fft_len = L;
            p.lbin = band[b][0] < 0 ? L + band[b][0] : band[b][0];
            p.ubin = band[b][1] < 0 ? L + band[b][1] : band[b][1];
            p.dbmhz_term = 10 * log10f_fast((float)((p.ubin - p.lbin) * p.bin_bw));       /* of 0 for the one-bin passbands */
            if (!(p.dbmhz_term == p.dbmhz_term) || isinf(p.dbmhz_term)) { printf("wild: dbmhz_term\n"); return 1; }
            p.snap = METER_SNAP_ALWAYS;
            meter_state s;
            meter_state_reset(&s);
            for (int f = 0; f < 200; f++)
            {
                float* mag = malloc(sizeof(float) * L);
                for (int i = 0; i < L; i++)
                {
                    const uint32_t r = rng();
                    float v = (r / 4294967296.0f) * powf(10.0f, (float)(r % 39) - 8.0f);
                    if (r % 97 == 0) v = NAN;
                    if (r % 89 == 1) v = INFINITY;
                    if (r % 83 == 2) v = -v;
                    if (r % 7 == 3) v = 0.0f;
                    mag[i] = v;
                }
                if (f % 5 == 1) mag[meter_bin(L, p.lbin)] = 3e38f;          /* the maximum in the passband's first bin */
                if (f % 5 == 2) mag[meter_bin(L, p.ubin)] = 3e38f;          /* and in its last, which may be the frame's */
                if (f % 5 == 3) memset(mag, 0, sizeof(float) * L);
                meter_frame(&p, &s, mag, 1);
                free(mag);
                if (s.s_count < 1 || s.s_count > METER_S_SIZE) { printf("wild: s_count %d\n", s.s_count); return 1; }
                frames++;
            }
        }
    printf("wild input: %ld frames\n", frames);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: meter_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    uhsdr_meter_plan plan;
    memset(&plan, 0, sizeof plan);
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t head[4];
        if (fread(head, 4, 4, f) != 4) return 1;
        const int C = head[1], F = head[2], L = head[3];
        if (head[0] != (int32_t)sizeof plan || fread(&plan, sizeof plan, 1, f) != 1 || L != plan.fft_len) { fprintf(stderr, "case %d: plan\n", k); return 1; }
        const size_t n = (size_t)C * F;
        float* mag = malloc(sizeof(float) * n * L);
        uint8_t* cw = malloc(n);
        uint32_t* want = malloc(4 * 6 * n);
        if (fread(mag, 4, n * L, f) != n * L || fread(cw, 1, n, f) != n || fread(want, 4, 6 * n, f) != 6 * n) return 1;
        long wrong = 0;
        for (int c = 0; c < C; c++)
        {
            meter_state s;
            meter_state_reset(&s);
            for (int fr = 0; fr < F; fr++)
            {
                const size_t at = (size_t)c * F + fr;
                float* frame = malloc(sizeof(float) * L);
                memcpy(frame, mag + at * L, sizeof(float) * L);
                meter_frame(&plan, &s, frame, cw[at]);
                free(frame);
                const void* got[6] = { &s.dbm_cur, &s.dbmhz_cur, &s.dbm, &s.dbmhz, &s.s_count, &s.snap };
                for (int o = 0; o < 6; o++) wrong += !same32(got[o], &want[o * n + at], o < 4);
            }
        }
        printf("case %d: %d channels x %d frames of %d: %s\n", k, C, F, L, wrong ? "MISMATCH" : "ok");
        bad |= wrong != 0;
        free(mag);
        free(cw);
        free(want);
    }
    fclose(f);
    if (cases < 1) return 1;
    bad |= wild(&plan);
    return bad;
}
