/*
 * Stand-alone driver of the display stage's host step functions (uhsdr_amd/csrc/uhsdr_display.h, the
 * text the display_frames kernel and the spectrum kernel's epilogue run) for a host sanitizer build;
 * plain C, no device call:
 *
 *   make sanitize          (tools/sanitize.mk: builds display_sanitize and runs it on what dump_cases.py writes)
 *
 * File: see dump_cases.py.  Every frame of every case runs from heap blocks of exactly fft_len floats
 * for the average and for the scaled row and of exactly width columns for the two outputs (so a read
 * or write outside them is seen), and the four outputs are compared with the recording, a NaN equal
 * to a NaN.  Then wild input: every accepted width of both lengths, walked with the plan's tables
 * rebuilt here the way uhsdr_display_plan_build builds them, over pseudo-random averages of 38
 * decades with NaN, infinities, negative values and zeros in them and an edge of the same kind.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr_display.h"

static int same32(const void* a, const void* b)
{
    if (!memcmp(a, b, 4)) return 1;
    float x, y;
    memcpy(&x, a, 4);
    memcpy(&y, b, 4);
    return x != x && y != y;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static float wild_value(void)
{
    const uint32_t r = rng();
    float v = (r / 4294967296.0f) * powf(10.0f, (float)(r % 39) - 8.0f);
    if (r % 97 == 0) v = NAN;
    if (r % 89 == 1) v = INFINITY;
    if (r % 83 == 2) v = -v;
    if (r % 7 == 3) v = 0.0f;
    return v;
}

/* the walk as uhsdr_display_plan_build runs it (uhsdr_setup.c); 1: the width is refused there */
static int walk(uhsdr_display_plan* p)
{
    const int L = p->fft_len, W = p->width;
    float amount = p->full_amount = (float)L / (float)W;
    int idx_old = 0;
    p->reads_edge = 0;
    for (int x = 0; x < W; x++)
    {
        int n = 0;
        if (idx_old < x) return 1;
        p->first[x] = (uint16_t)idx_old;
        while (amount >= 1) { idx_old++; n++; amount = (float)((double)amount - 1.0); }
        if (n > 2 || idx_old > L) return 1;
        p->whole[x] = (uint8_t)n;
        p->amount[x] = amount;
        if (idx_old == L) p->reads_edge = 1;
        if (x + 1 < W) { idx_old++; amount = p->full_amount - (1 - amount); }
    }
    return 0;
}

static int wild(const uhsdr_display_plan* base)
{
    long frames = 0, edges = 0;
    for (int L = 256; L <= 512; L *= 2)
        for (int W = L / 2; W <= L; W++)
        {
            uhsdr_display_plan p = *base;
            p.fft_len = L;
            p.width = W;
            p.resample = W != L;
            p.limit = (int32_t)(rng() % 70000);
            if (p.resample && walk(&p)) { printf("wild: %d -> %d refused\n", L, W); return 1; }
            edges += p.reads_edge;
            float offset = DISPLAY_OFFSET_INIT;
            for (int f = 0; f < 3; f++)
            {
                float* avg = malloc(sizeof(float) * L);
                float* row = malloc(sizeof(float) * L);
                uint16_t* scope = malloc(sizeof(uint16_t) * W);
                uint8_t* wfall = malloc(W);
                for (int i = 0; i < L; i++) avg[i] = f == 2 ? 1.0f + (float)(rng() % 1000) : wild_value();
                display_frame(&p, &offset, avg, wild_value(), row, scope, wfall);
                free(avg);
                free(row);
                free(scope);
                free(wfall);
                frames++;
            }
        }
    printf("wild input: %ld frames, %ld widths read the edge\n", frames, edges);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: display_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    static uhsdr_display_plan plan;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t head[5];
        if (fread(head, 4, 5, f) != 5) return 1;
        const int C = head[1], F = head[2], L = head[3], W = head[4];
        if (head[0] != (int32_t)sizeof plan || fread(&plan, sizeof plan, 1, f) != 1 || L != plan.fft_len || W != plan.width)
        { fprintf(stderr, "case %d: plan\n", k); return 1; }
        const size_t n = (size_t)C * F;
        float* avg = malloc(sizeof(float) * n * L);
        float* edge = malloc(sizeof(float) * n);
        uint16_t* want_scope = malloc(sizeof(uint16_t) * n * W);
        uint8_t* want_wfall = malloc(n * W);
        float* want_tail = malloc(sizeof(float) * 2 * n);
        if (fread(avg, 4, n * L, f) != n * L || fread(edge, 4, n, f) != n || fread(want_scope, 2, n * W, f) != n * W
            || fread(want_wfall, 1, n * W, f) != n * W || fread(want_tail, 4, 2 * n, f) != 2 * n) return 1;
        long wrong = 0;
        for (int c = 0; c < C; c++)
        {
            float offset = DISPLAY_OFFSET_INIT;
            for (int fr = 0; fr < F; fr++)
            {
                const size_t at = (size_t)c * F + fr;
                float* frame = malloc(sizeof(float) * L);
                float* row = malloc(sizeof(float) * L);
                uint16_t* scope = malloc(sizeof(uint16_t) * W);
                uint8_t* wfall = malloc(W);
                memcpy(frame, avg + at * L, sizeof(float) * L);
                const float min1 = display_frame(&plan, &offset, frame, plan.reads_edge ? edge[at] : 0.0f, row, scope, wfall);
                wrong += memcmp(scope, want_scope + at * W, sizeof(uint16_t) * W) != 0;
                wrong += memcmp(wfall, want_wfall + at * W, W) != 0;
                wrong += !same32(&offset, &want_tail[at]) + !same32(&min1, &want_tail[n + at]);
                free(frame);
                free(row);
                free(scope);
                free(wfall);
            }
        }
        printf("case %d: %d channels x %d frames of %d -> %d: %s\n", k, C, F, L, W, wrong ? "MISMATCH" : "ok");
        bad |= wrong != 0;
        free(avg);
        free(edge);
        free(want_scope);
        free(want_wfall);
        free(want_tail);
    }
    fclose(f);
    if (cases < 1) return 1;
    bad |= wild(&plan);
    return bad;
}
