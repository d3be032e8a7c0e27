/*
 * Stand-alone driver of uhsdr_nr_process_frames_host / uhsdr_nr_process_host for a host sanitizer
 * build (no device call):
 *
 *   make sanitize          (tools/sanitize.mk: builds nr_sanitize and runs it on what dump_cases.py writes)
 *
 * File: see dump_cases.py.  Every frame case runs in one piece and in calls of 1, 3 and 21 frames,
 * alone and as one of three channels on rows longer than the run; every stream case in one piece and
 * in calls of 8, 136 and 1000 samples; the output is compared with the recording.  Then wild input:
 * pseudo-random samples over 38 decades with NaN, infinities and 3e38 in them, a silent row and a
 * 1e-30 row, through the frames and the stream of the narrowest and the widest accepted band and of
 * the empty one, with a reset in between.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr.h"

static int run_frames(const uhsdr_nr_config* cfg, const float* audio, const float* want, int samples, int reset, int per_call, int channels)
{
    uhsdr_nr_handle h;
    if (uhsdr_nr_create_host(channels, cfg, &h) != UHSDR_OK) return 1;
    const int frames = samples / 128, stride = samples + 40;
    float* in = calloc((size_t)channels * stride, sizeof(float));
    float* out = calloc((size_t)channels * stride, sizeof(float));
    for (int c = 0; c < channels; c++) memcpy(in + (size_t)c * stride, audio, sizeof(float) * samples);
    for (int f = 0; f < frames;)
    {
        int k = frames - f < per_call ? frames - f : per_call;
        if (reset > f && reset < f + k) k = reset - f;
        if (f == reset && uhsdr_nr_reset(h) != UHSDR_OK) return 1;
        if (uhsdr_nr_process_frames_host(h, in + f * 128, out + f * 128, k, stride) != UHSDR_OK) return 1;
        f += k;
    }
    int bad = 0;
    for (int c = 0; c < channels; c++) bad |= memcmp(out + (size_t)c * stride, want, sizeof(float) * samples) != 0;
    int32_t ft[3];
    bad |= uhsdr_nr_state(h, ft, NULL, NULL) != UHSDR_OK || ft[0] != 3;
    free(in);
    free(out);
    uhsdr_nr_destroy(h);
    return bad;
}

static int run_stream(const uhsdr_nr_config* cfg, const float* audio, const float* want, int samples, int per_call, int channels)
{
    uhsdr_nr_handle h;
    if (uhsdr_nr_create_host(channels, cfg, &h) != UHSDR_OK) return 1;
    float* in = malloc(sizeof(float) * (size_t)channels * per_call);
    float* out = malloc(sizeof(float) * (size_t)channels * per_call);
    int bad = 0;
    for (int b = 0; b < samples; b += per_call)
    {
        const int n = samples - b < per_call ? samples - b : per_call;
        for (int c = 0; c < channels; c++) memcpy(in + (size_t)c * n, audio + b, sizeof(float) * n);       /* exact-size rows */
        if (uhsdr_nr_process_host(h, in, out, n, n) != UHSDR_OK) return 1;
        for (int c = 0; c < channels; c++) bad |= memcmp(out + (size_t)c * n, want + b, sizeof(float) * n) != 0;
    }
    free(in);
    free(out);
    uhsdr_nr_destroy(h);
    return bad;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(void)
{
    const int C = 5, n = 128 * 60;
    float* x = malloc(sizeof(float) * C * n);
    float* y = malloc(sizeof(float) * C * n);
    for (int i = 0; i < C * n; i++)
    {
        const uint32_t r = rng();
        const int c = i / n, s = i % n;
        float v = ((int32_t)r / 2147483648.0f) * powf(10.0f, (float)(r % 39));
        if (r % 997 == 0) v = NAN;
        if (r % 991 == 1) v = (r & 8) ? INFINITY : -INFINITY;
        if (r % 983 == 2) v = 3.4e38f;
        if (c == 2) v = 0.0f;
        if (c == 3) v = 1e-30f * sinf(0.7f * (float)s);
        if (c == 4) v = 3000.0f * sinf(0.7f * (float)s) + ((int32_t)r / 2147483648.0f) * 300.0f;
        x[i] = v;
    }
    const int bands[4][3] = { { 200, 300, 6000 }, { 200, 2830, 6000 }, { 6000, 3000, 12000 }, { 2700, 1000, 6000 } };
    int nn_sum = 0;
    for (int b = 0; b < 4; b++)
        for (int width = 1; width <= 5; width += 3)
        {
            uhsdr_nr_config cfg;
            uhsdr_nr_config_default(&cfg);
            cfg.width_hz = bands[b][0];
            cfg.offset_hz = bands[b][1];
            cfg.sample_rate = bands[b][2];
            cfg.width = width;
            cfg.alpha = uhsdr_nr_alpha_from_strength(b * 60 + 1);
            uhsdr_nr_handle h;
            if (uhsdr_nr_create_host(C, &cfg, &h) != UHSDR_OK) { printf("wild: band %d width %d refused\n", b, width); return 1; }
            if (uhsdr_nr_process_frames_host(h, x, y, 60, n) != UHSDR_OK) return 1;
            int32_t nn[5];
            uhsdr_nr_state(h, NULL, nn, NULL);
            for (int c = 0; c < C; c++) nn_sum += nn[c];
            if (uhsdr_nr_reset(h) != UHSDR_OK) return 1;
            for (int at = 0; at + 1000 <= n; at += 1000)
                if (uhsdr_nr_process_host(h, x + at, y + at, 1000, n) != UHSDR_OK && at == 0)
                    printf("wild: band %d: the stream's own rate refuses it\n", b);
            uhsdr_nr_destroy(h);
        }
    free(x);
    free(y);
    printf("wild input: 4 bands x 2 widths, NN sum %d\n", nn_sum);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nr_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t kind, w[6], tail[2];
        float alpha;
        if (fread(&kind, 4, 1, f) != 1 || fread(&alpha, 4, 1, f) != 1 || fread(w, 4, 6, f) != 6 || fread(tail, 4, 2, f) != 2) return 1;
        uhsdr_nr_config cfg;
        uhsdr_nr_config_default(&cfg);
        cfg.alpha = alpha;
        cfg.asnr = w[0]; cfg.width = w[1]; cfg.power_threshold_int = w[2];
        cfg.width_hz = w[3]; cfg.offset_hz = w[4]; cfg.sample_rate = w[5];
        const int samples = tail[0], reset = tail[1];
        float* audio = malloc(sizeof(float) * samples);
        float* want = malloc(sizeof(float) * samples);
        if (fread(audio, 4, samples, f) != (size_t)samples || fread(want, 4, samples, f) != (size_t)samples) return 1;
        int b = 0;
        if (kind == 0)
        {
            b |= run_frames(&cfg, audio, want, samples, reset, samples / 128, 1);
            b |= run_frames(&cfg, audio, want, samples, reset, 1, 1);
            b |= run_frames(&cfg, audio, want, samples, reset, 3, 3);
            b |= run_frames(&cfg, audio, want, samples, reset, 21, 1);
        }
        else
        {
            b |= run_stream(&cfg, audio, want, samples, samples, 1);
            b |= run_stream(&cfg, audio, want, samples, 8, 1);
            b |= run_stream(&cfg, audio, want, samples, 136, 3);
            b |= run_stream(&cfg, audio, want, samples, 1000, 1);
        }
        printf("case %d: %s, %d samples, band %d +- %d Hz at %d: %s\n", k, kind ? "stream" : "frames", samples, cfg.offset_hz, cfg.width_hz / 2,
               cfg.sample_rate, b ? "MISMATCH" : "ok");
        bad |= b;
        free(audio);
        free(want);
    }
    fclose(f);
    bad |= wild();
    return bad;
}
