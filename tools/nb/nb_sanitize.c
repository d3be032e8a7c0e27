/*
 * Stand-alone driver of the noise blanker's host step functions (uhsdr_amd/csrc/uhsdr_nb.h, the text
 * the nb_frames kernel runs) for a host sanitizer build; plain C, no device call:
 *
 *   make sanitize          (tools/sanitize.mk: builds nb_sanitize and runs it on what dump_cases.py writes)
 *
 * File: see dump_cases.py.  Every frame case runs on a working buffer and a filtered frame that are
 * heap blocks of exactly 154 and 128 floats (so a step outside them is seen), once with the samples
 * next to each other and once 65 floats apart as the kernel has them; the output is compared with
 * the recording, a NaN equal to a NaN.  Then wild input at every setting: pseudo-random samples over
 * 38 decades with NaN, infinities and 3e38 in them, a silent run, a 1e-30 run and a tone with
 * impulses; here only the counts are printed.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr_nb.h"

/* `samples` of audio through the blanker with the buffers' samples `pitch` floats apart; the number
   of places repaired, or -1 when the output differs from `want` (null: not compared) */
static long run(const float* audio, const float* want, float* got, int samples, int setting, int pitch)
{
    float* wb = calloc((size_t)(NB_WB - 1) * pitch + 1, sizeof(float));
    float* ts = calloc((size_t)(NB_FRAME - 1) * pitch + 1, sizeof(float));
    long repaired = 0;
    int bad = 0;
    for (int f = 0; f + 1 <= samples / NB_FRAME; f++)
    {
        for (int i = 0; i < NB_FRAME; i++) wb[(NB_KEEP + i) * pitch] = audio[f * NB_FRAME + i];
        const int count = nb_frame(wb, pitch, ts, pitch, setting);
        if (count < 0 || count > NB_MAX_HITS) bad = 1;
        repaired += count;
        for (int i = 0; i < NB_FRAME; i++) got[f * NB_FRAME + i] = wb[(NB_LEAD + i) * pitch];
        for (int i = 0; i < NB_KEEP; i++) wb[i * pitch] = wb[(NB_FRAME + i) * pitch];
    }
    if (want)
        for (int i = 0; i < samples; i++)
            if (memcmp(&got[i], &want[i], 4) != 0 && !(got[i] != got[i] && want[i] != want[i])) bad = 1;
    free(wb);
    free(ts);
    return bad ? -1 : repaired;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(void)
{
    const int rows = 4, n = NB_FRAME * 40;
    float* x = malloc(sizeof(float) * rows * n);
    float* y = malloc(sizeof(float) * n);
    for (int i = 0; i < rows * n; i++)
    {
        const uint32_t r = rng();
        const int c = i / n, s = i % n;
        float v = ((int32_t)r / 2147483648.0f) * powf(10.0f, (float)(r % 39));
        if (r % 997 == 0) v = NAN;
        if (r % 991 == 1) v = (r & 8) ? INFINITY : -INFINITY;
        if (r % 983 == 2) v = 3.4e38f;
        if (c == 1) v = 0.0f;
        if (c == 2) v = 1e-30f * sinf(0.7f * (float)s);
        if (c == 3) v = 3000.0f * sinf(0.7f * (float)s) + ((int32_t)r / 2147483648.0f) * 300.0f + (r % 211 == 0 ? 25000.0f : 0.0f);
        x[i] = v;
    }
    long total = 0;
    for (int setting = 1; setting <= NB_MAX_SETTING; setting++)
        for (int c = 0; c < rows; c++)
        {
            const long k = run(x + (size_t)c * n, NULL, y, n, setting, c & 1 ? 65 : 1);
            if (k < 0) { printf("wild: row %d setting %d: a count outside 0 .. 5\n", c, setting); return 1; }
            if ((c == 1 || c == 2) && k != 0) { printf("wild: row %d setting %d: %ld repairs in silence\n", c, setting, k); return 1; }
            total += k;
        }
    free(x);
    free(y);
    printf("wild input: 4 rows x 15 settings, %ld places repaired\n", total);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nb_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        int32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 1;
        const int setting = head[0], samples = head[1];
        float* audio = malloc(sizeof(float) * samples);
        float* want = malloc(sizeof(float) * samples);
        float* got = malloc(sizeof(float) * samples);
        if (fread(audio, 4, samples, f) != (size_t)samples || fread(want, 4, samples, f) != (size_t)samples) return 1;
        const long a = run(audio, want, got, samples, setting, 1), b = run(audio, want, got, samples, setting, 65);
        printf("case %d: setting %d, %d samples, %ld places repaired: %s\n", k, setting, samples, a, a < 0 || b != a ? "MISMATCH" : "ok");
        bad |= a < 0 || b != a;
        free(audio);
        free(want);
        free(got);
    }
    fclose(f);
    bad |= wild();
    return bad;
}
