/*
 * Stand-alone driver of uhsdr_cwgen_process_host for a host sanitizer build (no device call):
 *
 *   make sanitize          (tools/sanitize.mk: builds cwgen_sanitize and runs it on what dump_cases.py writes)
 *
 * (linked with uhsdr_digimod.hip as well, which has the text queue's put.)  File: see dump_cases.py.  Every fixture runs with
 * one call between two events, in calls of 7 blocks as the middle one of three channels, and in
 * calls of one block, on exact-size rows; the block crc32s of I and Q, the flags, the characters
 * taken and the echo are compared.  Then every keyer mode runs with the smallest queue and echo
 * ring over pseudo-random key lines and bytes of all 256 values, put in pseudo-random pieces between
 * calls of pseudo-random length, with speed changes and resets thrown in.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr.h"

typedef struct { int32_t block, type, a, b; uint8_t* text; } event_t;
typedef struct
{
    int32_t mode, speed, weight, reverse, rx_delay, sidetone, capacity, blocks, events, echo_len;
    uint32_t consumed;
    uint8_t *keys, *flags, *echo;
    uint32_t *i_crc, *q_crc;
    event_t* ev;
} case_t;

static uint32_t crc32_of(const void* data, size_t n)
{
    const uint8_t* p = data;
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++)
    {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

/* the case on channel `at` of `channels`, at most per_call blocks per call; 0 if all is as recorded */
static int run(const case_t* c, int per_call, int channels, int at)
{
    const uhsdr_cwgen_config cfg = { c->mode, c->speed, c->weight, c->reverse, c->rx_delay, c->sidetone };
    uhsdr_cwgen_handle h;
    if (uhsdr_cwgen_create_host(channels, &cfg, c->capacity, c->echo_len > 8 ? c->echo_len : 8, &h) != UHSDR_OK) return 1;
    int32_t* len = calloc((size_t)channels, sizeof(int32_t));
    int bad = 0, e = 0;
    for (int b = 0; b < c->blocks;)
    {
        for (; e < c->events && c->ev[e].block == b; e++)
        {
            const event_t* ev = &c->ev[e];
            if (ev->type == 1) { bad |= uhsdr_cwgen_set_speed(h, ev->a, ev->b) != UHSDR_OK; continue; }
            uint8_t* rows = calloc((size_t)channels * (ev->a ? ev->a : 1), 1);      /* exact-size rows */
            memcpy(rows + (size_t)at * ev->a, ev->text, ev->a);
            len[at] = ev->a;
            bad |= uhsdr_cwgen_put_text(h, rows, len, ev->a, NULL) != UHSDR_OK;
            free(rows);
        }
        int m = c->blocks - b < per_call ? c->blocks - b : per_call;
        if (e < c->events && c->ev[e].block - b < m) m = c->ev[e].block - b;
        uint8_t* keys = calloc((size_t)channels * m, 1);
        float* i = malloc(sizeof(float) * (size_t)channels * 32 * m);
        float* q = malloc(sizeof(float) * (size_t)channels * 32 * m);
        memcpy(keys + (size_t)at * m, c->keys + b, (size_t)m);
        bad |= uhsdr_cwgen_process_host(h, keys, i, q, 32 * m, 32 * m) != UHSDR_OK;
        uint8_t* flags;
        bad |= uhsdr_cwgen_outputs(h, &flags, NULL, NULL, NULL, NULL) != UHSDR_OK;
        for (int k = 0; k < m; k++)
        {
            bad |= flags[(size_t)at * m + k] != c->flags[b + k];
            bad |= crc32_of(i + ((size_t)at * m + k) * 32, 128) != c->i_crc[b + k];
            bad |= crc32_of(q + ((size_t)at * m + k) * 32, 128) != c->q_crc[b + k];
        }
        free(keys);
        free(i);
        free(q);
        b += m;
    }
    uint32_t *consumed, *echo_total;
    uint8_t* echo;
    bad |= uhsdr_cwgen_outputs(h, NULL, &consumed, &echo, &echo_total, NULL) != UHSDR_OK;
    const int cap = c->echo_len > 8 ? c->echo_len : 8;
    bad |= consumed[at] != c->consumed || echo_total[at] != (uint32_t)c->echo_len;
    bad |= memcmp(echo + (size_t)at * cap, c->echo, (size_t)c->echo_len) != 0;
    uhsdr_cwgen_destroy(h);
    free(len);
    return bad;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(void)
{
    enum { C = 5, STRIDE = 12 };
    unsigned long took = 0, printed = 0;
    for (int mode = 0; mode < 4; mode++)
    {
        const uhsdr_cwgen_config cfg = { mode, 48, 50 + (int)(rng() % 101), (int)(rng() & 1), (int)(rng() % 3), 400 + (int)(rng() % 601) };
        uhsdr_cwgen_handle h;
        if (uhsdr_cwgen_create_host(C, &cfg, 8, 8, &h) != UHSDR_OK) return 1;
        for (int round = 0; round < 200; round++)
        {
            uint8_t text[C * STRIDE];
            int32_t len[C], acc[C];
            for (int i = 0; i < C * STRIDE; i++) text[i] = (uint8_t)(rng() >> 7);
            for (int i = 0; i < C; i++) len[i] = (int32_t)(rng() % (STRIDE + 1));
            if (uhsdr_cwgen_put_text(h, text, len, STRIDE, acc) != UHSDR_OK) return 1;
            for (int i = 0; i < C; i++) if (acc[i] < 0 || acc[i] > len[i] || acc[i] > 7) return 1;
            const int m = 1 + (int)(rng() % 400);
            uint8_t* keys = malloc((size_t)C * m);
            for (int i = 0; i < C; i++)
            {
                uint8_t line = 0;
                for (int k = 0; k < m; k++)
                {
                    if (rng() % 23 == 0) line = (i == 0) ? 0 : (uint8_t)(rng() & 0xff);       /* channel 0: text only; high bits are ignored */
                    keys[(size_t)i * m + k] = line;
                }
            }
            float* iq = malloc(sizeof(float) * 2 * C * 32 * (size_t)m);
            if (uhsdr_cwgen_process_host(h, keys, iq, iq + (size_t)C * 32 * m, 32 * m, 32 * m) != UHSDR_OK) return 1;
            free(iq);
            free(keys);
            if (rng() % 5 == 0 && uhsdr_cwgen_set_speed(h, 5 + (int)(rng() % 44), 50 + (int)(rng() % 101)) != UHSDR_OK) return 1;
            if (round == 120 && uhsdr_cwgen_reset(h) != UHSDR_OK) return 1;
        }
        uint32_t *consumed, *echo_total;
        uhsdr_cwgen_outputs(h, NULL, &consumed, NULL, &echo_total, NULL);
        for (int i = 0; i < C; i++) { took += consumed[i]; printed += echo_total[i]; }
        uhsdr_cwgen_destroy(h);
    }
    printf("wild keys and text: 4 keyer modes, %lu characters taken, %lu bytes echoed\n", took, printed);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: cwgen_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        case_t c;
        if (fread(&c.mode, 4, 10, f) != 10 || fread(&c.consumed, 4, 1, f) != 1) return 1;
        const size_t B = (size_t)c.blocks;
        c.keys = malloc(B); c.flags = malloc(B); c.i_crc = malloc(4 * B); c.q_crc = malloc(4 * B);
        c.echo = malloc((size_t)c.echo_len + 1);
        c.ev = calloc((size_t)c.events + 1, sizeof(event_t));
        if (fread(c.keys, 1, B, f) != B || fread(c.flags, 1, B, f) != B || fread(c.i_crc, 4, B, f) != B || fread(c.q_crc, 4, B, f) != B) return 1;
        if (fread(c.echo, 1, (size_t)c.echo_len, f) != (size_t)c.echo_len) return 1;
        for (int i = 0; i < c.events; i++)
        {
            if (fread(&c.ev[i].block, 4, 4, f) != 4) return 1;
            if (c.ev[i].type == 0)
            {
                c.ev[i].text = malloc((size_t)c.ev[i].a + 1);
                if (fread(c.ev[i].text, 1, (size_t)c.ev[i].a, f) != (size_t)c.ev[i].a) return 1;
            }
        }
        const int b1 = run(&c, c.blocks, 1, 0);
        const int b2 = run(&c, 7, 3, 1);
        const int b3 = run(&c, 1, 1, 0);
        printf("case %d: mode %d, %d blocks, %d events: %s\n", k, c.mode, c.blocks, c.events, b1 | b2 | b3 ? "MISMATCH" : "ok");
        bad |= b1 | b2 | b3;
        for (int i = 0; i < c.events; i++) free(c.ev[i].text);
        free(c.ev); free(c.echo); free(c.q_crc); free(c.i_crc); free(c.flags); free(c.keys);
    }
    fclose(f);
    bad |= wild();
    return bad;
}
