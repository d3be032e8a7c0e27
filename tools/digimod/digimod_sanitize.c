/*
 * Stand-alone driver of uhsdr_rttymod_process_host / uhsdr_pskmod_process_host for a host sanitizer
 * build (no device call):
 *
 *   make sanitize          (tools/sanitize.mk: builds digimod_sanitize and runs it on what dump_cases.py writes)
 *
 * File: see dump_cases.py.  Every fixture runs in one piece, in calls of 97 samples as the middle
 * one of three channels (the other two without text), in calls of 23 and, up to 70000 samples, of 1,
 * on exact-size rows; the block crc32s and the outputs are compared.  Then every parameter set runs
 * with the smallest queue over pseudo-random bytes of all 256 values, put in pseudo-random pieces
 * between calls of pseudo-random length, with StartTX / PrepareTx and resets thrown in.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uhsdr.h"

enum { OP_PUT, OP_GEN, OP_START };
typedef struct { int32_t type, arg; uint8_t* text; } op_t;
typedef struct { int32_t kind, shift, speed, stop, cap, total, blocks, ops; uint32_t last[3]; uint32_t* crc; op_t* op; } case_t;

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

/* the two modulators behind one set of calls */
typedef struct { int psk; uhsdr_rttymod_handle r; uhsdr_pskmod_handle p; } mod_t;

static int mod_create(mod_t* m, const case_t* c, int channels, int cap)
{
    m->psk = c->kind;
    return m->psk ? uhsdr_pskmod_create_host(channels, c->speed, cap, &m->p)
                  : uhsdr_rttymod_create_host(channels, c->shift, c->speed, c->stop, cap, &m->r);
}
static int mod_put(mod_t* m, const uint8_t* t, const int32_t* len, int stride, int32_t* acc)
{ return m->psk ? uhsdr_pskmod_put_text(m->p, t, len, stride, acc) : uhsdr_rttymod_put_text(m->r, t, len, stride, acc); }
static int mod_gen(mod_t* m, int16_t* a, int n, int stride)
{ return m->psk ? uhsdr_pskmod_process_host(m->p, a, n, stride) : uhsdr_rttymod_process_host(m->r, a, n, stride); }
static int mod_start(mod_t* m) { return m->psk ? uhsdr_pskmod_prepare_tx(m->p) : uhsdr_rttymod_start_tx(m->r); }
static int mod_reset(mod_t* m) { return m->psk ? uhsdr_pskmod_reset(m->p) : uhsdr_rttymod_reset(m->r); }
static int mod_out(mod_t* m, uint32_t** a, uint32_t** b, uint8_t** s)
{ return m->psk ? uhsdr_pskmod_outputs(m->p, a, b, s) : uhsdr_rttymod_outputs(m->r, a, b, s); }
static void mod_destroy(mod_t* m) { if (m->psk) uhsdr_pskmod_destroy(m->p); else uhsdr_rttymod_destroy(m->r); }

/* the case on channel `at` of `channels`, at most per_call samples per call; 0 if all is as recorded */
static int run(const case_t* c, int per_call, int channels, int at)
{
    mod_t m;
    if (mod_create(&m, c, channels, c->cap) != UHSDR_OK) return 1;
    int16_t* all = malloc(sizeof(int16_t) * (size_t)(c->total ? c->total : 1));
    int32_t* len = calloc((size_t)channels, sizeof(int32_t));
    int done = 0, bad = 0;
    for (int k = 0; k < c->ops; k++)
    {
        const op_t* op = &c->op[k];
        if (op->type == OP_PUT)
        {
            uint8_t* rows = calloc((size_t)channels * (op->arg ? op->arg : 1), 1);      /* exact-size rows */
            memcpy(rows + (size_t)at * op->arg, op->text, op->arg);
            len[at] = op->arg;
            bad |= mod_put(&m, rows, len, op->arg, NULL) != UHSDR_OK;
            free(rows);
        }
        else if (op->type == OP_START) bad |= mod_start(&m) != UHSDR_OK;
        else
            for (int b = 0; b < op->arg; b += per_call)
            {
                const int n = op->arg - b < per_call ? op->arg - b : per_call;
                int16_t* rows = malloc(sizeof(int16_t) * (size_t)channels * n);
                bad |= mod_gen(&m, rows, n, n) != UHSDR_OK;
                memcpy(all + done, rows + (size_t)at * n, sizeof(int16_t) * n);
                done += n;
                free(rows);
            }
    }
    for (int b = 0; b < c->blocks; b++)
    {
        const int n = c->total - b * 1024 < 1024 ? c->total - b * 1024 : 1024;
        bad |= crc32_of(all + b * 1024, sizeof(int16_t) * n) != c->crc[b];
    }
    uint32_t *consumed, *txoff;
    uint8_t* state;
    bad |= mod_out(&m, &consumed, &txoff, &state) != UHSDR_OK;
    bad |= consumed[at] != c->last[0] || txoff[at] != c->last[1] || state[at] != c->last[2];
    mod_destroy(&m);
    free(all);
    free(len);
    return bad;
}

static uint32_t rng_state = 2463534242u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int wild(void)
{
    enum { C = 5, STRIDE = 12 };
    unsigned long took = 0, sets = 0;
    for (int kind = 0; kind < 2; kind++)
        for (int shift = 0; shift < (kind ? 1 : 6); shift++)
            for (int speed = 0; speed < (kind ? 3 : 2); speed++)
                for (int stop = 0; stop < (kind ? 1 : 3); stop++)
                {
                    const case_t c = { .kind = kind, .shift = shift, .speed = speed, .stop = stop };
                    mod_t m;
                    if (mod_create(&m, &c, C, 8) != UHSDR_OK) return 1;
                    for (int round = 0; round < 60; round++)
                    {
                        uint8_t text[C * STRIDE];
                        int32_t len[C], acc[C];
                        for (int i = 0; i < C * STRIDE; i++) text[i] = (uint8_t)(rng() >> 7);
                        for (int i = 0; i < C; i++) len[i] = (int32_t)(rng() % (STRIDE + 1));
                        if (rng() % 4 == 0) text[rng() % (C * STRIDE)] = 4;      /* EOT */
                        if (mod_put(&m, text, len, STRIDE, acc) != UHSDR_OK) return 1;
                        for (int i = 0; i < C; i++) if (acc[i] < 0 || acc[i] > len[i] || acc[i] > 7) return 1;
                        const int n = 1 + (int)(rng() % 40000);
                        int16_t* rows = malloc(sizeof(int16_t) * C * (size_t)n);
                        if (mod_gen(&m, rows, n, n) != UHSDR_OK) return 1;
                        free(rows);
                        if (rng() % 5 == 0 && mod_start(&m) != UHSDR_OK) return 1;
                        if (round == 40 && mod_reset(&m) != UHSDR_OK) return 1;
                    }
                    uint32_t* consumed;
                    mod_out(&m, &consumed, NULL, NULL);
                    for (int i = 0; i < C; i++) took += consumed[i];
                    mod_destroy(&m);
                    sets++;
                }
    printf("wild text: %lu parameter sets, %lu characters taken\n", sets, took);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: digimod_sanitize <cases.bin>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t cases = 0, bad = 0;
    if (fread(&cases, 4, 1, f) != 1) return 1;
    for (int k = 0; k < cases; k++)
    {
        case_t c;
        if (fread(&c.kind, 4, 8, f) != 8 || fread(c.last, 4, 3, f) != 3) return 1;
        c.crc = malloc(sizeof(uint32_t) * (size_t)(c.blocks ? c.blocks : 1));
        c.op = calloc((size_t)(c.ops ? c.ops : 1), sizeof(op_t));
        if (fread(c.crc, 4, (size_t)c.blocks, f) != (size_t)c.blocks) return 1;
        for (int i = 0; i < c.ops; i++)
        {
            if (fread(&c.op[i].type, 4, 2, f) != 2) return 1;
            if (c.op[i].type == OP_PUT)
            {
                c.op[i].text = malloc((size_t)(c.op[i].arg ? c.op[i].arg : 1));
                if (fread(c.op[i].text, 1, (size_t)c.op[i].arg, f) != (size_t)c.op[i].arg) return 1;
            }
        }
        const int b1 = run(&c, c.total ? c.total : 1, 1, 0);
        const int b2 = run(&c, 97, 3, 1);
        const int b3 = run(&c, 23, 1, 0);
        const int b4 = c.total <= 70000 ? run(&c, 1, 1, 0) : 0;
        printf("case %d: %s, %d samples, %d ops: %s\n", k, c.kind ? "psk" : "rtty", c.total, c.ops, b1 | b2 | b3 | b4 ? "MISMATCH" : "ok");
        bad |= b1 | b2 | b3 | b4;
        for (int i = 0; i < c.ops; i++) free(c.op[i].text);
        free(c.op);
        free(c.crc);
    }
    fclose(f);
    bad |= wild();
    return bad;
}
