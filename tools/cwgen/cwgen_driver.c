/*
 * Fixture recorder for the CW generator (tests/golden/cwgen_*.npz), stand-alone cases.
 *
 * Linked with the reference firmware's objects as oracle/ref/Makefile builds them (cwgen.mk),
 * without the harness' main.  The harness' empty key-line, text-ring, TX-request and text-output
 * hooks are re-routed with -Wl,--wrap to the ones below, so the reference's CwGen_Process runs
 * against key lines, a text ring and an echo log this program owns.  Nothing of this program or its
 * output other than the recorded data is committed.
 *
 *   cwgen_driver gen mode speed weight reverse rx_delay sidetone capacity <ops.txt> <out.bin>
 *   cwgen_driver tables nchars nsigns <out.bin>
 *
 * gen: the firmware is in TX in DEMOD_CW without text entry, the ring's consumer is CW.  CwGen_Init
 * and AudioManagement_SetSidetoneForDemodMode run once, then the ops, one per line:
 *   put <hex bytes>      append to the ring what fits; prints "accepted <k>"
 *   speed <wpm> <weight> ts.cw_keyer_speed / weight and CwGen_SetSpeed
 *   blk <lines> <count>  count calls of CwGen_Process over 32 samples with the key lines at <lines>
 *                        (bit 0 DIT, bit 1 DAH/PTT); in the first block where a line has closed
 *                        CwGen_DitIRQ runs first, as the EXTI interrupt would
 * Every block appends to <out.bin> six uint32 (flags: bit 0 the return value, bit 1 TxOn requested,
 * bit 2 TxOff requested; cw_state, key_timer, sm_tbl_ptr, port_state, the DDS accumulator) and the
 * block's I and Q, 32 floats each, zeros where CwGen_Process returned false.  At the end:
 * "end <consumed> <echo as hex>".  consumed counts the characters removed and those discarded by
 * DigiModes_TxBufferReset.
 *
 * tables: writes nchars, nsigns, cw_char_codes, cw_char_chars, cw_sign_codes, the two letters of
 * each cw_sign_chars, and sm_table.  sm_table is private to cw_gen.c; it is read through the
 * straight key's rising edge with softdds_runIQ re-routed to produce 1.0, so that every output
 * sample is one table entry.  The counts come from the symbols' sizes (make_cwgen_golden.py).
 *
 * The ring is the firmware's (uhsdr_digi_buffer.c) with the capacity an argument: one slot stays free.
 */
#include "uhsdr_board.h"
#include "cw_gen.h"
#include "softdds.h"
#include "audio_management.h"
#include "uhsdr_digi_buffer.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* cw_gen.c's public state, whose type it keeps to itself: thirteen 32-bit words */
enum { PS_PORT = 0, PS_STATE, PS_DIT, PS_DAH, PS_PAUSE, PS_SPACE, PS_KEY_TIMER, PS_BREAK_TIMER, PS_SPACE_TIMER, PS_SM_PTR, PS_ULTIM, PS_CHAR, PS_SENDING, PS_WORDS };
extern struct { uint32_t w[PS_WORDS]; } ps;
extern soft_dds_t dbldds[2];
extern const uint32_t cw_char_codes[], cw_sign_codes[];
extern const char cw_char_chars[];
extern const char* cw_sign_chars[];

static uint8_t* ring;
static int capacity, head, tail, lines, ones;
static unsigned long consumed;
static unsigned flags;
static uint8_t echo[1 << 16];
static int echoed;

bool __wrap_Board_DitLinePressed(void) { return (lines & 1) != 0; }
bool __wrap_Board_PttDahLinePressed(void) { return (lines & 2) != 0; }
void __wrap_RadioManagement_Request_TxOn(void) { flags |= 2; }
void __wrap_RadioManagement_Request_TxOff(void) { flags |= 4; }
void __wrap_UiDriver_TextMsgPutChar(char ch) { if (echoed < (int)sizeof echo) echo[echoed++] = (uint8_t)ch; }

bool __wrap_DigiModes_TxBufferRemove(uint8_t* c_ptr, digi_buff_consumer_t consumer)
{
    if (consumer != CW || head == tail) return false;
    *c_ptr = ring[tail];
    tail = (tail + 1) % capacity;
    consumed++;
    return true;
}

/* source and consumer are both CW: printed, not queued */
int32_t __wrap_DigiModes_TxBufferPutChar(uint8_t c, digi_buff_consumer_t source)
{
    (void)source;
    __wrap_UiDriver_TextMsgPutChar((char)c);
    return 0;
}

void __wrap_DigiModes_TxBufferPutSign(const char* s, digi_buff_consumer_t source)
{
    __wrap_DigiModes_TxBufferPutChar('<', source);
    __wrap_DigiModes_TxBufferPutChar((uint8_t)s[0], source);
    __wrap_DigiModes_TxBufferPutChar((uint8_t)s[1], source);
    __wrap_DigiModes_TxBufferPutChar('>', source);
}

/* the harness has none: the ring is emptied */
void DigiModes_TxBufferReset(void)
{
    consumed += (unsigned long)((head - tail + capacity) % capacity);
    tail = head;
}

void __real_softdds_runIQ(float32_t* i_buff, float32_t* q_buff, uint16_t size);
void __wrap_softdds_runIQ(float32_t* i_buff, float32_t* q_buff, uint16_t size)
{
    if (!ones) { __real_softdds_runIQ(i_buff, q_buff, size); return; }
    for (int k = 0; k < size; k++) i_buff[k] = q_buff[k] = 1.0f;
}

static int put_char(uint8_t c)
{
    const int next = (head + 1) % capacity;
    if (next == tail) return 0;
    ring[head] = c;
    head = next;
    return 1;
}

static void setup(int mode, int speed, int weight, int reverse, int rx_delay, int sidetone)
{
    ts.samp_rate = 48000;
    ts.txrx_mode = TRX_MODE_TX;
    ts.dmod_mode = DEMOD_CW;
    ts.cw_text_entry = false;
    ts.tune = 0;
    ts.cw_keyer_mode = (uint8_t)mode;
    ts.cw_keyer_speed = (uint8_t)speed;
    ts.cw_keyer_weight = (uint8_t)weight;
    ts.cw_paddle_reverse = (uint8_t)reverse;
    ts.cw_rx_delay = (uint8_t)rx_delay;
    ts.cw_sidetone_freq = (uint32_t)sidetone;
    /* in CW transmit CwGen_Init leaves cw_state and the timers as they are: a fresh ps has them 0 */
    CwGen_Init();
    AudioManagement_SetSidetoneForDemodMode(ts.dmod_mode, false);
}

static int tables(int nchars, int nsigns, const char* path)
{
    FILE* out = fopen(path, "wb");
    if (!out) { perror(path); return 1; }
    const uint32_t n[2] = { (uint32_t)nchars, (uint32_t)nsigns };
    fwrite(n, 4, 2, out);
    fwrite(cw_char_codes, 4, (size_t)nchars, out);
    fwrite(cw_char_chars, 1, (size_t)nchars, out);
    fwrite(cw_sign_codes, 4, (size_t)nsigns, out);
    for (int k = 0; k < nsigns; k++) fwrite(cw_sign_chars[k], 1, 2, out);
    capacity = 8;
    setup(CW_KEYER_MODE_STRAIGHT, 20, 100, 0, 0, 750);
    ones = 1;
    lines = 2;
    for (int b = 0; b < 8; b++)
    {
        float32_t i[32], q[32];
        if (!CwGen_Process(i, q, 32)) return 1;
        for (int k = 0; k < 32; k += 2)
        {
            if (i[k] != i[k + 1] || i[k] != q[k]) return 1;
            fwrite(&i[k], 4, 1, out);
        }
    }
    fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 5 && !strcmp(argv[1], "tables")) return tables(atoi(argv[2]), atoi(argv[3]), argv[4]);
    if (argc != 11 || strcmp(argv[1], "gen")) { fprintf(stderr, "usage: see the head of cwgen_driver.c\n"); return 2; }
    capacity = atoi(argv[8]);
    ring = malloc((size_t)capacity);
    FILE* ops = fopen(argv[9], "r");
    FILE* out = fopen(argv[10], "wb");
    if (!ops || !out || !ring) { perror("cwgen_driver"); return 1; }
    setup(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]));

    static char line[1 << 16];
    int before = 0;
    while (fgets(line, sizeof line, ops))
    {
        char* arg = strchr(line, ' ');
        if (arg) *arg++ = 0;
        line[strcspn(line, "\n")] = 0;
        if (!strcmp(line, "put"))
        {
            int k = 0;
            unsigned byte;
            for (; arg && sscanf(arg, "%2x", &byte) == 1; arg += 2) k += put_char((uint8_t)byte);
            printf("accepted %d\n", k);
        }
        else if (!strcmp(line, "speed"))
        {
            int s, w;
            if (sscanf(arg, "%d %d", &s, &w) != 2) return 2;
            ts.cw_keyer_speed = (uint8_t)s;
            ts.cw_keyer_weight = (uint8_t)w;
            CwGen_SetSpeed();
        }
        else if (!strcmp(line, "blk"))
        {
            int count;
            if (sscanf(arg, "%d %d", &lines, &count) != 2) return 2;
            for (; count > 0; count--)
            {
                float32_t iq[2][32];
                memset(iq, 0, sizeof iq);
                flags = 0;
                if (lines & ~before & 3) CwGen_DitIRQ();
                before = lines;
                if (CwGen_Process(iq[0], iq[1], 32)) flags |= 1;
                else memset(iq, 0, sizeof iq);
                const uint32_t rec[6] = { flags, ps.w[PS_STATE], ps.w[PS_KEY_TIMER], ps.w[PS_SM_PTR], ps.w[PS_PORT], dbldds[0].acc };
                fwrite(rec, 4, 6, out);
                fwrite(iq, 4, 64, out);
            }
        }
        else if (line[0]) { fprintf(stderr, "unknown op %s\n", line); return 2; }
    }
    fclose(out);
    printf("end %lu ", consumed);
    for (int k = 0; k < echoed; k++) printf("%02x", echo[k]);
    printf("\n");
    return 0;
}
