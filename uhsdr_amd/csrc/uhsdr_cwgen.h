/*
 * CW generator: one channel's keyer (PaddleState), softdds accumulator, text queue and echo ring,
 * advanced by one 32-sample block (one call of the firmware's CwGen_Process at 1500 Hz).
 *
 * Restates drivers/audio/cw/cw_gen.c: CwGen_SetSpeed :387-406, CwGen_Init :421-444, the two edge
 * shapers :449-507, CwGen_CheckPaddleState / CwGen_CheckDigiBufferState :572-634,
 * CwGen_ProcessStraightKey :661-745, CwGen_AddChar :792-825, CwGen_ProcessIambic :827-1033,
 * CwGen_TestFirstPaddle / CwGen_ResetBufferSending / CwGen_DitIRQ :1036-1081, and the single tone of
 * softdds_runIQ (softdds.c:60-78).  Everything is integer arithmetic except the envelope multiply,
 * one rounded binary32 product per shaper that touches a sample, in the firmware's order.
 *
 * The same functions run on the host (uhsdr_cwgen_process_host) and in the cwgen_gen kernel.
 *
 * A block is planned first (CwGenChan::block: the state machine, which never looks at a sample) and
 * its 32 samples follow from the plan (cwgen_sample): whether the tone runs, the accumulator at the
 * block's first sample, and the table pointer each shaper starts the block with.  A shaper moves its
 * pointer every second sample, so the pointer after a block is known without running the samples:
 * the rising one adds 16 and stops at 128, the falling one starts at 127 at most, takes 16 off and
 * stops at 0.
 *
 * The firmware's surroundings as modelled here: the transmitter is in TX throughout (CW_WAIT passes
 * at once), DEMOD_CW, no text entry, no CAT keying.  The key lines are constant over a block.  In
 * the block where a line closes, CwGen_DitIRQ's effects run before CwGen_Process: the text queue is
 * emptied (DigiModes_TxBufferReset: the consumer jumps to the producer, so `consumed` counts what
 * was taken and what was discarded), sending_char is cleared and, outside STRAIGHT, the ULTIMATE
 * keyer notes which paddle came first.
 *
 * Kept as the firmware has them:
 *   - softdds_runIQ runs only in blocks with a tone, so the phase stands still between elements and
 *     nothing resets it;
 *   - the iambic machine runs its states again within one call until one of them makes a block;
 *   - a character of the text queue that has no code is taken and dropped, one per visit of CW_IDLE;
 *   - cw_char is 32 bits and wraps; above 50000 the character is given to CwGen_AddChar as -1,
 *     which no table has: '*';
 *   - CwGen_AddChar's output is what DigiModes_TxBufferPutChar / PutSign hand to
 *     UiDriver_TextMsgPutChar when CW is both source and consumer: the character, or the four
 *     bytes "<XX>" of a prosign, or '*'; the word space is CwGen_AddChar(1);
 *   - the straight key reads the DAH/PTT line whatever paddle_reverse says.
 */
#ifndef UHSDR_CWGEN_H
#define UHSDR_CWGEN_H

#include "uhsdr_digiq.h"

#define CWGEN_BLOCK       32
#define CWGEN_ENV_SIZE    128          /* CW_SMOOTH_TBL_SIZE */
#define CWGEN_ENV_BLOCK   16           /* table steps per block: CWGEN_BLOCK / CW_SMOOTH_LEN */
#define CWGEN_SMOOTH_STEPS 9           /* CW_SMOOTH_STEPS */
#define CWGEN_DEC_MAX     64           /* room for the character and prosign codes */

enum { CWGEN_MODE_IAM_B = 0, CWGEN_MODE_IAM_A, CWGEN_MODE_STRAIGHT, CWGEN_MODE_ULTIMATE };
enum { CWGEN_IDLE = 0, CWGEN_DIT_CHECK = 1, CWGEN_DAH_CHECK = 3, CWGEN_KEY_DOWN = 4, CWGEN_KEY_UP = 5, CWGEN_PAUSE = 6, CWGEN_WAIT = 7 };
enum { CWGEN_DIT_L = 0x01, CWGEN_DAH_L = 0x02, CWGEN_DIT_PROC = 0x04, CWGEN_END_PROC = 0x10 };
enum { CWGEN_F_ACTIVE = 1, CWGEN_F_TXON = 2, CWGEN_F_TXOFF = 4 };

/* integer state, rows of DigiModArena::is */
enum
{
    CWGEN_I_PORT = 0,        /* ps.port_state */
    CWGEN_I_STATE,           /* ps.cw_state */
    CWGEN_I_KEY_TIMER,
    CWGEN_I_BREAK_TIMER,
    CWGEN_I_SPACE_TIMER,
    CWGEN_I_SM_PTR,          /* ps.sm_tbl_ptr */
    CWGEN_I_ULTIM,
    CWGEN_I_CW_CHAR,
    CWGEN_I_SENDING,         /* ps.sending_char */
    CWGEN_I_ACC,             /* dbldds[0].acc */
    CWGEN_I_KEYS,            /* the key lines of the block before */
    CWGEN_I_COUNT
};

/* Handle-wide, as ts is one per transceiver: the launch constants of a generator */
struct CwGenParams
{
    int32_t mode, reverse;
    int32_t dit_time, dah_time, pause_time, space_time;     /* CwGen_SetSpeed */
    int32_t break_time;                                     /* CwGen_GetBreakTime */
    uint32_t step;                                          /* softdds step of the tone */
};

/* CwGen_SetSpeed: 1500 blocks a second, times in blocks, scaled by 100 until the end */
inline void cwgen_set_speed(CwGenParams& p, int32_t speed, int32_t weight)
{
    const int32_t dit = 180000 / speed + CWGEN_SMOOTH_STEPS * 100;
    const int32_t dah = 3 * 180000 / speed + CWGEN_SMOOTH_STEPS * 100;
    const int32_t pause = 180000 / speed - CWGEN_SMOOTH_STEPS * 100;
    const int32_t space = 6 * 180000 / speed;
    const int32_t corr = (weight - 100) * dit / 100;
    p.dit_time = (dit + corr) / 100;
    p.dah_time = (dah + corr) / 100;
    p.pause_time = (pause - corr) / 100;
    p.space_time = space / 100;
}

/* What the generator adds to the modulators' arena (m.codes: byte -> the character's code with its
   elements in sending order, CwGen_ReverseCode, 0 where the table has none; lower case as upper) */
struct CwGenArena
{
    DigiModArena m;
    const float* env;            /* [128] sm_table */
    const uint32_t* dec_code;    /* [dec_count] cw_char_codes, then cw_sign_codes */
    const uint32_t* dec_out;     /* [dec_count] the bytes CwGen_AddChar prints, first byte lowest */
    int32_t dec_chars, dec_count;
    int32_t echo_capacity;
    uint32_t* echo_total;        /* [C] bytes printed since reset */
    uint8_t* echo;               /* [C][echo_capacity], byte k at k % echo_capacity */
};

/* One block as planned: flags, and what the 32 samples need */
struct CwGenBlock
{
    uint32_t flags;
    uint32_t acc;        /* the accumulator at the block's first sample */
    int32_t rise, fall;  /* the table pointer a shaper starts the block with, -1: it does not run */
};

/* Sample s of a planned block with a tone: softdds_genIQSingleTone, then the shapers in order */
DIGI_HD void cwgen_sample(const CwGenBlock& b, uint32_t step, int32_t s, const int16_t* sine, const float* env, float& i, float& q)
{
    const uint32_t k = ((b.acc + (uint32_t)s * step) >> 22) % 1024u;
    float vi = (float)sine[k], vq = (float)sine[(k + 768u) % 1024u];
    if (b.rise >= 0)
    {
        const int32_t p = b.rise + (s >> 1);
        if (p < CWGEN_ENV_SIZE) { vi = vi * env[p]; vq = vq * env[p]; }        /* past the table: the loop has left */
    }
    if (b.fall >= 0)
    {
        const int32_t p = b.fall - (s >> 1);
        const float e = env[p > 0 ? p : 0];
        vi = vi * e;
        vq = vq * e;
    }
    i = vi;
    q = vq;
}

/* One channel: its state, its end of the text queue and of the echo ring in registers. */
struct CwGenChan
{
    uint32_t port, state;
    int32_t key_timer, break_timer, space_timer;
    uint32_t sm_ptr, ultim, cw_char, sending, acc, keys;
    uint32_t echo_total;
    DigiQueue q;

    DIGI_HD void load(const CwGenArena& a, int32_t c)
    {
        const size_t n = (size_t)a.m.C;
        const uint32_t* i = a.m.is + c;
        port = i[CWGEN_I_PORT * n]; state = i[CWGEN_I_STATE * n];
        key_timer = (int32_t)i[CWGEN_I_KEY_TIMER * n]; break_timer = (int32_t)i[CWGEN_I_BREAK_TIMER * n];
        space_timer = (int32_t)i[CWGEN_I_SPACE_TIMER * n];
        sm_ptr = i[CWGEN_I_SM_PTR * n]; ultim = i[CWGEN_I_ULTIM * n]; cw_char = i[CWGEN_I_CW_CHAR * n];
        sending = i[CWGEN_I_SENDING * n]; acc = i[CWGEN_I_ACC * n]; keys = i[CWGEN_I_KEYS * n];
        echo_total = a.echo_total[c];
        q.load(a.m, c);
    }

    DIGI_HD void store(const CwGenArena& a, int32_t c, const CwGenParams& p) const
    {
        const size_t n = (size_t)a.m.C;
        uint32_t* i = a.m.is + c;
        i[CWGEN_I_PORT * n] = port; i[CWGEN_I_STATE * n] = state;
        i[CWGEN_I_KEY_TIMER * n] = (uint32_t)key_timer; i[CWGEN_I_BREAK_TIMER * n] = (uint32_t)break_timer;
        i[CWGEN_I_SPACE_TIMER * n] = (uint32_t)space_timer;
        i[CWGEN_I_SM_PTR * n] = sm_ptr; i[CWGEN_I_ULTIM * n] = ultim; i[CWGEN_I_CW_CHAR * n] = cw_char;
        i[CWGEN_I_SENDING * n] = sending; i[CWGEN_I_ACC * n] = acc; i[CWGEN_I_KEYS * n] = keys;
        a.echo_total[c] = echo_total;
        a.m.state[c] = (uint8_t)(p.mode == CWGEN_MODE_STRAIGHT ? (uint32_t)key_timer : state);
        q.store(a.m, c);
    }

    /* CwGen_Init on a fresh ps, the accumulator at 0, the queue and the echo empty.  The model is in
       CW transmit throughout, where CwGen_Init leaves the break timer alone: it starts at 0, and the
       first TX-off request follows the first element. */
    DIGI_HD void reset()
    {
        port = 0; state = CWGEN_IDLE;
        key_timer = 0; break_timer = 0; space_timer = 0;
        sm_ptr = 0; ultim = 0; cw_char = 0; sending = 0; acc = 0; keys = 0;
        echo_total = 0;
        q.put = q.consumed = 0;
        q.txoff_at = DIGI_NO_TXOFF;
    }

    DIGI_HD void print(const CwGenArena& a, int32_t c, uint8_t ch)
    {
        a.echo[(size_t)c * a.echo_capacity + echo_total % (uint32_t)a.echo_capacity] = ch;
        ++echo_total;
    }

    /* CwGen_AddChar */
    DIGI_HD void add_char(const CwGenArena& a, int32_t c, uint32_t code)
    {
        int32_t k = 0;
        while (k < a.dec_count && a.dec_code[k] != code) k++;
        if (k == a.dec_count) print(a, c, '*');
        else
        {
            const uint32_t out = a.dec_out[k];
            const int32_t bytes = k < a.dec_chars ? 1 : 4;
            for (int32_t b = 0; b < bytes; b++) print(a, c, (uint8_t)(out >> (8 * b)));
        }
        cw_char = 0;
    }

    static DIGI_HD bool dit_requested(const CwGenParams& p, uint32_t lines) { return ((p.reverse ? lines >> 1 : lines) & 1u) != 0; }
    static DIGI_HD bool dah_requested(const CwGenParams& p, uint32_t lines) { return ((p.reverse ? lines : lines >> 1) & 1u) != 0; }

    /* CwGen_CheckPaddleState */
    DIGI_HD void check_paddles(const CwGenParams& p, uint32_t lines)
    {
        if (dah_requested(p, lines)) port |= CWGEN_DAH_L;
        if (dit_requested(p, lines)) port |= CWGEN_DIT_L;
    }

    /* CwGen_TestFirstPaddle */
    DIGI_HD void test_first_paddle(const CwGenParams& p, uint32_t lines)
    {
        if (p.mode != CWGEN_MODE_ULTIMATE) return;
        const bool dit = dit_requested(p, lines), dah = dah_requested(p, lines);
        if (!dit && dah) ultim = 1;
        if (dit && !dah) ultim = 0;
    }

    /* CwGen_CheckDigiBufferState */
    DIGI_HD void check_text(const CwGenArena& a, const CwGenParams& p, CwGenBlock& b)
    {
        if (!sending && !(port & CWGEN_END_PROC) && space_timer < p.space_time - p.dah_time && q.has_data())
        {
            const uint32_t code = a.m.codes[q.remove()];
            if (code)
            {
                sending = code;
                if (sending == 1) space_timer = p.space_time;
                else b.flags |= CWGEN_F_TXON;
            }
        }
        if (sending > 1)
        {
            port |= sending % 4 == 3 ? CWGEN_DAH_L : CWGEN_DIT_L;
            sending /= 4;
        }
    }

    /* softdds_runIQ over the block */
    DIGI_HD void tone(const CwGenParams& p, CwGenBlock& b)
    {
        b.flags |= CWGEN_F_ACTIVE;
        b.acc = acc;
        acc += (uint32_t)CWGEN_BLOCK * p.step;
    }

    /* CwGen_RemoveClickOnRisingEdge */
    DIGI_HD void rise(CwGenBlock& b)
    {
        if (sm_ptr < CWGEN_ENV_SIZE)
        {
            b.rise = (int32_t)sm_ptr;
            sm_ptr = sm_ptr + CWGEN_ENV_BLOCK < CWGEN_ENV_SIZE ? sm_ptr + CWGEN_ENV_BLOCK : CWGEN_ENV_SIZE;
        }
    }

    /* CwGen_RemoveClickOnFallingEdge */
    DIGI_HD void fall(CwGenBlock& b)
    {
        if (sm_ptr > CWGEN_ENV_SIZE - 1) sm_ptr = CWGEN_ENV_SIZE - 1;
        b.fall = (int32_t)sm_ptr;
        sm_ptr = sm_ptr > CWGEN_ENV_BLOCK ? sm_ptr - CWGEN_ENV_BLOCK : 0;
    }

    /* CwGen_ProcessStraightKey */
    DIGI_HD void straight(const CwGenParams& p, uint32_t lines, CwGenBlock& b)
    {
        const bool pressed = (lines & 2u) != 0;
        if (pressed && key_timer == 0)
        {
            sm_ptr = 0;
            key_timer = 3;
            break_timer = p.break_time;
        }
        if (key_timer == 0)
        {
            if (break_timer > 0 && --break_timer == 0) b.flags |= CWGEN_F_TXOFF;
            return;
        }
        tone(p, b);
        if (key_timer > 2)
        {
            rise(b);
            if (sm_ptr >= CWGEN_ENV_SIZE) key_timer = 2;
        }
        if (key_timer < 2)
        {
            fall(b);
            if (sm_ptr == 0)
            {
                break_timer = p.break_time;
                key_timer = 0;
            }
        }
        if (key_timer == 2 && !pressed) key_timer = 1;
    }

    /* CwGen_ProcessIambic */
    DIGI_HD void iambic(const CwGenArena& a, const CwGenParams& p, int32_t c, uint32_t lines, CwGenBlock& b)
    {
        bool rerun;
        do
        {
            rerun = false;
            switch (state)
            {
            case CWGEN_IDLE:
                check_paddles(p, lines);
                check_text(a, p, b);
                if (port & (CWGEN_DAH_L | CWGEN_DIT_L))
                {
                    state = CWGEN_WAIT;
                    rerun = true;
                }
                else
                {
                    if (port & CWGEN_END_PROC)
                    {
                        add_char(a, c, cw_char > 50000u ? 0xffffffffu : cw_char);
                        port &= ~(uint32_t)CWGEN_END_PROC;
                        space_timer = p.space_time;
                    }
                    if (space_timer > 0 && --space_timer == 0)
                    {
                        add_char(a, c, 1);
                        if (sending == 1) sending = 0;
                    }
                    if (break_timer > 0 && --break_timer == 0) b.flags |= CWGEN_F_TXOFF;
                }
                break;
            case CWGEN_WAIT:             /* in TX throughout */
                state = CWGEN_DIT_CHECK;
                rerun = true;
                break;
            case CWGEN_DIT_CHECK:
                if (port & CWGEN_DIT_L)
                {
                    port |= CWGEN_DIT_PROC;
                    key_timer = p.dit_time;
                    state = CWGEN_KEY_DOWN;
                    cw_char = cw_char * 4u + 2u;
                }
                else state = CWGEN_DAH_CHECK;
                rerun = true;
                break;
            case CWGEN_DAH_CHECK:
                if (port & CWGEN_DAH_L)
                {
                    key_timer = p.dah_time;
                    cw_char = cw_char * 4u + 3u;
                    state = CWGEN_KEY_DOWN;
                }
                else
                {
                    break_timer = p.break_time;
                    port |= CWGEN_END_PROC;
                    state = CWGEN_IDLE;
                }
                rerun = true;
                break;
            case CWGEN_KEY_DOWN:
                tone(p, b);
                key_timer--;
                sm_ptr = 0;
                rise(b);
                port &= ~(uint32_t)(CWGEN_DIT_L + CWGEN_DAH_L);
                state = CWGEN_KEY_UP;
                break;
            case CWGEN_KEY_UP:
                if (key_timer == 0)
                {
                    key_timer = p.pause_time;
                    state = CWGEN_PAUSE;
                }
                else
                {
                    tone(p, b);
                    key_timer--;
                    if (key_timer > p.dit_time / 2) rise(b);
                    if (key_timer < CWGEN_SMOOTH_STEPS) fall(b);
                    if (p.mode == CWGEN_MODE_IAM_B) check_paddles(p, lines);
                }
                break;
            case CWGEN_PAUSE:
                key_timer--;
                if (key_timer == 0)
                {
                    check_paddles(p, lines);
                    bool to_dah;
                    if (p.mode == CWGEN_MODE_IAM_A || p.mode == CWGEN_MODE_IAM_B) to_dah = (port & CWGEN_DIT_PROC) != 0;
                    else
                    {
                        test_first_paddle(p, lines);
                        to_dah = (port & CWGEN_DAH_L) && ultim == 0;
                    }
                    if (to_dah)
                    {
                        port &= ~(uint32_t)(CWGEN_DIT_L + CWGEN_DIT_PROC);
                        state = CWGEN_DAH_CHECK;
                    }
                    else
                    {
                        port |= CWGEN_END_PROC;
                        port &= ~(uint32_t)CWGEN_DAH_L;
                        break_timer = p.break_time;
                        state = CWGEN_IDLE;
                    }
                    rerun = true;
                }
                break;
            default:
                break;
            }
        } while (rerun);
    }

    /* One block: the key lines' edge (CwGen_DitIRQ), then CwGen_Process */
    DIGI_HD CwGenBlock block(const CwGenArena& a, const CwGenParams& p, int32_t c, uint32_t lines)
    {
        CwGenBlock b;
        b.flags = 0; b.acc = 0; b.rise = -1; b.fall = -1;
        lines &= 3u;
        if (lines & ~keys)
        {
            q.consumed = q.put;          /* CwGen_ResetBufferSending */
            sending = 0;
            if (p.mode != CWGEN_MODE_STRAIGHT) test_first_paddle(p, lines);
        }
        keys = lines;
        if (p.mode == CWGEN_MODE_STRAIGHT) straight(p, lines, b);
        else iambic(a, p, c, lines, b);
        return b;
    }
};

#endif
