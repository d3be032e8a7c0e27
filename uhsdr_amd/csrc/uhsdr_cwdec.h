/*
 * CW decoder back end: one channel's Morse-to-text state machine, advanced by one CW block.
 *
 * Restates what the firmware runs after the mark/space decision of a block
 * (drivers/audio/cw/cw_decoder.c:326-375, with InitializationFunc :409-489, the spike cancel
 * :500-539, DataRecognitionFunc :556-718, PrintCharFunc / WordSpaceFunc :731-850,
 * ErrorCorrectionFunc :867-1027, CW_Decode :1040-1078 and CwGen_CharacterIdFunc, cw_gen.c:756).
 * The input of a step is the value ads.CW_signal has at :319; the front end that produces it is
 * rx_back's (uhsdr_rx.hip, BackAudio::end).
 *
 * The same function runs on the host (uhsdr_cwdec_process_host) and in the cw_decode kernel:
 * both address one field-major arena, so a channel's state is a column of it.
 *
 * Arithmetic follows the reference's C exactly: an expression with a double literal is
 * evaluated in double and rounded once on the store to float, a comparison between floats stays
 * in float.  The build has -ffp-contract=off.
 *
 * Float -> integer stores.  The reference binary is x86-64 gcc output: float -> int32 is
 * cvttss2si (anything out of range or NaN gives 0x80000000), float -> uint32 is the 64-bit
 * cvttss2si with the low 32 bits kept, and a narrower destination (uint8_t, int16_t, the 31-bit
 * time field) keeps the low bits of that.  The GPU's v_cvt_* saturate instead, so the two
 * helpers below test the range first and convert only in-range values; cwdec_cvt_* then give the
 * x86 result on both sides.
 */
#ifndef UHSDR_CWDEC_H
#define UHSDR_CWDEC_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CWD_HD __host__ __device__ inline
#else
#define CWD_HD inline
#endif

#define CWDEC_SIG_SIZE   256      /* CW_SIG_BUFSIZE */
#define CWDEC_DATA_SIZE   40      /* CW_DATA_BUFSIZE */
#define CWDEC_TIMEOUT      3      /* CW_TIMEOUT, seconds */
#define CWDEC_SPIKE_MAX    8u     /* CW_SPIKECANCEL_MAX_DURATION */
#define CWDEC_LOOP_MAX   256      /* bound of every reprocessing loop: one trip per ring counter step */

/* integer scalars of a channel, rows of CwDecArena::iscal */
enum
{
    CWD_I_LASTRX = 0, CWD_I_INCOUNT, CWD_I_OUTCOUNT, CWD_I_CUR_OUT, CWD_I_LAST_OUT,
    CWD_I_TIMER, CWD_I_CUR_TIME, CWD_I_DATA_LEN, CWD_I_W_SPACE, CWD_I_STARTPOS, CWD_I_PROGRESS,
    CWD_I_FLAGS, CWD_I_COUNT
};
/* float scalars, rows of CwDecArena::fscal */
enum { CWD_F_PULSE = 0, CWD_F_DOT, CWD_F_DASH, CWD_F_SYMSPACE, CWD_F_CWSPACE, CWD_F_WPM_AVG, CWD_F_COUNT };

/* flag bits: bflags (initialized, dash, wspace, timeout, overload), prevstate and the
   function-local statics processed / spike / initializing */
enum
{
    CWD_INITIALIZED = 1u, CWD_DASH = 2u, CWD_WSPACE = 4u, CWD_TIMEOUT = 8u, CWD_OVERLOAD = 16u,
    CWD_PREVSTATE = 32u, CWD_PROCESSED = 64u, CWD_SPIKE = 128u, CWD_INITIALIZING = 256u
};

/* All channels' state, field-major.  A ring / data element is (time << 1) | state. */
struct CwDecArena
{
    int32_t C;
    int32_t text_capacity;
    uint32_t* ring;      /* [256][C] */
    uint32_t* data;      /* [40][C]  */
    int32_t* iscal;      /* [CWD_I_COUNT][C] */
    float* fscal;        /* [CWD_F_COUNT][C] */
    uint8_t* text;       /* [C][text_capacity], character k at k % text_capacity */
    uint32_t* total;     /* [C] */
    uint8_t* wpm;        /* [C] */
};

CWD_HD int32_t cwdec_cvt_i32(float f)
{
    if (!(f > -2147483904.0f && f < 2147483648.0f)) return INT32_MIN;   /* cvttss2si's indefinite */
    return (int32_t)f;
}

CWD_HD uint32_t cwdec_cvt_u32(float f)
{
    if (!(f > -9223373136366403584.0f && f < 9223372036854775808.0f)) return 0u;   /* low half of 0x8000000000000000 */
    return (uint32_t)(uint64_t)(int64_t)f;
}

/* dots and dashes to the reference's code: two bits per element, 10 a dot, 11 a dash, first element highest */
constexpr uint32_t cwdec_code(const char* s)
{
    uint32_t code = 0;
    for (; *s; ++s) code = code * 4u + (*s == '-' ? 3u : 2u);
    return code;
}

/* CwGen_CharacterIdFunc: ITU-R M.1677 letters, figures and punctuation, then the prosigns as the
   one-character stand-ins the print step spells out; 0xfe for the empty code, 0xff unknown */
CWD_HD uint8_t cwdec_char_id(uint32_t code)
{
    switch (code)
    {
    case 0u: return 0xfe;
    case 1u: return ' ';
    case cwdec_code(".-"): return 'A';     case cwdec_code("-..."): return 'B';
    case cwdec_code("-.-."): return 'C';   case cwdec_code("-.."): return 'D';
    case cwdec_code("."): return 'E';      case cwdec_code("..-."): return 'F';
    case cwdec_code("--."): return 'G';    case cwdec_code("...."): return 'H';
    case cwdec_code(".."): return 'I';     case cwdec_code(".---"): return 'J';
    case cwdec_code("-.-"): return 'K';    case cwdec_code(".-.."): return 'L';
    case cwdec_code("--"): return 'M';     case cwdec_code("-."): return 'N';
    case cwdec_code("---"): return 'O';    case cwdec_code(".--."): return 'P';
    case cwdec_code("--.-"): return 'Q';   case cwdec_code(".-."): return 'R';
    case cwdec_code("..."): return 'S';    case cwdec_code("-"): return 'T';
    case cwdec_code("..-"): return 'U';    case cwdec_code("...-"): return 'V';
    case cwdec_code(".--"): return 'W';    case cwdec_code("-..-"): return 'X';
    case cwdec_code("-.--"): return 'Y';   case cwdec_code("--.."): return 'Z';
    case cwdec_code(".----"): return '1';  case cwdec_code("..---"): return '2';
    case cwdec_code("...--"): return '3';  case cwdec_code("....-"): return '4';
    case cwdec_code("....."): return '5';  case cwdec_code("-...."): return '6';
    case cwdec_code("--..."): return '7';  case cwdec_code("---.."): return '8';
    case cwdec_code("----."): return '9';  case cwdec_code("-----"): return '0';
    case cwdec_code("-...-"): return '=';  case cwdec_code("-..-."): return '/';
    case cwdec_code("..--.."): return '?'; case cwdec_code(".-..-."): return '"';
    case cwdec_code(".-.-.-"): return '.'; case cwdec_code(".--.-."): return '@';
    case cwdec_code(".----."): return '\''; case cwdec_code("-....-"): return '-';
    case cwdec_code("--..--"): return ','; case cwdec_code("---..."): return ':';
    case cwdec_code(".-.-"): return '^';       /* AA */
    case cwdec_code(".-.-."): return '+';      /* AR */
    case cwdec_code(".-..."): return '&';      /* AS */
    case cwdec_code("-.-..-.."): return '{';   /* CL */
    case cwdec_code("-.-.-"): return '}';      /* CT */
    case cwdec_code("........"): return 0x7f;  /* HH, the error sign */
    case cwdec_code("-.--."): return '(';      /* KN */
    case cwdec_code("-..---"): return '%';     /* NJ */
    case cwdec_code("...-.-"): return '>';     /* SK */
    case cwdec_code("...-."): return '~';      /* SN */
    default: return 0xff;
    }
}

/* One channel: its scalars in registers, ring / data / text through the arena column. */
struct CwDec
{
    int32_t sig_lastrx, sig_incount, sig_outcount, cur_outcount, last_outcount;
    int32_t sig_timer, cur_time, data_len, w_space, startpos, progress;
    uint32_t flags;
    float pulse_avg, dot_avg, dash_avg, symspace_avg, cwspace_avg, speed_wpm_avg;
    uint32_t total, code;
    uint8_t speed;

    uint32_t* ring;
    uint32_t* data;
    uint8_t* text;
    int32_t C, text_capacity, one_second, spikecancel;
    float blocksize_f;

    CWD_HD void load(const CwDecArena& a, int32_t c, int32_t blocksize, int32_t spikecancel_)
    {
        const size_t n = (size_t)a.C;
        const int32_t* i = a.iscal + c;
        sig_lastrx = i[CWD_I_LASTRX * n]; sig_incount = i[CWD_I_INCOUNT * n]; sig_outcount = i[CWD_I_OUTCOUNT * n];
        cur_outcount = i[CWD_I_CUR_OUT * n]; last_outcount = i[CWD_I_LAST_OUT * n];
        sig_timer = i[CWD_I_TIMER * n]; cur_time = i[CWD_I_CUR_TIME * n]; data_len = i[CWD_I_DATA_LEN * n];
        w_space = i[CWD_I_W_SPACE * n]; startpos = i[CWD_I_STARTPOS * n]; progress = i[CWD_I_PROGRESS * n];
        flags = (uint32_t)i[CWD_I_FLAGS * n];
        const float* f = a.fscal + c;
        pulse_avg = f[CWD_F_PULSE * n]; dot_avg = f[CWD_F_DOT * n]; dash_avg = f[CWD_F_DASH * n];
        symspace_avg = f[CWD_F_SYMSPACE * n]; cwspace_avg = f[CWD_F_CWSPACE * n]; speed_wpm_avg = f[CWD_F_WPM_AVG * n];
        total = a.total[c];
        speed = a.wpm[c];
        code = 0;
        ring = a.ring + c; data = a.data + c;
        text = a.text + (size_t)c * a.text_capacity;
        C = a.C; text_capacity = a.text_capacity;
        one_second = 12000 / blocksize;             /* ONE_SECOND, integer */
        spikecancel = spikecancel_;
        blocksize_f = (float)blocksize;
    }

    CWD_HD void store(const CwDecArena& a, int32_t c) const
    {
        const size_t n = (size_t)a.C;
        int32_t* i = a.iscal + c;
        i[CWD_I_LASTRX * n] = sig_lastrx; i[CWD_I_INCOUNT * n] = sig_incount; i[CWD_I_OUTCOUNT * n] = sig_outcount;
        i[CWD_I_CUR_OUT * n] = cur_outcount; i[CWD_I_LAST_OUT * n] = last_outcount;
        i[CWD_I_TIMER * n] = sig_timer; i[CWD_I_CUR_TIME * n] = cur_time; i[CWD_I_DATA_LEN * n] = data_len;
        i[CWD_I_W_SPACE * n] = w_space; i[CWD_I_STARTPOS * n] = startpos; i[CWD_I_PROGRESS * n] = progress;
        i[CWD_I_FLAGS * n] = (int32_t)flags;
        float* f = a.fscal + c;
        f[CWD_F_PULSE * n] = pulse_avg; f[CWD_F_DOT * n] = dot_avg; f[CWD_F_DASH * n] = dash_avg;
        f[CWD_F_SYMSPACE * n] = symspace_avg; f[CWD_F_CWSPACE * n] = cwspace_avg; f[CWD_F_WPM_AVG * n] = speed_wpm_avg;
        a.total[c] = total;
        a.wpm[c] = speed;
    }

    /* ring and data access: every index is masked / clamped, whatever the counters hold */
    CWD_HD uint32_t sig(int32_t i) const { return ring[(size_t)(i & (CWDEC_SIG_SIZE - 1)) * C]; }
    CWD_HD void sig_set(int32_t i, uint32_t v) { ring[(size_t)(i & (CWDEC_SIG_SIZE - 1)) * C] = v; }
    CWD_HD uint32_t sig_time(int32_t i) const { return sig(i) >> 1; }
    CWD_HD bool sig_state(int32_t i) const { return (sig(i) & 1u) != 0; }
    CWD_HD void sig_set_time(int32_t i, uint32_t t) { sig_set(i, (t << 1) | (sig(i) & 1u)); }
    CWD_HD static int32_t didx(int32_t i) { return i < 0 ? 0 : (i > CWDEC_DATA_SIZE - 1 ? CWDEC_DATA_SIZE - 1 : i); }
    /* data[-1] (a space after a time-out that finalised a character ending in a dash) reads as 0 */
    CWD_HD uint32_t dat(int32_t i) const { return i < 0 ? 0u : data[(size_t)didx(i) * C]; }
    CWD_HD void dat_set(int32_t i, uint32_t v) { data[(size_t)didx(i) * C] = v; }

    CWD_HD static int32_t inc(int32_t v) { return (v + 1) == CWDEC_SIG_SIZE ? 0 : v + 1; }
    CWD_HD static int32_t dec(int32_t v) { return v == 0 ? CWDEC_SIG_SIZE - 1 : v - 1; }
    CWD_HD static int32_t up(int32_t v, int32_t by) { v += by; return v >= CWDEC_SIG_SIZE ? v - CWDEC_SIG_SIZE : v; }
    CWD_HD static int32_t down(int32_t v, int32_t by) { v -= by; return v < 0 ? v + CWDEC_SIG_SIZE : v; }

    CWD_HD bool flag(uint32_t f) const { return (flags & f) != 0; }
    CWD_HD void set(uint32_t f, bool on) { flags = on ? (flags | f) : (flags & ~f); }

    /* UiDriver_TextMsgPutChar */
    CWD_HD void put(uint8_t ch)
    {
        text[total % (uint32_t)text_capacity] = ch;
        ++total;
    }

    /* PrintCharFunc: prosigns spelled out, 0xff as '#' */
    CWD_HD void print_char(uint8_t c)
    {
        switch (c)
        {
        case '}': put('c'); put('t'); break;
        case '(': put('k'); put('n'); break;
        case '&': put('a'); put('s'); break;
        case '~': put('s'); put('n'); break;
        case '>': put('s'); put('k'); break;
        case '+': put('a'); put('r'); break;
        case '^': put('b'); put('k'); break;
        case '{': put('c'); put('l'); break;
        case '%': put('n'); put('j'); break;
        case 0x7f: put('e'); put('r'); put('r'); break;
        case 0xff: put('#'); break;
        default: put(c); break;
        }
    }

    /* WordSpaceFunc, with the longer space wanted after letters that seldom end a word (e.q. 4.15) */
    CWD_HD void word_space(uint8_t c)
    {
        if (!flag(CWD_WSPACE)) return;
        set(CWD_WSPACE, false);
        if (c == 'I' || c == 'J' || c == 'Q' || c == 'U' || c == 'V' || c == 'Z')
        {
            const float xf = (cwspace_avg + pulse_avg) - (float)w_space;
            const int16_t x = (int16_t)(uint16_t)(uint32_t)cwdec_cvt_i32(xf);
            if (x < 0) put(' ');
        }
        else put(' ');
    }

    /* InitializationFunc: dot / dash / space averages over the first 98 states */
    CWD_HD void initialization()
    {
        if (!flag(CWD_INITIALIZING))
        {
            startpos = sig_outcount;
            progress = sig_outcount;
            set(CWD_INITIALIZING, true);
            pulse_avg = 0.0f; dot_avg = 0.0f; dash_avg = 0.0f; symspace_avg = 0.0f; cwspace_avg = 0.0f;
            w_space = 0;
        }
        const int32_t processed = progress < startpos ? (CWDEC_SIG_SIZE + progress) - startpos : progress - startpos;
        if (processed >= 98)
        {
            set(CWD_INITIALIZED, true);
            set(CWD_INITIALIZING, false);
        }
        if (progress != sig_incount)
        {
            const float t = (float)(int32_t)sig_time(progress);
            if (sig_state(progress))
            {
                if (processed > 32)
                {
                    if (t > pulse_avg) dash_avg = (float)((double)dash_avg + (double)(t - dash_avg) / 4.0);
                    else dot_avg = (float)((double)dot_avg + (double)(t - dot_avg) / 4.0);
                }
                else
                {
                    if (t > pulse_avg) dash_avg = (float)((double)(t + dash_avg) / 2.0);
                    else dot_avg = (float)((double)(t + dot_avg) / 2.0);
                }
                pulse_avg = (float)((double)(dot_avg / 4.0f + dash_avg) / 2.0);
            }
            else if (processed > 32)
            {
                if (t > pulse_avg) cwspace_avg = (float)((double)cwspace_avg + (double)(t - cwspace_avg) / 4.0);
                else symspace_avg = (float)((double)symspace_avg + (double)(t - symspace_avg) / 4.0);
            }
            progress = inc(progress & (CWDEC_SIG_SIZE - 1));
        }
    }

    /* CwDecoder_IsSpike */
    CWD_HD bool is_spike(uint32_t t) const
    {
        if (spikecancel == 1) return t <= CWDEC_SPIKE_MAX;
        if (spikecancel == 2) return ((float)(3u * t) < dot_avg) && flag(CWD_INITIALIZED);
        return false;
    }

    /* spikeCancel: 0 for a spike (and the out counter moves on), else the time, with the two
       states before it added once after a spike */
    CWD_HD float spike_cancel(float t)
    {
        if (spikecancel != 0)
        {
            if (is_spike(cwdec_cvt_u32(t)))
            {
                set(CWD_SPIKE, true);
                sig_outcount = inc(sig_outcount);
                t = 0.0f;
            }
            else if (flag(CWD_SPIKE))
            {
                set(CWD_SPIKE, false);
                t = t + (float)(int32_t)sig_time(down(sig_outcount, 1)) + (float)(int32_t)sig_time(down(sig_outcount, 2));
            }
        }
        return t;
    }

    /* DataRecognitionFunc: one state off the ring into data[], or the long key-up time-out.
       Returns whether a state was pending; new_char says a character is complete. */
    CWD_HD bool data_recognition(bool& new_char)
    {
        bool not_done = false;
        new_char = false;
        if (sig_outcount != sig_incount)
        {
            not_done = true;
            set(CWD_TIMEOUT, false);
            const float t = spike_cancel((float)(int32_t)sig_time(sig_outcount));
            if (t > 0.0f)
            {
                const bool mark = sig_state(sig_outcount);
                sig_outcount = inc(sig_outcount);
                if (mark)
                {
                    set(CWD_PROCESSED, false);
                    uint32_t el;
                    if ((pulse_avg - t) >= 0.0f)                 /* dot (e.q. 4.10) */
                    {
                        set(CWD_DASH, false);
                        el = 0u;
                        dot_avg = (float)((double)dot_avg + (double)(t - dot_avg) / 8.0);
                    }
                    else
                    {
                        set(CWD_DASH, true);
                        el = 1u;
                        if (t <= 5.0f * dash_avg)                /* not a stuck key */
                            dash_avg = (float)((double)dash_avg + (double)(t - dash_avg) / 8.0);
                    }
                    dat_set(data_len, ((cwdec_cvt_u32(t) & 0x7fffffffu) << 1) | el);
                    ++data_len;
                    pulse_avg = (float)((double)(dot_avg / 4.0f + dash_avg) / 2.0);
                }
                else
                {
                    bool full_char = true;
                    if (flag(CWD_DASH))
                    {
                        set(CWD_DASH, false);
                        const float last = (float)(dat(data_len - 1) >> 1) - pulse_avg;
                        const float eq4_12 = (float)((double)t - ((double)pulse_avg - (double)last / 4.0));
                        if (eq4_12 < 0.0f)                       /* symbol space */
                        {
                            symspace_avg = (float)((double)symspace_avg + (double)(t - symspace_avg) / 8.0);
                            full_char = false;
                        }
                        else if (t <= 10.0f * dash_avg)          /* not a time-out */
                        {
                            const float eq4_14 = (float)((double)t - ((double)cwspace_avg - (double)last / 4.0));
                            if (eq4_14 >= 0.0f)
                            {
                                w_space = cwdec_cvt_i32(t);
                                set(CWD_WSPACE, true);
                            }
                        }
                    }
                    else
                    {
                        if ((t - pulse_avg) < 0.0f)              /* symbol space (e.q. 4.11) */
                        {
                            symspace_avg = (float)((double)symspace_avg + (double)(t - symspace_avg) / 8.0);
                            full_char = false;
                        }
                        else if (t <= 10.0f * dash_avg)
                        {
                            cwspace_avg = (float)((double)cwspace_avg + (double)(t - cwspace_avg) / 8.0);
                            if ((t - cwspace_avg) >= 0.0f)       /* word space (e.q. 4.13) */
                            {
                                w_space = cwdec_cvt_i32(t);
                                set(CWD_WSPACE, true);
                            }
                        }
                    }
                    if (full_char && !flag(CWD_PROCESSED)) new_char = true;
                }
            }
        }
        else if ((float)cur_time > 10.0f * dash_avg)
        {
            /* reads the slot the current state will be written to: the ring's stale contents */
            if (!sig_state(sig_incount) && !flag(CWD_PROCESSED))
            {
                set(CWD_PROCESSED, true);
                set(CWD_WSPACE, true);
                set(CWD_TIMEOUT, true);
                new_char = true;
            }
        }
        if (data_len > CWDEC_DATA_SIZE - 2) data_len = CWDEC_DATA_SIZE - 2;
        if (new_char)
        {
            last_outcount = cur_outcount;
            cur_outcount = sig_outcount;
        }
        return not_done;
    }

    /* CodeGenFunc */
    CWD_HD void code_gen()
    {
        code = 0u;
        for (int32_t a = 0; a < data_len && a < CWDEC_DATA_SIZE; a++)
            code = code * 4u + ((dat(a) & 1u) ? 3u : 2u);
        data_len = 0;
    }

    /* reprocess what is pending; every trip moves sig_outcount one slot towards sig_incount in the
       reference, so 256 trips are never needed */
    CWD_HD void drain()
    {
        bool dummy;
        for (int32_t n = 0; n < CWDEC_LOOP_MAX && data_recognition(dummy); n++) { }
    }

    /* ErrorCorrectionFunc */
    CWD_HD bool error_correction()
    {
        bool result = false;
        if (data_len >= CWDEC_DATA_SIZE - 2)
        {
            print_char(0xff);
            word_space(0xff);
            return result;
        }
        set(CWD_WSPACE, false);
        int32_t temp = last_outcount & (CWDEC_SIG_SIZE - 1);
        int32_t slocation = last_outcount, plocation = last_outcount;
        uint32_t pduration = UINT32_MAX, sduration = 0u;
        for (int32_t n = 0; n < CWDEC_LOOP_MAX && temp != cur_outcount; n++)
        {
            const uint32_t e = sig(temp);
            const uint32_t et = e >> 1;
            if (e & 1u)
            {
                if (et < pduration && !is_spike(et)) { pduration = et; plocation = temp; }
            }
            /* (cur_outcount - 1) is not wrapped in the reference either */
            if (temp != last_outcount && temp != (cur_outcount - 1) && !(e & 1u))
            {
                if (et > sduration) { sduration = et; slocation = temp; }
            }
            temp = inc(temp);
        }
        uint8_t decoded0 = 0xff, decoded1 = 0xff;
        if (((float)pduration < dot_avg / 2.0f) && (plocation != temp))
        {
            /* drop the shortest pulse: it and the spaces around it become one space */
            sig_set_time(up(plocation, 1), (sig_time(down(plocation, 1)) + sig_time(plocation) + sig_time(up(plocation, 1))) & 0x7fffffffu);
            temp = down(plocation, 2);
            for (int32_t n = 0; n < CWDEC_LOOP_MAX && temp != last_outcount; n++)
            {
                sig_set(up(temp, 2), sig(temp));
                temp = dec(temp);
            }
            sig_outcount = up(last_outcount, 2);
            drain();
            code_gen();
            decoded0 = cwdec_char_id(code);
            if (decoded0 != 0xff) { print_char(decoded0); result = true; }
            else print_char(0xff);
        }
        else
        {
            /* make the longest symbol space a character space: two characters */
            const float split = (cwspace_avg - 1.0f) >= 1.0f ? cwspace_avg - 1.0f : 1.0f;
            sig_set_time(slocation, cwdec_cvt_u32(split) & 0x7fffffffu);
            sig_outcount = last_outcount;
            drain();
            code_gen();
            decoded0 = cwdec_char_id(code);
            drain();
            code_gen();
            decoded1 = cwdec_char_id(code);
            if (decoded0 != 0xff && decoded1 != 0xff) { print_char(decoded0); print_char(decoded1); result = true; }
            else print_char(0xff);
        }
        return result;
    }

    /* CW_Decode */
    CWD_HD void decode()
    {
        if (!flag(CWD_INITIALIZED)) initialization();
        if (flag(CWD_INITIALIZED) || cur_time >= one_second * CWDEC_TIMEOUT)
        {
            bool received;
            data_recognition(received);
            if (received && data_len > 0)
            {
                code_gen();
                const uint8_t decoded = cwdec_char_id(code);
                if (decoded < 0xfe)
                {
                    print_char(decoded);
                    word_space(decoded);
                }
                else if (decoded == 0xff)
                {
                    if (!error_correction()) set(CWD_INITIALIZED, false);
                }
            }
        }
    }

    /* CW_Decode_exe from :326 on, for one block whose mark/space state is cw_state */
    CWD_HD void step(bool cw_state)
    {
        if (cw_state != flag(CWD_PREVSTATE))
        {
            sig_set(sig_lastrx, (((uint32_t)sig_timer & 0x7fffffffu) << 1) | (flag(CWD_PREVSTATE) ? 1u : 0u));
            sig_lastrx = inc(sig_lastrx & (CWDEC_SIG_SIZE - 1));
            sig_timer = 0;
            set(CWD_PREVSTATE, cw_state);
        }
        sig_timer = sig_timer + 1;
        if (sig_timer > one_second * CWDEC_TIMEOUT) sig_timer = one_second * CWDEC_TIMEOUT;
        sig_incount = sig_lastrx;
        cur_time = sig_timer;

        decode();

        /* speed from the PARIS word: 10 dots, 4 dashes, 9 symbol spaces, 5 character spaces */
        const float spdcalc = (float)(10.0 * (double)dot_avg + 4.0 * (double)dash_avg + 9.0 * (double)symspace_avg
                                      + 5.0 * (double)cwspace_avg);
        if (flag(CWD_INITIALIZED) && spdcalc > 0.0f)
        {
            const float ms_per_word = (float)((double)spdcalc * 1000.0 / (double)(12000.0f / blocksize_f));
            const float wpm_raw = (float)(0.5 + 60000.0 / (double)ms_per_word);
            speed_wpm_avg = (float)((double)wpm_raw * 0.3 + 0.7 * (double)speed_wpm_avg);
        }
        else speed_wpm_avg = 0.0f;
        speed = (uint8_t)(uint32_t)cwdec_cvt_i32(speed_wpm_avg);
    }
};

/* a channel over `blocks` blocks; block b's state byte is state[offset + b * step] */
CWD_HD void cwdec_run_channel(const CwDecArena& a, int32_t c, const uint8_t* state, int32_t blocks, int32_t offset,
                              int32_t step, int32_t blocksize, int32_t spikecancel)
{
    CwDec d;
    d.load(a, c, blocksize, spikecancel);
    for (int32_t b = 0; b < blocks; b++) d.step(state[(size_t)offset + (size_t)b * step] != 0);
    d.store(a, c);
}

#endif
