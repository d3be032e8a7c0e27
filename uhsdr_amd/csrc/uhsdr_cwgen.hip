// CW generator: batched keyer and tone generator, channel == lane (uhsdr_cwgen.h has the block
// function and the sample function, uhsdr_digiq.h the text queue).
//
// cwgen_gen: a wave's 64 channels load their state (eleven words each, the queue's counters and the
// echo count) from the field-major arena.  Per 32-sample block every lane runs the keyer once (the
// firmware's CwGen_Process is called once per block; lanes diverge in it, but it is a few dozen
// integer instructions and touches no sample) and gets a plan: tone or silence, the accumulator at
// the block's start, the envelope pointer each shaper starts with.  The lanes then write their 32
// I and 32 Q samples from the plan, and the state goes back once at the end of the launch.  Only
// channels run in parallel; nothing crosses lanes and nothing is atomic.
//
// The 1024-entry sine table (int16, 2 KiB) and the 128-entry envelope (f32, 512 B) are copied to
// LDS at the start of a launch.  Text bytes, the byte -> code table and the code -> character table
// are read from global memory only where a channel takes or prints a character.
//
// The outputs are f32 [C][stride], channel-major.  Written straight from the lanes they would be one
// 4-byte store per lane per sample, 64 rows apart.  So a block goes through two LDS tiles, as dm_gen
// (uhsdr_digimod.hip) does it: lane c writes sample s to tile[c][s], and the wave stores row by row,
// lanes 0..31 the 32 I samples of a row and lanes 32..63 its 32 Q samples, 128 contiguous bytes
// each.  The pitch is 33 words, odd: ds_write_b32 banks by word address mod 32 within each half of
// the wave, and lane c's word 33 c + s puts a half's lanes on 32 different banks; a row's read is
// 32 consecutive words.
//
// Occupancy: 19456 bytes of LDS per one-wave workgroup (2 KiB sine, 512 B envelope, two 64 x 33 f32
// tiles) let 8 workgroups share a CU's 160 KiB, 2 waves per SIMD, where 76 VGPRs would allow 6: LDS is
// the limit.  The kernel is store-bound (8 bytes out per sample against a table look-up and at most
// two multiplies), and at 262144 channels it writes 4.3 TB/s (profiles/r11_cwgen_throughput.jsonl), so
// more waves per SIMD were not needed to reach the memory system's rate.  Not tried: 128 or 256
// channels per workgroup sharing one copy of the tables, or half-block tiles.  The 60 SGPR spills
// (profiles/r11_kres.txt) go to VGPR lanes, not to scratch; they come from the arena's twelve
// pointers and the launch constants, which are live across the block loop.
// Chosen and not measured: one block per tile and two barriers per block; key bytes and flag bytes read and written by their lanes, one byte per channel per block, 1/256 of
// the sample traffic.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_cwgen_host.h"
#include "uhsdr_cwgen_tables.h"

constexpr int CG_WG = 64;
constexpr int CG_PITCH = CWGEN_BLOCK + 1;
constexpr int CG_SINE = 1024;
constexpr int CG_SEND = 256;

__global__ __launch_bounds__(CG_WG) void cwgen_gen(CwGenArena a, CwGenParams p, const uint8_t* __restrict__ keys, float* __restrict__ out_i,
                                                   float* __restrict__ out_q, uint8_t* __restrict__ flags, int blocks, int stride)
{
    __shared__ int16_t sine[CG_SINE];
    __shared__ float env[CWGEN_ENV_SIZE];
    __shared__ float tile[2][CG_WG * CG_PITCH];
    const int lane = threadIdx.x, c0 = blockIdx.x * CG_WG, c = c0 + lane;
    const bool live = c < a.m.C;            // the other lanes of a partial last wave still help storing
    const int rows = a.m.C - c0 < CG_WG ? a.m.C - c0 : CG_WG;
    {
        const uint32_t* src = (const uint32_t*)a.m.sine;        // 256-byte aligned in the arena
        uint32_t* dst = (uint32_t*)sine;
        for (int i = lane; i < CG_SINE / 2; i += CG_WG) dst[i] = src[i];
        for (int i = lane; i < CWGEN_ENV_SIZE; i += CG_WG) env[i] = a.env[i];
    }
    CwGenChan ch{};
    if (live) ch.load(a, c);
    __syncthreads();
    const int half = lane >> 5, s_out = lane & 31;
    float* const out = half ? out_q : out_i;
    for (int b = 0; b < blocks; b++)
    {
        if (live)
        {
            const size_t kb = (size_t)c * blocks + b;               // c < C, b < blocks
            const CwGenBlock plan = ch.block(a, p, c, keys[kb]);
            flags[kb] = (uint8_t)plan.flags;
            float* ri = tile[0] + lane * CG_PITCH;
            float* rq = tile[1] + lane * CG_PITCH;
            if (plan.flags & CWGEN_F_ACTIVE)
                for (int s = 0; s < CWGEN_BLOCK; s++) cwgen_sample(plan, p.step, s, sine, env, ri[s], rq[s]);
            else
                for (int s = 0; s < CWGEN_BLOCK; s++) ri[s] = rq[s] = 0.0f;
        }
        __syncthreads();
        {
            float* dst = out + (size_t)c0 * stride + (size_t)b * CWGEN_BLOCK + s_out;     // 32 b + s_out < n <= stride, c0 + r < C
            const float* src = tile[half] + s_out;
#pragma unroll 8
            for (int r = 0; r < rows; r++) dst[(size_t)r * stride] = src[r * CG_PITCH];
        }
        __syncthreads();
    }
    if (live) ch.store(a, c, p);
}

__global__ __launch_bounds__(CG_WG) void cwgen_reset(CwGenArena a, CwGenParams p)
{
    const int c = blockIdx.x * CG_WG + threadIdx.x;
    if (c >= a.m.C) return;
    CwGenChan ch{};
    ch.q.load(a.m, c);
    ch.reset();
    a.m.put[c] = 0;
    ch.store(a, c, p);
}

static size_t cg_layout(uhsdr_cwgen_s* h, char* base)
{
    CwGenArena& a = h->ca;
    const size_t C = (size_t)a.m.C;
    ArenaCarver m{base, 0};
    a.m.sine = m.take<int16_t>(CG_SINE);
    a.m.codes = m.take<uint16_t>(CG_SEND);
    a.env = m.take<float>(CWGEN_ENV_SIZE);
    a.dec_code = m.take<uint32_t>(CWGEN_DEC_MAX);
    a.dec_out = m.take<uint32_t>(CWGEN_DEC_MAX);
    h->tables = m.off;
    a.m.is = m.take<uint32_t>(CWGEN_I_COUNT * C);
    a.m.consumed = m.take<uint32_t>(C);
    a.m.txoff_at = m.take<uint32_t>(C);
    a.m.put = m.take<uint32_t>(C);
    a.echo_total = m.take<uint32_t>(C);
    a.m.state = m.take<uint8_t>(C);
    a.m.text = m.take<uint8_t>(C * (size_t)a.m.text_capacity);
    a.echo = m.take<uint8_t>(C * (size_t)a.echo_capacity);
    h->a = a.m;
    return m.off;
}

// CwGen_ReverseCode: the elements in sending order, the first one lowest
static uint32_t cg_reverse(uint32_t code)
{
    uint32_t r = 0;
    for (; code > 0; code /= 4) r = r * 4 + code % 4;
    return r;
}

static_assert(CWGEN_CHARS + CWGEN_SIGNS <= CWGEN_DEC_MAX, "code tables do not fit");

static void cg_fill_tables(const uhsdr_cwgen_s* h, char* dst)
{
    const CwGenArena& a = h->ca;
    const char* base = (const char*)a.m.sine;
    memcpy(dst, uhsdr_dds_table, sizeof(int16_t) * CG_SINE);
    uint16_t* send = (uint16_t*)(dst + ((const char*)a.m.codes - base));
    for (int k = 0; k < CG_SEND; k++) send[k] = 0;
    for (int k = CWGEN_CHARS - 1; k >= 0; k--) send[cwgen_char_chars[k]] = (uint16_t)cg_reverse(cwgen_char_codes[k]);     // the first entry of a character wins
    for (int k = 'a'; k <= 'z'; k++) send[k] = send[k - 32];
    memcpy(dst + ((const char*)a.env - base), cwgen_env_bits, sizeof(float) * CWGEN_ENV_SIZE);
    uint32_t* code = (uint32_t*)(dst + ((const char*)a.dec_code - base));
    uint32_t* out = (uint32_t*)(dst + ((const char*)a.dec_out - base));
    for (int k = 0; k < CWGEN_CHARS; k++) { code[k] = cwgen_char_codes[k]; out[k] = cwgen_char_chars[k]; }
    for (int k = 0; k < CWGEN_SIGNS; k++)
    {
        code[CWGEN_CHARS + k] = cwgen_sign_codes[k];
        out[CWGEN_CHARS + k] = (uint32_t)'<' | (uint32_t)cwgen_sign_chars[k][0] << 8 | (uint32_t)cwgen_sign_chars[k][1] << 16 | (uint32_t)'>' << 24;
    }
}

static void cg_free(uhsdr_cwgen_s* h)
{
    dm_free(h);
    if (h->host) free(h->flags);
    else (void)hipFree(h->flags);
    delete h;
}

static uhsdr_status cg_check_speed(int32_t speed, int32_t weight)
{
    if (speed < 5 || speed > 48 || weight < 50 || weight > 150)
    {
        uhsdr_set_error("cwgen: keyer_speed %d, keyer_weight %d not 5 .. 48, 50 .. 150", speed, weight);
        return UHSDR_ARGUMENT_ERROR;
    }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_reset(uhsdr_cwgen_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const int32_t C = h->a.C;
    if (h->host)
        for (int32_t c = 0; c < C; c++)
        {
            CwGenChan ch{};
            ch.q.load(h->a, c);
            ch.reset();
            h->a.put[c] = 0;
            ch.store(h->ca, c, h->p);
        }
    else
    {
        hipLaunchKernelGGL(cwgen_reset, dim3((C + CG_WG - 1) / CG_WG), dim3(CG_WG), 0, h->stream, h->ca, h->p);
        HIPCHK(hipGetLastError());
        memset(h->h_put, 0, sizeof(uint32_t) * (size_t)C);
    }
    h->t = 0;
    return UHSDR_OK;
}

static uhsdr_status cwgen_new(int32_t num_channels, const uhsdr_cwgen_config* cfg, int32_t text_capacity, int32_t echo_capacity, bool host,
                              void* stream, uhsdr_cwgen_handle* out)
{
    if (!out || !cfg || num_channels < 1) { uhsdr_set_error("cwgen: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    if (text_capacity < 8 || echo_capacity < 8) { uhsdr_set_error("cwgen: text_capacity %d or echo_capacity %d below 8", text_capacity, echo_capacity); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->keyer_mode < CWGEN_MODE_IAM_B || cfg->keyer_mode > CWGEN_MODE_ULTIMATE || cfg->rx_delay < 0 || cfg->rx_delay > 50 ||
        cfg->sidetone_freq < 400 || cfg->sidetone_freq > 1000)
    {
        uhsdr_set_error("cwgen: keyer_mode %d, rx_delay %d, sidetone_freq %d not 0 .. 3, 0 .. 50, 400 .. 1000", cfg->keyer_mode, cfg->rx_delay, cfg->sidetone_freq);
        return UHSDR_ARGUMENT_ERROR;
    }
    const uhsdr_status ss = cg_check_speed(cfg->keyer_speed, cfg->keyer_weight);
    if (ss != UHSDR_OK) return ss;
    uhsdr_cwgen_s* h = new (std::nothrow) uhsdr_cwgen_s();
    if (!h) { uhsdr_set_error("cwgen: host allocation failed"); return UHSDR_DEVICE_ERROR; }
    h->p.mode = cfg->keyer_mode;
    h->p.reverse = cfg->paddle_reverse != 0;
    h->p.break_time = cfg->rx_delay * 50 + 1;
    h->p.step = digi_dds_step((float)cfg->sidetone_freq, 48000);
    cwgen_set_speed(h->p, cfg->keyer_speed, cfg->keyer_weight);
    h->ca.m.C = num_channels;
    h->ca.m.text_capacity = text_capacity;
    h->ca.echo_capacity = echo_capacity;
    h->ca.dec_chars = CWGEN_CHARS;
    h->ca.dec_count = CWGEN_CHARS + CWGEN_SIGNS;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = cg_layout(h, nullptr);
    uhsdr_status st = h->alloc("cwgen");
    if (st == UHSDR_OK)
    {
        cg_layout(h, (char*)h->mem);
        st = dm_alloc_queues(h, "cwgen");
    }
    if (st == UHSDR_OK) st = h->upload_tables("cwgen", [h](char* image) { cg_fill_tables(h, image); });
    if (st == UHSDR_OK) st = uhsdr_cwgen_reset(h);
    if (st != UHSDR_OK) { cg_free(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_create(int32_t num_channels, const uhsdr_cwgen_config* cfg, int32_t text_capacity, int32_t echo_capacity,
                                           void* stream, uhsdr_cwgen_handle* out)
{
    return cwgen_new(num_channels, cfg, text_capacity, echo_capacity, false, stream, out);
}

extern "C" uhsdr_status uhsdr_cwgen_create_host(int32_t num_channels, const uhsdr_cwgen_config* cfg, int32_t text_capacity, int32_t echo_capacity,
                                                uhsdr_cwgen_handle* out)
{
    return cwgen_new(num_channels, cfg, text_capacity, echo_capacity, true, nullptr, out);
}

// the launch constants travel with every launch, so a change is ordered between two process calls
extern "C" uhsdr_status uhsdr_cwgen_set_speed(uhsdr_cwgen_handle h, int32_t speed, int32_t weight)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status ss = cg_check_speed(speed, weight);
    if (ss != UHSDR_OK) return ss;
    cwgen_set_speed(h->p, speed, weight);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_put_text(uhsdr_cwgen_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted)
{
    return dm_put_text(h, text, len, stride, accepted);
}

uhsdr_status cg_flags_room(uhsdr_cwgen_s* h, int32_t blocks)
{
    if (blocks <= h->flag_blocks) return UHSDR_OK;
    const size_t bytes = (size_t)h->a.C * blocks;
    if (h->host)
    {
        uint8_t* f = (uint8_t*)realloc(h->flags, bytes);
        if (!f) { uhsdr_set_error("cwgen: host allocation of %zu bytes failed", bytes); return UHSDR_DEVICE_ERROR; }
        h->flags = f;
    }
    else
    {
        HIPCHK(hipStreamSynchronize(h->stream));        // an earlier call may still write the old one
        uint8_t* f = nullptr;
        HIPCHK(hipMalloc((void**)&f, bytes));
        (void)hipFree(h->flags);
        h->flags = f;
    }
    h->flag_blocks = blocks;
    return UHSDR_OK;
}

static uhsdr_status cg_check_run(uhsdr_cwgen_s* h, const uint8_t* keys, const float* i, const float* q, int32_t n, int32_t stride, bool host)
{
    if (!h || !keys || !i || !q) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = arena_check_row("cwgen", "samples", n, n, stride);
    if (st != UHSDR_OK) return st;
    if (n % CWGEN_BLOCK) { uhsdr_set_error("cwgen: %d samples are not a multiple of %d", n, CWGEN_BLOCK); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, host, "cwgen", host ? "the _process call" : "the _process_host call")) return UHSDR_ARGUMENT_ERROR;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_process(uhsdr_cwgen_handle h, const uint8_t* keys, float* i, float* q, int32_t n, int32_t stride)
{
    const uhsdr_status st = cg_check_run(h, keys, i, q, n, stride, false);
    if (st != UHSDR_OK) return st;
    if (n == 0) return UHSDR_OK;
    const int32_t blocks = n / CWGEN_BLOCK;
    const uhsdr_status fs = cg_flags_room(h, blocks);
    if (fs != UHSDR_OK) return fs;
    hipLaunchKernelGGL(cwgen_gen, dim3((h->a.C + CG_WG - 1) / CG_WG), dim3(CG_WG), 0, h->stream, h->ca, h->p, keys, i, q, h->flags, (int)blocks, (int)stride);
    HIPCHK(hipGetLastError());
    h->t += (uint32_t)n;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_process_host(uhsdr_cwgen_handle h, const uint8_t* keys, float* i, float* q, int32_t n, int32_t stride)
{
    const uhsdr_status st = cg_check_run(h, keys, i, q, n, stride, true);
    if (st != UHSDR_OK) return st;
    if (n == 0) return UHSDR_OK;
    const int32_t blocks = n / CWGEN_BLOCK;
    const uhsdr_status fs = cg_flags_room(h, blocks);
    if (fs != UHSDR_OK) return fs;
    const float* env = h->ca.env;
    for (int32_t c = 0; c < h->a.C; c++)
    {
        CwGenChan ch{};
        ch.load(h->ca, c);
        for (int32_t b = 0; b < blocks; b++)
        {
            const size_t kb = (size_t)c * blocks + b;
            const CwGenBlock plan = ch.block(h->ca, h->p, c, keys[kb]);
            h->flags[kb] = (uint8_t)plan.flags;
            float* ri = i + (size_t)c * stride + (size_t)b * CWGEN_BLOCK;
            float* rq = q + (size_t)c * stride + (size_t)b * CWGEN_BLOCK;
            for (int32_t s = 0; s < CWGEN_BLOCK; s++)
            {
                if (plan.flags & CWGEN_F_ACTIVE) cwgen_sample(plan, h->p.step, s, h->a.sine, env, ri[s], rq[s]);
                else ri[s] = rq[s] = 0.0f;
            }
        }
        ch.store(h->ca, c, h->p);
    }
    h->t += (uint32_t)n;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_outputs(uhsdr_cwgen_handle h, uint8_t** flags, uint32_t** consumed, uint8_t** echo, uint32_t** echo_total, uint8_t** state)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    if (flags) *flags = h->flags;
    if (consumed) *consumed = h->a.consumed;
    if (echo) *echo = h->ca.echo;
    if (echo_total) *echo_total = h->ca.echo_total;
    if (state) *state = h->a.state;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_peek(uhsdr_cwgen_handle h, uint32_t** words, int32_t* rows)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    if (words) *words = h->a.is;
    if (rows) *rows = CWGEN_I_COUNT;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwgen_set_stream(uhsdr_cwgen_handle h, void* stream) { return dm_set_stream(h, stream); }
extern "C" uhsdr_status uhsdr_cwgen_synchronize(uhsdr_cwgen_handle h) { return dm_synchronize(h); }
extern "C" uhsdr_status uhsdr_cwgen_destroy(uhsdr_cwgen_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    cg_free(h);
    return UHSDR_OK;
}
