// RTTY and BPSK modulators: batched text-to-audio, channel == lane (uhsdr_rttymod.h and
// uhsdr_pskmod.h have the steps, uhsdr_digiq.h the text queue and the arena).
//
// rttymod_gen / pskmod_gen: a wave's 64 channels load their state (ten or eight words each and the
// queue's three counters) from the field-major arena, each lane runs its state machine over the
// launch's n samples in registers and stores the state back once.  A channel's samples depend on
// each other through the oscillators and the framer, so only channels run in parallel, and
// workgroups are one wave: C / 64 independent waves spread over the CUs.  Lanes diverge wherever
// their texts do; nothing crosses lanes and nothing is atomic.
//
// The 1024-entry sine table is copied to LDS as int16 (2 KiB) at the start of a launch; a step
// reads one or two entries of it.  Text bytes and the code table are read from global memory only
// when a channel loads a character, once in several thousand samples.
//
// The output is [C][stride] int16, channel-major.  Written straight from the lanes it would be one
// 2-byte store per lane per sample, 64 rows apart.  So it goes through an LDS tile, the decoders'
// input staging reversed: lane c writes its sample s to tile[c][s], and after DM_TILE samples the
// wave stores the tile row by row, lane l sample l of the row, 128 contiguous bytes per store
// whatever the row's alignment (a row starts at c * stride + n0 int16, odd for an odd stride).
// The pitch is 66 int16 = 33 words, odd: LDS writes bank by word address mod 32 within each half of
// the wave, and lane c's word 33 c + s / 2 puts the 32 lanes of a half on 32 different banks.  A
// row's read has two neighbouring lanes per word, which is a broadcast and no conflict.
//
// Chosen and not measured: one tile and two barriers per 64 samples instead of a double buffer (the
// stores are not waited for, the wave goes on generating once the tile's LDS reads are done);
// 2-byte global stores per lane instead of dword stores with a scalar head and tail for odd
// alignment; a 64-sample tile (8448 bytes; 10496 bytes of LDS with the table, so LDS does not
// limit occupancy before the wave slots do).
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_digimod_host.h"
#include "uhsdr_psk.h"
#include "uhsdr_rttymod.h"
#include "uhsdr_pskmod.h"

constexpr int DM_WG = 64;
constexpr int DM_TILE = 64;
constexpr int DM_PITCH = DM_TILE + 2;       // int16: 33 words
constexpr int DM_SINE = 1024;

enum { DM_OP_RESET = 0, DM_OP_START };

// what the two modulators differ in
struct RttyMod
{
    typedef RttyModChan Chan;
    typedef RttyModParams Params;
    static constexpr int rows = RTTYMOD_I_COUNT, codes = 128;
    static DIGI_HD void reset(Chan& ch, const Params& p) { ch.reset(p); }
    static DIGI_HD void start(Chan& ch, const Params& p) { ch.start_tx(p); }
};
struct PskMod
{
    typedef PskModChan Chan;
    typedef PskModParams Params;
    static constexpr int rows = PSKMOD_I_COUNT, codes = 256;
    static DIGI_HD void reset(Chan& ch, const Params&) { ch.reset(); }
    static DIGI_HD void start(Chan& ch, const Params&) { ch.prepare_tx(); }
};

// reset or StartTX / PrepareTx of one channel, on either side
template <class M>
DIGI_HD void dm_ctl_one(const DigiModArena& a, const typename M::Params& p, int32_t c, int op)
{
    typename M::Chan ch{};
    if (op == DM_OP_RESET)
    {
        ch.q.load(a, c);
        M::reset(ch, p);
        a.put[c] = 0;
        a.state[c] = 0;
    }
    else
    {
        ch.load(a, c);
        M::start(ch, p);
    }
    ch.store(a, c);
}

template <class M>
__device__ __forceinline__ void dm_gen(const DigiModArena& a, const typename M::Params& p, uint32_t t0, int16_t* __restrict__ out, int n, int stride)
{
    __shared__ int16_t sine[DM_SINE];
    __shared__ int16_t tile[DM_WG * DM_PITCH];
    const int lane = threadIdx.x, c0 = blockIdx.x * DM_WG, c = c0 + lane;
    const bool live = c < a.C;          // the other lanes of a partial last wave still help storing
    const int rows = a.C - c0 < DM_WG ? a.C - c0 : DM_WG;
    {
        const uint32_t* src = (const uint32_t*)a.sine;      // 256-byte aligned in the arena
        uint32_t* dst = (uint32_t*)sine;
        for (int i = lane; i < DM_SINE / 2; i += DM_WG) dst[i] = src[i];
    }
    typename M::Chan ch{};
    if (live) ch.load(a, c);
    __syncthreads();
    for (int n0 = 0; n0 < n; n0 += DM_TILE)
    {
        const int m = n - n0 < DM_TILE ? n - n0 : DM_TILE;
        if (live)
        {
            int16_t* row = tile + lane * DM_PITCH;
            for (int s = 0; s < m; s++) row[s] = ch.step(sine, a.codes, p, t0 + (uint32_t)(n0 + s));
        }
        __syncthreads();
        if (lane < m)
        {
            int16_t* dst = out + (size_t)c0 * stride + n0 + lane;       // n0 + lane < n <= stride, c0 + r < C
#pragma unroll 8
            for (int r = 0; r < rows; r++) dst[(size_t)r * stride] = tile[r * DM_PITCH + lane];
        }
        __syncthreads();
    }
    if (live) ch.store(a, c);
}

__global__ __launch_bounds__(DM_WG) void rttymod_gen(DigiModArena a, RttyModParams p, uint32_t t0, int16_t* __restrict__ out, int n, int stride)
{
    dm_gen<RttyMod>(a, p, t0, out, n, stride);
}

__global__ __launch_bounds__(DM_WG) void pskmod_gen(DigiModArena a, PskModParams p, uint32_t t0, int16_t* __restrict__ out, int n, int stride)
{
    dm_gen<PskMod>(a, p, t0, out, n, stride);
}

template <class M>
__global__ __launch_bounds__(DM_WG) void digimod_ctl(DigiModArena a, typename M::Params p, int op)
{
    const int c = blockIdx.x * DM_WG + threadIdx.x;
    if (c < a.C) dm_ctl_one<M>(a, p, c, op);
}

// the part of a handle both modulators have: DigiMod, uhsdr_digimod_host.h
struct uhsdr_rttymod_s : DigiMod { RttyModParams p; };
struct uhsdr_pskmod_s : DigiMod { PskModParams p; };

template <class M>
static size_t dm_layout(DigiMod* h, char* base)
{
    DigiModArena& a = h->a;
    const size_t C = (size_t)a.C;
    ArenaCarver m{base, 0};
    a.sine = m.take<int16_t>(DM_SINE);
    a.codes = m.take<uint16_t>(M::codes);
    h->tables = m.off;
    a.is = m.take<uint32_t>(M::rows * C);
    a.consumed = m.take<uint32_t>(C);
    a.txoff_at = m.take<uint32_t>(C);
    a.put = m.take<uint32_t>(C);
    a.state = m.take<uint8_t>(C);
    a.text = m.take<uint8_t>(C * (size_t)a.text_capacity);
    return m.off;
}

static void dm_fill_codes(RttyMod, uint16_t* codes) { rttymod_fill_codes(codes); }

// byte -> varicode: the decoder's lookup (uhsdr_psk.h) read backwards
static void dm_fill_codes(PskMod, uint16_t* codes)
{
    static uint8_t chars[PSK_CODES];
    psk_fill_chars(chars);
    for (int k = 0; k < 128; k++) codes[k] = psk_varicode_ascii[k];
    for (int code = 0; code < PSK_CODES; code++) if (chars[code] >= 128) codes[chars[code]] = (uint16_t)code;
}

template <class M>
static void dm_fill_tables(const DigiMod* h, char* dst)
{
    memcpy(dst, uhsdr_dds_table, sizeof(int16_t) * DM_SINE);
    dm_fill_codes(M(), (uint16_t*)(dst + ((const char*)h->a.codes - (const char*)h->a.sine)));
}

uhsdr_status dm_alloc_queues(DigiMod* h, const char* who)
{
    if (h->host) return UHSDR_OK;
    const size_t C = (size_t)h->a.C;
    h->h_put = (uint32_t*)calloc(C, sizeof(uint32_t));
    h->h_consumed = (uint32_t*)calloc(C, sizeof(uint32_t));
    h->h_text = (uint8_t*)calloc(C, (size_t)h->a.text_capacity);
    if (h->h_put && h->h_consumed && h->h_text) return UHSDR_OK;
    uhsdr_set_error("%s: host allocation of the queues failed", who);
    return UHSDR_DEVICE_ERROR;
}

void dm_free(DigiMod* h)
{
    h->release();
    free(h->h_put);         // null in a host handle
    free(h->h_consumed);
    free(h->h_text);
}

template <class M, class H>
static uhsdr_status dm_reset(H* h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const int32_t C = h->a.C;
    if (h->host) for (int32_t c = 0; c < C; c++) dm_ctl_one<M>(h->a, h->p, c, DM_OP_RESET);
    else
    {
        hipLaunchKernelGGL(digimod_ctl<M>, dim3((C + DM_WG - 1) / DM_WG), dim3(DM_WG), 0, h->stream, h->a, h->p, (int)DM_OP_RESET);
        HIPCHK(hipGetLastError());
        memset(h->h_put, 0, sizeof(uint32_t) * (size_t)C);
    }
    h->t = 0;
    return UHSDR_OK;
}

template <class M, class H>
static uhsdr_status dm_start(H* h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const int32_t C = h->a.C;
    if (h->host) for (int32_t c = 0; c < C; c++) dm_ctl_one<M>(h->a, h->p, c, DM_OP_START);
    else
    {
        hipLaunchKernelGGL(digimod_ctl<M>, dim3((C + DM_WG - 1) / DM_WG), dim3(DM_WG), 0, h->stream, h->a, h->p, (int)DM_OP_START);
        HIPCHK(hipGetLastError());
    }
    return UHSDR_OK;
}

// a handle with its memory, tables and state set up; the parameters are already in *h
template <class M, class H>
static uhsdr_status dm_create(H* h, int32_t num_channels, int32_t text_capacity, bool host, void* stream, H** out)
{
    if (!h) { uhsdr_set_error("digimod: host allocation failed"); return UHSDR_DEVICE_ERROR; }
    h->a.C = num_channels;
    h->a.text_capacity = text_capacity;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = dm_layout<M>(h, nullptr);
    uhsdr_status st = h->alloc("digimod");
    if (st == UHSDR_OK)
    {
        dm_layout<M>(h, (char*)h->mem);
        st = dm_alloc_queues(h, "digimod");
    }
    if (st == UHSDR_OK) st = h->upload_tables("digimod", [h](char* image) { dm_fill_tables<M>(h, image); });
    if (st == UHSDR_OK) st = dm_reset<M>(h);
    if (st != UHSDR_OK) { dm_free(h); delete h; return st; }
    *out = h;
    return UHSDR_OK;
}

static uhsdr_status dm_check_create(const char* who, int32_t num_channels, int32_t text_capacity, const void* out)
{
    if (!out || num_channels < 1) { uhsdr_set_error("%s: bad argument", who); return UHSDR_ARGUMENT_ERROR; }
    if (text_capacity < 8) { uhsdr_set_error("%s: text_capacity %d below 8", who, text_capacity); return UHSDR_ARGUMENT_ERROR; }
    return UHSDR_OK;
}

// Appends to every channel's queue what fits of its row.  The free space of a queue depends on what
// the modulator has taken, so a device handle waits for the work enqueued and reads the counters back.
uhsdr_status dm_put_text(DigiMod* h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted)
{
    if (!h || !text || !len) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    const int32_t C = h->a.C;
    const uint32_t cap = (uint32_t)h->a.text_capacity;
    if (stride < 0) { uhsdr_set_error("digimod: stride %d", stride); return UHSDR_LENGTH_ERROR; }
    for (int32_t c = 0; c < C; c++)
        if (len[c] < 0 || len[c] > stride) { uhsdr_set_error("digimod: %d characters do not fit a row of %d", len[c], stride); return UHSDR_LENGTH_ERROR; }
    uint32_t* put = h->host ? h->a.put : h->h_put;
    uint8_t* ring = h->host ? h->a.text : h->h_text;
    const uint32_t* consumed = h->a.consumed;
    if (!h->host)
    {
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(h->h_consumed, h->a.consumed, sizeof(uint32_t) * (size_t)C, hipMemcpyDeviceToHost));
        consumed = h->h_consumed;
    }
    int32_t lo = C, hi = -1;
    for (int32_t c = 0; c < C; c++)
    {
        const uint32_t room = cap - 1u - (put[c] - consumed[c]);
        const uint32_t k = (uint32_t)len[c] < room ? (uint32_t)len[c] : room;
        for (uint32_t i = 0; i < k; i++) ring[(size_t)c * cap + (put[c] + i) % cap] = text[(size_t)c * stride + i];
        put[c] += k;
        if (accepted) accepted[c] = (int32_t)k;
        if (k) { if (c < lo) lo = c; hi = c; }
    }
    if (!h->host && hi >= lo)
    {
        const size_t cnt = (size_t)(hi - lo + 1);
        HIPCHK(hipMemcpyAsync(h->a.text + (size_t)lo * cap, ring + (size_t)lo * cap, cnt * cap, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->a.put + lo, put + lo, sizeof(uint32_t) * cnt, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));     // the host copies may change at the next put
    }
    return UHSDR_OK;
}

static uhsdr_status dm_check_run(const DigiMod* h, const int16_t* audio, int32_t n, int32_t stride)
{
    if (!h || !audio) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    return arena_check_row("digimod", "samples", n, n, stride);
}

template <class M, class H, class K>
static uhsdr_status dm_process(H* h, K kernel, int16_t* audio, int32_t n, int32_t stride)
{
    const uhsdr_status st = dm_check_run(h, audio, n, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, false, "digimod", "the _process_host call")) return UHSDR_ARGUMENT_ERROR;
    if (n == 0) return UHSDR_OK;
    hipLaunchKernelGGL(kernel, dim3((h->a.C + DM_WG - 1) / DM_WG), dim3(DM_WG), 0, h->stream, h->a, h->p, h->t, audio, (int)n, (int)stride);
    HIPCHK(hipGetLastError());
    h->t += (uint32_t)n;
    return UHSDR_OK;
}

template <class M, class H>
static uhsdr_status dm_process_host(H* h, int16_t* audio, int32_t n, int32_t stride)
{
    const uhsdr_status st = dm_check_run(h, audio, n, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, true, "digimod", "the _process call")) return UHSDR_ARGUMENT_ERROR;
    for (int32_t c = 0; c < h->a.C; c++)
    {
        typename M::Chan ch{};
        ch.load(h->a, c);
        int16_t* row = audio + (size_t)c * stride;
        for (int32_t i = 0; i < n; i++) row[i] = ch.step(h->a.sine, h->a.codes, h->p, h->t + (uint32_t)i);
        ch.store(h->a, c);
    }
    h->t += (uint32_t)n;
    return UHSDR_OK;
}

static uhsdr_status dm_outputs(DigiMod* h, uint32_t** consumed, uint32_t** txoff_at, uint8_t** state)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    if (consumed) *consumed = h->a.consumed;
    if (txoff_at) *txoff_at = h->a.txoff_at;
    if (state) *state = h->a.state;
    return UHSDR_OK;
}

// ---- RTTY ----

static uhsdr_status rttymod_new(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx, int32_t text_capacity,
                                bool host, void* stream, uhsdr_rttymod_handle* out)
{
    const uhsdr_status st = dm_check_create("rttymod", num_channels, text_capacity, out);
    if (st != UHSDR_OK) return st;
    if (shift_idx < 0 || shift_idx >= RTTYMOD_SHIFT_COUNT || speed_idx < 0 || speed_idx >= RTTYMOD_SPEED_COUNT ||
        stopbits_idx < 0 || stopbits_idx >= RTTYMOD_STOP_COUNT)
    {
        uhsdr_set_error("rttymod: shift_idx %d, speed_idx %d, stopbits_idx %d not 0 .. 5, 0 .. 1, 0 .. 2", shift_idx, speed_idx, stopbits_idx);
        return UHSDR_ARGUMENT_ERROR;
    }
    uhsdr_rttymod_s* h = new (std::nothrow) uhsdr_rttymod_s();
    if (h) h->p = rttymod_params(shift_idx, speed_idx, stopbits_idx);
    return dm_create<RttyMod>(h, num_channels, text_capacity, host, stream, out);
}

extern "C" uhsdr_status uhsdr_rttymod_create(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                             int32_t text_capacity, void* stream, uhsdr_rttymod_handle* out)
{
    return rttymod_new(num_channels, shift_idx, speed_idx, stopbits_idx, text_capacity, false, stream, out);
}

extern "C" uhsdr_status uhsdr_rttymod_create_host(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                                  int32_t text_capacity, uhsdr_rttymod_handle* out)
{
    return rttymod_new(num_channels, shift_idx, speed_idx, stopbits_idx, text_capacity, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_rttymod_reset(uhsdr_rttymod_handle h) { return dm_reset<RttyMod>(h); }
extern "C" uhsdr_status uhsdr_rttymod_start_tx(uhsdr_rttymod_handle h) { return dm_start<RttyMod>(h); }
extern "C" uhsdr_status uhsdr_rttymod_put_text(uhsdr_rttymod_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted)
{
    return dm_put_text(h, text, len, stride, accepted);
}
extern "C" uhsdr_status uhsdr_rttymod_process(uhsdr_rttymod_handle h, int16_t* audio, int32_t n, int32_t stride)
{
    return dm_process<RttyMod>(h, rttymod_gen, audio, n, stride);
}
extern "C" uhsdr_status uhsdr_rttymod_process_host(uhsdr_rttymod_handle h, int16_t* audio, int32_t n, int32_t stride)
{
    return dm_process_host<RttyMod>(h, audio, n, stride);
}
extern "C" uhsdr_status uhsdr_rttymod_outputs(uhsdr_rttymod_handle h, uint32_t** consumed, uint32_t** txoff_at, uint8_t** state)
{
    return dm_outputs(h, consumed, txoff_at, state);
}
extern "C" uhsdr_status uhsdr_rttymod_set_stream(uhsdr_rttymod_handle h, void* stream) { return dm_set_stream(h, stream); }
extern "C" uhsdr_status uhsdr_rttymod_synchronize(uhsdr_rttymod_handle h) { return dm_synchronize(h); }
extern "C" uhsdr_status uhsdr_rttymod_destroy(uhsdr_rttymod_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    dm_free(h);
    delete h;
    return UHSDR_OK;
}

// ---- BPSK ----

static uhsdr_status pskmod_new(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, bool host, void* stream, uhsdr_pskmod_handle* out)
{
    const uhsdr_status st = dm_check_create("pskmod", num_channels, text_capacity, out);
    if (st != UHSDR_OK) return st;
    if (speed_idx < 0 || speed_idx >= PSKMOD_SPEED_COUNT) { uhsdr_set_error("pskmod: speed_idx %d not 0 .. 2", speed_idx); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_pskmod_s* h = new (std::nothrow) uhsdr_pskmod_s();
    if (h) h->p = pskmod_params(speed_idx);
    return dm_create<PskMod>(h, num_channels, text_capacity, host, stream, out);
}

extern "C" uhsdr_status uhsdr_pskmod_create(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, void* stream, uhsdr_pskmod_handle* out)
{
    return pskmod_new(num_channels, speed_idx, text_capacity, false, stream, out);
}

extern "C" uhsdr_status uhsdr_pskmod_create_host(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, uhsdr_pskmod_handle* out)
{
    return pskmod_new(num_channels, speed_idx, text_capacity, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_pskmod_reset(uhsdr_pskmod_handle h) { return dm_reset<PskMod>(h); }
extern "C" uhsdr_status uhsdr_pskmod_prepare_tx(uhsdr_pskmod_handle h) { return dm_start<PskMod>(h); }
extern "C" uhsdr_status uhsdr_pskmod_put_text(uhsdr_pskmod_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted)
{
    return dm_put_text(h, text, len, stride, accepted);
}
extern "C" uhsdr_status uhsdr_pskmod_process(uhsdr_pskmod_handle h, int16_t* audio, int32_t n, int32_t stride)
{
    return dm_process<PskMod>(h, pskmod_gen, audio, n, stride);
}
extern "C" uhsdr_status uhsdr_pskmod_process_host(uhsdr_pskmod_handle h, int16_t* audio, int32_t n, int32_t stride)
{
    return dm_process_host<PskMod>(h, audio, n, stride);
}
extern "C" uhsdr_status uhsdr_pskmod_outputs(uhsdr_pskmod_handle h, uint32_t** consumed, uint32_t** txoff_at, uint8_t** state)
{
    return dm_outputs(h, consumed, txoff_at, state);
}
extern "C" uhsdr_status uhsdr_pskmod_set_stream(uhsdr_pskmod_handle h, void* stream) { return dm_set_stream(h, stream); }
extern "C" uhsdr_status uhsdr_pskmod_synchronize(uhsdr_pskmod_handle h) { return dm_synchronize(h); }
extern "C" uhsdr_status uhsdr_pskmod_destroy(uhsdr_pskmod_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    dm_free(h);
    delete h;
    return UHSDR_OK;
}
