// RTTY decoder: batched Baudot-to-text, channel == lane (uhsdr_rtty.h has the step).
//
// rtty_decode: a wave's 64 channels load their state (33 words each) from the field-major arena,
// each lane runs its own filters and framer over the launch's samples in registers and stores the
// state back.  The recursion is serial per channel, so only channels run in parallel, and
// workgroups are one wave: C / 64 independent waves spread over the CUs.
//
// The input is [C][stride], channel-major: a lane walking its own row would touch 4 bytes of a
// different 128-byte line per load.  So the wave stages the launch in tiles of RTTY_TILE samples
// through LDS: it reads each channel's 128-byte row segment coalesced (a half-wave per segment),
// writes it to tile[channel][RTTY_PITCH] -- a half-wave writes 32 consecutive dwords, all banks --
// and lane c then reads tile[c][s].  RTTY_PITCH is odd, so the 32 lanes of a ds_read_b32 group are
// on 32 different banks (bank = (c * 33 + s) mod 32 = (c + s) mod 32).  The next tile's global
// loads are issued before the current tile's arithmetic and land in the other LDS buffer after it.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_rtty.h"

constexpr int RTTY_WG = 64;
constexpr int RTTY_TILE = 32;
constexpr int RTTY_PITCH = RTTY_TILE + 1;
constexpr int RTTY_PER_LANE = RTTY_TILE;       // RTTY_WG * RTTY_TILE elements over RTTY_WG lanes

// The tile at sample n0 into registers: element e = i * 64 + lane is sample e % 32 of channel e / 32 of
// the wave.  Rows past the last channel and samples past n are clamped to the last valid ones, so
// every load is inside [0, C) x [0, n) and none is predicated; what they fetch is never decoded.
__device__ __forceinline__ void rtty_fetch(float (&r)[RTTY_PER_LANE], const float* __restrict__ in, int c0, int C, int n0, int n,
                                           int stride)
{
    const int s = threadIdx.x % RTTY_TILE, half = threadIdx.x / RTTY_TILE;
    const int col = n0 + s < n ? n0 + s : n - 1;
    const int last = C - 1 - c0 - half;          // the highest 2 * i of a valid row
#pragma unroll
    for (int i = 0; i < RTTY_PER_LANE; i++)
    {
        const int row = c0 + half + (2 * i < last ? 2 * i : (last < 0 ? -half : last));
        r[i] = in[(size_t)row * stride + col];
    }
}

__device__ __forceinline__ void rtty_stage(float* tile, const float (&r)[RTTY_PER_LANE])
{
    const int s = threadIdx.x % RTTY_TILE, half = threadIdx.x / RTTY_TILE;
#pragma unroll
    for (int i = 0; i < RTTY_PER_LANE; i++) tile[(2 * i + half) * RTTY_PITCH + s] = r[i];
}

__global__ __launch_bounds__(RTTY_WG) void rtty_decode(RttyArena a, RttyParams p, const float* __restrict__ in, int n, int stride)
{
    __shared__ float tiles[2][RTTY_WG * RTTY_PITCH];
    const int c0 = blockIdx.x * RTTY_WG, c = c0 + threadIdx.x;
    const bool live = c < a.C;          // the other lanes of a partial last wave still help staging
    RttyChan ch;
    if (live) ch.load(a, c);
    float r[RTTY_PER_LANE];
    rtty_fetch(r, in, c0, a.C, 0, n, stride);
    rtty_stage(tiles[0], r);
    __syncthreads();
    for (int n0 = 0, t = 0; n0 < n; n0 += RTTY_TILE, t ^= 1)
    {
        const bool more = n0 + RTTY_TILE < n;
        if (more) rtty_fetch(r, in, c0, a.C, n0 + RTTY_TILE, n, stride);
        if (live)
        {
            const float* row = tiles[t] + threadIdx.x * RTTY_PITCH;
            const int m = n - n0 < RTTY_TILE ? n - n0 : RTTY_TILE;
            for (int s = 0; s < m; s++) ch.step(row[s], p);
        }
        if (more) rtty_stage(tiles[t ^ 1], r);      // last read two tiles ago, before the previous barrier
        __syncthreads();
    }
    if (live) ch.store(a, c);
}

struct uhsdr_rtty_s : ArenaMem
{
    RttyArena a;
    RttyParams p;
};

static size_t rtty_layout(RttyArena& a, char* base)
{
    const size_t C = (size_t)a.C;
    ArenaCarver m{base, 0};
    a.fs = m.take<float>(RTTY_F_COUNT * C);
    a.is = m.take<int32_t>(RTTY_I_COUNT * C);
    a.total = m.take<uint32_t>(C);
    a.text = m.take<uint8_t>(C * (size_t)a.text_capacity);
    return m.off;
}

// every static of the firmware's decoder starts at zero
extern "C" uhsdr_status uhsdr_rtty_reset(uhsdr_rtty_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    return h->zero_state();
}

static uhsdr_status rtty_create(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx, int32_t atc_disable,
                                int32_t text_capacity, bool host, void* stream, uhsdr_rtty_handle* out)
{
    if (!out || num_channels < 1) { uhsdr_set_error("rtty: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    if (shift_idx < 0 || shift_idx >= RTTY_SHIFT_COUNT) { uhsdr_set_error("rtty: shift_idx %d not 0 .. 5", shift_idx); return UHSDR_ARGUMENT_ERROR; }
    if (speed_idx < 0 || speed_idx >= RTTY_SPEED_COUNT) { uhsdr_set_error("rtty: speed_idx %d not 0 .. 1", speed_idx); return UHSDR_ARGUMENT_ERROR; }
    if (stopbits_idx < 0 || stopbits_idx >= RTTY_STOP_COUNT) { uhsdr_set_error("rtty: stopbits_idx %d not 0 .. 2", stopbits_idx); return UHSDR_ARGUMENT_ERROR; }
    if (text_capacity < 8) { uhsdr_set_error("rtty: text_capacity %d below 8", text_capacity); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_rtty_s* h = new (std::nothrow) uhsdr_rtty_s();
    if (!h) return UHSDR_DEVICE_ERROR;
    h->a.C = num_channels;
    h->a.text_capacity = text_capacity;
    h->p = rtty_params(shift_idx, speed_idx, stopbits_idx, atc_disable);
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = rtty_layout(h->a, nullptr);
    uhsdr_status st = h->alloc("rtty");
    if (st == UHSDR_OK)
    {
        rtty_layout(h->a, (char*)h->mem);
        st = h->zero_state();
    }
    if (st != UHSDR_OK) { uhsdr_rtty_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_rtty_create(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                          int32_t atc_disable, int32_t text_capacity, void* stream, uhsdr_rtty_handle* out)
{
    return rtty_create(num_channels, shift_idx, speed_idx, stopbits_idx, atc_disable, text_capacity, false, stream, out);
}

extern "C" uhsdr_status uhsdr_rtty_create_host(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                               int32_t atc_disable, int32_t text_capacity, uhsdr_rtty_handle* out)
{
    return rtty_create(num_channels, shift_idx, speed_idx, stopbits_idx, atc_disable, text_capacity, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_rtty_destroy(uhsdr_rtty_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_rtty_set_stream(uhsdr_rtty_handle h, void* stream) { return arena_set_stream(h, "rtty", stream, false); }

static uhsdr_status rtty_check_run(uhsdr_rtty_handle h, const float* samples, int32_t n, int32_t stride)
{
    if (!h || !samples) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    return arena_check_row("rtty", "samples", n, n, stride);
}

extern "C" uhsdr_status uhsdr_rtty_process(uhsdr_rtty_handle h, const float* samples, int32_t n, int32_t stride)
{
    const uhsdr_status st = rtty_check_run(h, samples, n, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, false, "rtty", "uhsdr_rtty_process_host")) return UHSDR_ARGUMENT_ERROR;
    if (n == 0) return UHSDR_OK;
    const int grid = (h->a.C + RTTY_WG - 1) / RTTY_WG;
    hipLaunchKernelGGL(rtty_decode, dim3(grid), dim3(RTTY_WG), 0, h->stream, h->a, h->p, samples, n, stride);
    HIPCHK(hipGetLastError());
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_rtty_process_host(uhsdr_rtty_handle h, const float* samples, int32_t n, int32_t stride)
{
    const uhsdr_status st = rtty_check_run(h, samples, n, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, true, "rtty", "uhsdr_rtty_process")) return UHSDR_ARGUMENT_ERROR;
    for (int32_t c = 0; c < h->a.C; c++) rtty_run_channel(h->a, c, h->p, samples + (size_t)c * stride, n);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_rtty_outputs(uhsdr_rtty_handle h, uint8_t** text, uint32_t** total)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    if (text) *text = h->a.text;
    if (total) *total = h->a.total;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_rtty_synchronize(uhsdr_rtty_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}
