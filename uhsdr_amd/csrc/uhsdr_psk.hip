// BPSK decoder: batched varicode-to-text, channel == lane (uhsdr_psk.h has the step).
//
// psk_decode: a wave's 64 channels load their state (13 words each, and the product ring) from the
// field-major arena, each lane runs its band-pass, mixer and framer over the launch's samples in
// registers and stores the state back.  The recursion is serial per channel, so only channels run in parallel, and
// workgroups are one wave: C / 64 independent waves spread over the CUs.
//
// The clock (oscillator accumulator, rx_phase, ring index, strobe count) is the same for every
// channel: the host keeps it per handle, advances it with psk_tick after each launch and passes the
// start values as kernel arguments, so the kernel's copy is wave-uniform and the branch of the bit
// decision is taken by the whole wave or not at all.
//
// The input is [C][stride], channel-major, and is staged through LDS in tiles of PSK_TILE samples
// exactly as rtty_decode does it (uhsdr_rtty.hip): coalesced 128-byte row segments, written to
// tile[channel][PSK_PITCH] with an odd pitch so lane c's read of tile[c][s] is conflict-free, the
// next tile's global loads issued before the current tile's arithmetic.  Row 64 of a tile holds the
// oscillator's 32 values of that tile, gathered from the table by 32 lanes with the tile's loads;
// every lane reads the same word of it per sample, a broadcast.
//
// The 24-entry product ring of a channel lives in LDS as ring[slot][lane]: the slot is uniform, so
// the wave reads and writes 64 consecutive words.  A launch moves only the slots it touches, at most
// 24 and n of them on a short call, between the arena and LDS.  The slot of the next sample is read
// before the current sample's arithmetic (it is never the slot the sample writes), so the read's
// latency is not on the recursion's path.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_psk.h"

constexpr int PSK_WG = 64;
constexpr int PSK_TILE = 32;
constexpr int PSK_PITCH = PSK_TILE + 1;
constexpr int PSK_PER_LANE = PSK_TILE;         // PSK_WG * PSK_TILE elements over PSK_WG lanes
constexpr int PSK_TILE_WORDS = (PSK_WG + 1) * PSK_PITCH;

// The tile at sample n0 into registers: element e = i * 64 + lane is sample e % 32 of channel e / 32 of
// the wave.  Rows past the last channel and samples past n are clamped to the last valid ones, so
// every load is inside [0, C) x [0, n) and none is predicated; what they fetch is never decoded.
// vco: the oscillator's value of sample n0 + lane % 32, acc the accumulator at sample n0.
__device__ __forceinline__ void psk_fetch(float (&r)[PSK_PER_LANE], float& vco, const float* __restrict__ in, const float* __restrict__ sine,
                                          uint32_t acc, int c0, int C, int n0, int n, int stride)
{
    const int s = threadIdx.x % PSK_TILE, half = threadIdx.x / PSK_TILE;
    const int col = n0 + s < n ? n0 + s : n - 1;
    const int last = C - 1 - c0 - half;          // the highest 2 * i of a valid row
#pragma unroll
    for (int i = 0; i < PSK_PER_LANE; i++)
    {
        const int row = c0 + half + (2 * i < last ? 2 * i : (last < 0 ? -half : last));
        r[i] = in[(size_t)row * stride + col];
    }
    vco = sine[psk_sine_index(acc + (uint32_t)s * PSK_DDS_STEP)];
}

__device__ __forceinline__ void psk_stage(float* tile, const float (&r)[PSK_PER_LANE], float vco)
{
    const int s = threadIdx.x % PSK_TILE, half = threadIdx.x / PSK_TILE;
#pragma unroll
    for (int i = 0; i < PSK_PER_LANE; i++) tile[(2 * i + half) * PSK_PITCH + s] = r[i];
    if (half == 0) tile[PSK_WG * PSK_PITCH + s] = vco;
}

__global__ __launch_bounds__(PSK_WG) void psk_decode(PskArena a, PskParams p, PskClock k, const float* __restrict__ in, int n, int stride)
{
    __shared__ float tiles[2][PSK_TILE_WORDS];
    __shared__ float ring[PSK_RING][PSK_WG];
    const int c0 = blockIdx.x * PSK_WG, c = c0 + threadIdx.x;
    const bool live = c < a.C;          // the other lanes of a partial last wave still help staging
    const size_t C = (size_t)a.C;
    const int slots = n < PSK_RING ? n : PSK_RING, slot0 = k.idx;
    PskChan ch;
    float old = 0;
    if (live)
    {
        ch.load(a, c);
        for (int j = 0; j < slots; j++)
        {
            const int slot = (slot0 + j) % PSK_RING;
            ring[slot][threadIdx.x] = a.fs[(PSK_F_RING + slot) * C + c];
        }
        old = ring[slot0][threadIdx.x];
    }
    float r[PSK_PER_LANE], vco;
    psk_fetch(r, vco, in, a.sine, k.acc, c0, a.C, 0, n, stride);
    psk_stage(tiles[0], r, vco);
    __syncthreads();
    for (int n0 = 0, t = 0; n0 < n; n0 += PSK_TILE, t ^= 1)
    {
        const bool more = n0 + PSK_TILE < n;
        // (k.acc is the accumulator at n0 here: the next tile starts PSK_TILE steps on)
        if (more) psk_fetch(r, vco, in, a.sine, k.acc + (uint32_t)PSK_TILE * PSK_DDS_STEP, c0, a.C, n0 + PSK_TILE, n, stride);
        const float* row = tiles[t] + threadIdx.x * PSK_PITCH;
        const float* osc = tiles[t] + PSK_WG * PSK_PITCH;
        const int m = n - n0 < PSK_TILE ? n - n0 : PSK_TILE;
        for (int s = 0; s < m; s++)
        {
            const PskTick tk = psk_tick(k, p.symbol_len);       // uniform
            if (live)
            {
                const float ahead = ring[k.idx][threadIdx.x];   // the next sample's slot, not tk.slot
                ring[tk.slot][threadIdx.x] = ch.mix(row[s], osc[s], old, p);
                if (tk.decide) ch.decide(a.chars);
                old = ahead;
            }
        }
        if (more) psk_stage(tiles[t ^ 1], r, vco);      // last read two tiles ago, before the previous barrier
        __syncthreads();
    }
    if (live)
    {
        ch.store(a, c);
        for (int j = 0; j < slots; j++)
        {
            const int slot = (slot0 + j) % PSK_RING;
            a.fs[(PSK_F_RING + slot) * C + c] = ring[slot][threadIdx.x];
        }
    }
}

struct uhsdr_psk_s : ArenaMem
{
    PskArena a;
    PskParams p;
    PskClock k;          // advanced on the host as the launches are enqueued
};

// the two tables, then the state
static size_t psk_layout(uhsdr_psk_s* h, char* base)
{
    PskArena& a = h->a;
    const size_t C = (size_t)a.C;
    ArenaCarver m{base, 0};
    a.sine = m.take<float>(1024);
    a.chars = m.take<uint8_t>(PSK_CODES);
    h->tables = m.off;
    a.fs = m.take<float>(PSK_F_COUNT * C);
    a.is = m.take<uint32_t>(PSK_I_COUNT * C);
    a.total = m.take<uint32_t>(C);
    a.text = m.take<uint8_t>(C * (size_t)a.text_capacity);
    return m.off;
}

// the oscillator's table as floats and the varicode lookup, as they lie at the head of the arena
static void psk_fill_tables(const uhsdr_psk_s* h, char* dst)
{
    float* sine = (float*)dst;
    for (int i = 0; i < 1024; i++) sine[i] = (float)uhsdr_dds_table[i];
    psk_fill_chars((uint8_t*)(dst + ((const char*)h->a.chars - (const char*)h->a.sine)));
}

// every static of the firmware's decoder starts at zero; the tables stay
extern "C" uhsdr_status uhsdr_psk_reset(uhsdr_psk_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = h->zero_state();
    if (st != UHSDR_OK) return st;
    h->k = PskClock{};
    return UHSDR_OK;
}

static uhsdr_status psk_create(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, bool host, void* stream, uhsdr_psk_handle* out)
{
    if (!out || num_channels < 1) { uhsdr_set_error("psk: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    if (speed_idx < 0 || speed_idx >= PSK_SPEED_COUNT) { uhsdr_set_error("psk: speed_idx %d not 0 .. 2", speed_idx); return UHSDR_ARGUMENT_ERROR; }
    if (text_capacity < 8) { uhsdr_set_error("psk: text_capacity %d below 8", text_capacity); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_psk_s* h = new (std::nothrow) uhsdr_psk_s();
    if (!h) return UHSDR_DEVICE_ERROR;
    h->a.C = num_channels;
    h->a.text_capacity = text_capacity;
    h->p = psk_params(speed_idx);
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = psk_layout(h, nullptr);
    uhsdr_status st = h->alloc("psk");
    if (st == UHSDR_OK)
    {
        psk_layout(h, (char*)h->mem);
        st = h->upload_tables("psk", [h](char* image) { psk_fill_tables(h, image); });
    }
    if (st == UHSDR_OK) st = uhsdr_psk_reset(h);
    if (st != UHSDR_OK) { uhsdr_psk_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_psk_create(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, void* stream, uhsdr_psk_handle* out)
{
    return psk_create(num_channels, speed_idx, text_capacity, false, stream, out);
}

extern "C" uhsdr_status uhsdr_psk_create_host(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, uhsdr_psk_handle* out)
{
    return psk_create(num_channels, speed_idx, text_capacity, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_psk_destroy(uhsdr_psk_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_psk_set_stream(uhsdr_psk_handle h, void* stream) { return arena_set_stream(h, "psk", stream, false); }

static uhsdr_status psk_check_run(uhsdr_psk_handle h, const float* samples, int32_t n, int32_t stride)
{
    if (!h || !samples) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    return arena_check_row("psk", "samples", n, n, stride);
}

static void psk_advance(uhsdr_psk_s* h, int32_t n)
{
    for (int32_t i = 0; i < n; i++) (void)psk_tick(h->k, h->p.symbol_len);
}

extern "C" uhsdr_status uhsdr_psk_process(uhsdr_psk_handle h, const float* samples, int32_t n, int32_t stride)
{
    const uhsdr_status st = psk_check_run(h, samples, n, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, false, "psk", "uhsdr_psk_process_host")) return UHSDR_ARGUMENT_ERROR;
    if (n == 0) return UHSDR_OK;
    const int grid = (h->a.C + PSK_WG - 1) / PSK_WG;
    hipLaunchKernelGGL(psk_decode, dim3(grid), dim3(PSK_WG), 0, h->stream, h->a, h->p, h->k, samples, n, stride);
    HIPCHK(hipGetLastError());
    psk_advance(h, n);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_psk_process_host(uhsdr_psk_handle h, const float* samples, int32_t n, int32_t stride)
{
    const uhsdr_status st = psk_check_run(h, samples, n, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, true, "psk", "uhsdr_psk_process")) return UHSDR_ARGUMENT_ERROR;
    for (int32_t c = 0; c < h->a.C; c++) psk_run_channel(h->a, c, h->p, h->k, samples + (size_t)c * stride, n);
    psk_advance(h, n);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_psk_outputs(uhsdr_psk_handle h, uint8_t** text, uint32_t** total, float** symbol)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    if (text) *text = h->a.text;
    if (total) *total = h->a.total;
    if (symbol) *symbol = h->a.fs + (size_t)PSK_F_SYMBOL * h->a.C;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_psk_synchronize(uhsdr_psk_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}
