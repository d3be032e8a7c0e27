// Waterfall image: the panel's RGB565 rows of the last drawing of a call, and the line ring behind it
// (uhsdr_wfall.h has the steps and the call's descriptor).
//
// wfall_image: one workgroup of four waves renders a run of 16-byte pieces of one channel's image.
// It first fills LDS: the 65 colours, and per image row the source line's offset (into this call's
// lines or into the ring, as the descriptor says) with the row's offset_pixel, one lane per row, so the
// binary32 divide runs height times per workgroup and not per pixel.  Then every lane takes whole
// 16-byte pieces of the image, eight pixels, counted from the first 16-byte boundary of the channel's
// image, so a wave's 64 pieces are 1 KiB of whole 128-byte lines whatever the width; the pixels
// before the first boundary and behind the last are stored one by one.  A piece inside one row whose
// eight source bytes all exist takes them in one 8-byte load at their byte offset (the ring and the
// lines stay in L2: a channel reads at most 20480 bytes for 2 * height * width written);
// any other piece (padding, a row's end, a marker) goes pixel by pixel through wfall_pixel.
//
// wfall_commit runs behind it on the stream: per ring line the last frame of the call that wrote it
// is copied into the ring with its frequency (last writer wins, from the descriptor: no walk over
// the frames), and `drawn` is written.  The image kernel has read the ring by then.
//
// The descriptor is a kernel argument; its tables are read with a lane's own index only where they
// lie in the kernarg segment (no copy, no scratch).
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_wfall.h"

constexpr int WFALL_THREADS = 256;
constexpr int WFALL_PIECE = 8;                  // pixels of a 16-byte piece

struct uhsdr_wfall_s : ArenaMem
{
    int32_t C;
    uhsdr_wfall_plan plan;              // the host's copy
    uhsdr_wfall_plan* d_plan;           // the tables of the allocation
    uint8_t* ring;                      // [C][wfall_size][width]
    uint32_t* freq;                     // [C][wfall_size]
    wfall_counters counters;            // the handle's, advanced at enqueue
};

struct WfallArgs
{
    const uhsdr_wfall_plan* plan;
    uint8_t* ring;
    uint32_t* freq;
    const uint8_t* lines;               // [C][F][W]
    const uint32_t* center_hz;          // [C][F] or null
    uint16_t* image;                    // [C][H][W] or null
    uint8_t* drawn;                     // [C][F] or null
    int C;
};

// a row's source line: bytes into the call's lines, or -1 - bytes into the ring (an offset, not a
// pointer: a pointer through LDS would come back as a flat one)
struct WfallRow
{
    int64_t at;
    int32_t offset_pixel;
};

__device__ __forceinline__ const uint8_t* wfall_row_ptr(const WfallArgs& a, const WfallRow& row)
{
    return row.at >= 0 ? a.lines + row.at : a.ring + (-1 - row.at);
}

// pixel (r, x) of the drawing
__device__ __forceinline__ uint16_t wfall_image_pixel(const WfallArgs& a, const int* mk, const uint16_t* colours, const WfallRow* rows, int W, int r,
                                                      int x)
{
    if (wfall_marked(mk, x)) return colours[WFALL_MARKER_ENTRY];
    return wfall_pixel(colours, wfall_row_ptr(a, rows[r]), W, rows[r].offset_pixel, x);
}

__global__ __launch_bounds__(WFALL_THREADS) void wfall_image(WfallArgs a, WfallCall call)
{
    __shared__ WfallRow rows[WFALL_MAX_HEIGHT + 1];
    __shared__ uint16_t colours[UHSDR_WFALL_COLOURS + 1];
    const uhsdr_wfall_plan* __restrict__ p = a.plan;
    const int W = p->width, H = p->height, S = p->wfall_size, F = call.frames;
    const int c = blockIdx.x, t = threadIdx.x;
    int mk[UHSDR_WFALL_MAX_MARKER];
    wfall_markers(p, mk);
    if (t < UHSDR_WFALL_COLOURS) colours[t] = p->colours[t];
    if (t < H)
    {
        const int32_t src = call.row_src[t];
        const uint32_t cur_hz = a.center_hz ? a.center_hz[(size_t)c * F + call.draw_frame] : 0u;
        uint32_t line_hz;
        int64_t at;
        if (src >= 0)
        {
            at = (int64_t)(((size_t)c * F + src) * W);
            line_hz = a.center_hz ? a.center_hz[(size_t)c * F + src] : 0u;
        }
        else
        {
            const int l = -1 - src;
            at = -1 - (int64_t)(((size_t)c * S + l) * W);
            line_hz = a.freq[(size_t)c * S + l];
        }
        rows[t].at = at;
        rows[t].offset_pixel = wfall_offset_pixel(p, line_hz, cur_hz);
    }
    __syncthreads();

    const int N = H * W;                                        // pixels of the channel's image
    uint16_t* __restrict__ img = a.image + (size_t)c * N;
    const int lead = (int)(((16 - ((uintptr_t)img & 15)) & 15) >> 1);   // pixels before the first 16-byte boundary
    const int head = lead < N ? lead : N;
    const int pieces = (N - head) / WFALL_PIECE;
    const int tail = head + pieces * WFALL_PIECE;               // the first pixel behind the last whole piece
    for (int k = blockIdx.y * WFALL_THREADS + t; k < pieces; k += gridDim.y * WFALL_THREADS)
    {
        const int p0 = head + k * WFALL_PIECE;
        int r = p0 / W, x = p0 - r * W;
        uint16_t px[WFALL_PIECE];
        const int s = x - rows[r].offset_pixel;
        bool plain = x + WFALL_PIECE <= W && s >= 0 && s + WFALL_PIECE <= W;
#pragma unroll
        for (int m = 0; m < UHSDR_WFALL_MAX_MARKER; m++) plain &= !(mk[m] >= x && mk[m] < x + WFALL_PIECE);
        if (plain)
        {
            uint64_t b;
            __builtin_memcpy(&b, wfall_row_ptr(a, rows[r]) + s, 8);          // one load at a byte offset
#pragma unroll
            for (int j = 0; j < WFALL_PIECE; j++) px[j] = wfall_colour(colours, (uint8_t)(b >> (8 * j)));
        }
        else
        {
#pragma unroll
            for (int j = 0; j < WFALL_PIECE; j++)
            {
                px[j] = wfall_image_pixel(a, mk, colours, rows, W, r, x);
                if (++x == W) { x = 0; r++; }
            }
        }
        uint4 v;
        v.x = px[0] | ((uint32_t)px[1] << 16);
        v.y = px[2] | ((uint32_t)px[3] << 16);
        v.z = px[4] | ((uint32_t)px[5] << 16);
        v.w = px[6] | ((uint32_t)px[7] << 16);
        *(uint4*)(img + p0) = v;
    }
    // the pixels in front of the first whole piece and behind the last: fewer than 16, block 0's
    if (blockIdx.y == 0 && t < 2 * WFALL_PIECE)
    {
        const int q = t < WFALL_PIECE ? t : tail + (t - WFALL_PIECE);
        if (t < WFALL_PIECE ? q < head : q < N)
        {
            const int r = q / W;
            img[q] = wfall_image_pixel(a, mk, colours, rows, W, r, q - r * W);
        }
    }
}

__global__ __launch_bounds__(WFALL_THREADS) void wfall_commit(WfallArgs a, WfallCall call)
{
    const uhsdr_wfall_plan* __restrict__ p = a.plan;
    const int W = p->width, S = p->wfall_size, F = call.frames;
    const int c = blockIdx.x, t = threadIdx.x;
    for (int l = 0; l < S; l++)
    {
        const int32_t f = call.last[l];                          // the same for every lane
        if (f < 0) continue;
        const uint8_t* __restrict__ src = a.lines + ((size_t)c * F + f) * W;
        uint8_t* __restrict__ dst = a.ring + ((size_t)c * S + l) * W;
        if ((((uintptr_t)src | (uintptr_t)dst) & 3) == 0)
        {
            for (int i = t; i < W / 4; i += WFALL_THREADS) ((uint32_t*)dst)[i] = ((const uint32_t*)src)[i];
            for (int i = (W & ~3) + t; i < W; i += WFALL_THREADS) dst[i] = src[i];
        }
        else
            for (int i = t; i < W; i += WFALL_THREADS) dst[i] = src[i];
        if (t == 0) a.freq[(size_t)c * S + l] = a.center_hz ? a.center_hz[(size_t)c * F + f] : 0u;
    }
    if (a.drawn)
        for (int f = t; f < F; f += WFALL_THREADS) a.drawn[(size_t)c * F + f] = (uint8_t)((call.update0 + 1 + f) % call.step == 0);
}

static size_t wfall_layout(uhsdr_wfall_s* h, char* base)
{
    ArenaCarver m{base, 0};
    h->d_plan = m.take<uhsdr_wfall_plan>(1);
    h->tables = m.off;
    h->ring = m.take<uint8_t>((size_t)h->C * h->plan.wfall_size * h->plan.width);
    h->freq = m.take<uint32_t>((size_t)h->C * h->plan.wfall_size);
    return m.off;
}

// the ring and its frequencies zero (UiSpectrum_WaterfallClearData), the three counters zero
extern "C" uhsdr_status uhsdr_wfall_reset(uhsdr_wfall_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = h->zero_state();
    if (st != UHSDR_OK) return st;
    h->counters = wfall_counters{};
    return h->synchronize();
}

static uhsdr_status wfall_create(int32_t num_channels, const uhsdr_wfall_config* cfg, bool host, void* stream, uhsdr_wfall_handle* out)
{
    if (!out || !cfg || num_channels < 1) { uhsdr_set_error("wfall: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_wfall_s* h = new (std::nothrow) uhsdr_wfall_s();
    if (!h) { uhsdr_set_error("wfall: host allocation of the handle failed"); return UHSDR_DEVICE_ERROR; }
    uhsdr_status st = uhsdr_wfall_plan_build(cfg, &h->plan);
    if (st != UHSDR_OK) { delete h; return st; }
    h->C = num_channels;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = wfall_layout(h, nullptr);
    st = h->alloc("wfall");
    if (st == UHSDR_OK)
    {
        wfall_layout(h, (char*)h->mem);
        st = h->upload_tables("wfall", [&](char* image) { memcpy(image, &h->plan, sizeof h->plan); });
    }
    if (st == UHSDR_OK) st = uhsdr_wfall_reset(h);
    if (st != UHSDR_OK) { uhsdr_wfall_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_wfall_create(int32_t num_channels, const uhsdr_wfall_config* cfg, void* stream, uhsdr_wfall_handle* out)
{
    return wfall_create(num_channels, cfg, false, stream, out);
}

extern "C" uhsdr_status uhsdr_wfall_create_host(int32_t num_channels, const uhsdr_wfall_config* cfg, uhsdr_wfall_handle* out)
{
    return wfall_create(num_channels, cfg, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_wfall_destroy(uhsdr_wfall_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

// the ring is the old stream's work: it drains before the next call reads the ring on another one
extern "C" uhsdr_status uhsdr_wfall_set_stream(uhsdr_wfall_handle h, void* stream) { return arena_set_stream(h, "wfall", stream, true); }

extern "C" uhsdr_status uhsdr_wfall_synchronize(uhsdr_wfall_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}

// what both entry points refuse; *io is the caller's or an empty one
static uhsdr_status wfall_check(uhsdr_wfall_handle h, const uint8_t* lines, int32_t frames, const uhsdr_wfall_io** io, bool host, const char* other)
{
    static const uhsdr_wfall_io none = {};
    if (!h || !lines) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0) { uhsdr_set_error("wfall: %d frames", frames); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, host, "wfall", other)) return UHSDR_ARGUMENT_ERROR;
    if (!*io) *io = &none;
    const uint16_t* image = (*io)->image;
    if ((uintptr_t)image & 1) { uhsdr_set_error("wfall: image must be 2-byte aligned"); return UHSDR_ARGUMENT_ERROR; }
    if (image)
    {
        const uintptr_t a0 = (uintptr_t)lines, a1 = a0 + (size_t)h->C * frames * h->plan.width;
        const uintptr_t b0 = (uintptr_t)image, b1 = b0 + sizeof(uint16_t) * (size_t)h->C * h->plan.height * h->plan.width;
        if (a0 < b1 && b0 < a1) { uhsdr_set_error("wfall: lines and image overlap"); return UHSDR_ARGUMENT_ERROR; }
    }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_wfall_process_lines(uhsdr_wfall_handle h, const uint8_t* lines, const uint32_t* center_hz, int32_t frames,
                                                  const uhsdr_wfall_io* io)
{
    const uhsdr_status st = wfall_check(h, lines, frames, &io, false, "uhsdr_wfall_process_lines_host");
    if (st != UHSDR_OK) return st;
    if (frames == 0) return UHSDR_OK;
    wfall_counters k = h->counters;
    WfallCall call;
    wfall_describe(&h->plan, &k, frames, &call);
    WfallArgs a = {};
    a.plan = h->d_plan;
    a.ring = h->ring;
    a.freq = h->freq;
    a.lines = lines;
    a.center_hz = center_hz;
    a.image = io->image;
    a.drawn = io->drawn;
    a.C = h->C;
    if (io->image && call.draw_frame >= 0)
    {
        // enough workgroups per channel to fill the device at small batches, one at large ones
        const int pieces = h->plan.height * h->plan.width / WFALL_PIECE;
        int split = (2048 + h->C - 1) / h->C;
        const int most = (pieces + WFALL_THREADS - 1) / WFALL_THREADS;
        if (split > most) split = most;
        if (split < 1) split = 1;
        hipLaunchKernelGGL(wfall_image, dim3(h->C, split), dim3(WFALL_THREADS), 0, h->stream, a, call);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(wfall_commit, dim3(h->C), dim3(WFALL_THREADS), 0, h->stream, a, call);
    HIPCHK(hipGetLastError());
    h->counters = k;
    return UHSDR_OK;
}

// Every channel on the CPU, frame after frame (wfall_channel_host): no descriptor
extern "C" uhsdr_status uhsdr_wfall_process_lines_host(uhsdr_wfall_handle h, const uint8_t* lines, const uint32_t* center_hz, int32_t frames,
                                                       const uhsdr_wfall_io* io)
{
    const uhsdr_status st = wfall_check(h, lines, frames, &io, true, "uhsdr_wfall_process_lines");
    if (st != UHSDR_OK) return st;
    const uhsdr_wfall_plan* p = &h->plan;
    const size_t W = p->width, S = p->wfall_size, F = frames;
    for (size_t c = 0; c < (size_t)h->C; c++)
        wfall_channel_host(p, h->counters, h->ring + c * S * W, h->freq + c * S, lines + c * F * W, center_hz ? center_hz + c * F : nullptr, frames,
                           io->image ? io->image + c * p->height * W : nullptr, io->drawn ? io->drawn + c * F : nullptr);
    int draws;
    uint32_t lptr;
    for (int32_t f = 0; f < frames; f++) wfall_advance(p, &h->counters, &draws, &lptr);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_wfall_state(uhsdr_wfall_handle h, uint32_t* wfall_line, uint32_t* double_line_start, uint32_t* wfall_line_update)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = h->synchronize();
    if (st != UHSDR_OK) return st;
    if (wfall_line) *wfall_line = h->counters.line;
    if (double_line_start) *double_line_start = h->counters.dls;
    if (wfall_line_update) *wfall_line_update = h->counters.update;
    return UHSDR_OK;
}
