// Display stage: batched display frames, a wave per channel (uhsdr_display.h has the frame's steps).
//
// display_frames: a workgroup of four waves runs four channels, each wave its channel's frames in
// order with the channel's display_offset in a register from the first frame to the last.  A frame's
// row of L = 256 or 512 floats of sd.FFT_AVGData comes in as one 16-byte load per lane (two at 512),
// whole lines, into the wave's own L floats of LDS; the scaled row takes L more; no workgroup
// barrier.  Then display_wave_frame: the logarithm and the offset per bin, four or eight bins a lane,
// the minimum as a wave reduction, the offset's update, and per output column one lane for the width
// reduction (at most four samples of the scaled row), the height and the palette index, stored as
// consecutive uint16_t / uint8_t.  The next frame's loads are issued before this frame's arithmetic
// and land in registers, so the row in LDS is rewritten only after its readers.
//
// The shape is that of meter_frames and of the spectrum kernel, whose epilogue runs the same
// display_wave_frame on the average it has staged in LDS (uhsdr_spectrum.hip); DESIGN.md 4 and 5 have
// the count.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_dsp.h"
#include "uhsdr_display.h"
#include "uhsdr_display_host.h"

constexpr int DISPLAY_WAVES = 4;

template <int L>
__global__ __launch_bounds__(64 * DISPLAY_WAVES) void display_frames(DisplayArgs a, const float* __restrict__ avg,
                                                                     const float* __restrict__ edge)
{
    extern __shared__ __attribute__((aligned(16))) float display_rows[];     // [DISPLAY_WAVES][2][L]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * DISPLAY_WAVES + w;
    if (c >= a.C) return;                        // whole wave; no workgroup barrier below
    constexpr int Q = L / 256;                   // 16-byte pieces per lane
    float* in = display_rows + w * 2 * L;
    float* row = in + L;
    const float* __restrict__ src = avg + (size_t)c * a.F * L;
    const float* __restrict__ eg = edge ? edge + (size_t)c * a.F : nullptr;
    float offset = a.state[c], min1 = a.state[a.C + c];
    float next[4 * Q];                           // floats, not float4: an array of those stays in memory
    auto fetch = [&](int f) {
#pragma unroll
        for (int q = 0; q < Q; q++)
        {
            const float4 v = *(const float4*)(src + (size_t)f * L + 4 * (lane + 64 * q));
            next[4 * q] = v.x; next[4 * q + 1] = v.y; next[4 * q + 2] = v.z; next[4 * q + 3] = v.w;
        }
    };
    fetch(0);
    for (int f = 0; f < a.F; f++)
    {
#pragma unroll
        for (int q = 0; q < Q; q++) *(float4*)(in + 4 * (lane + 64 * q)) = make_float4(next[4 * q], next[4 * q + 1], next[4 * q + 2], next[4 * q + 3]);
        const float e = eg ? eg[f] : 0.0f;
        fetch(f + 1 < a.F ? f + 1 : f);          // the last frame again instead of a read past the rows
        wave_sync();
        min1 = display_wave_frame(a.plan, offset, in, row, e, (size_t)c * a.F + f, a.io, lane);
        wave_sync();                             // the rows' readers are done before the next frame lands
    }
    if (lane == 0) { a.state[c] = offset; a.state[a.C + c] = min1; }
}

static size_t display_layout(uhsdr_display_s* h, char* base)
{
    ArenaCarver m{base, 0};
    h->d_plan = m.take<uhsdr_display_plan>(1);
    h->tables = m.off;
    h->state = m.take<float>((size_t)DISPLAY_STATE_WORDS * h->C);
    return m.off;
}

// display_offset -80 (INIT_SPEC_AGC_LEVEL), the last min 0
extern "C" uhsdr_status uhsdr_display_reset(uhsdr_display_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = h->zero_state();
    if (st != UHSDR_OK) return st;
    const size_t C = (size_t)h->C;
    if (h->host) { for (size_t c = 0; c < C; c++) h->state[c] = DISPLAY_OFFSET_INIT; return UHSDR_OK; }
    float* image = (float*)malloc(sizeof(float) * C);
    if (!image) { uhsdr_set_error("display: host allocation failed"); return UHSDR_DEVICE_ERROR; }
    for (size_t c = 0; c < C; c++) image[c] = DISPLAY_OFFSET_INIT;
    hipError_t e = hipMemcpyAsync(h->state, image, sizeof(float) * C, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(image);
    HIPCHK(e);
    return UHSDR_OK;
}

static uhsdr_status display_create(int32_t num_channels, const uhsdr_display_config* cfg, bool host, void* stream, uhsdr_display_handle* out)
{
    if (!out || !cfg || num_channels < 1) { uhsdr_set_error("display: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_display_s* h = new (std::nothrow) uhsdr_display_s();
    if (!h) { uhsdr_set_error("display: host allocation of the handle failed"); return UHSDR_DEVICE_ERROR; }
    uhsdr_status st = uhsdr_display_plan_build(cfg, &h->plan);
    if (st != UHSDR_OK) { delete h; return st; }
    h->C = num_channels;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = display_layout(h, nullptr);
    st = h->alloc("display");
    if (st == UHSDR_OK)
    {
        display_layout(h, (char*)h->mem);
        st = h->upload_tables("display", [&](char* image) { memcpy(image, &h->plan, sizeof h->plan); });
    }
    if (st == UHSDR_OK) st = uhsdr_display_reset(h);
    if (st != UHSDR_OK) { uhsdr_display_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_display_create(int32_t num_channels, const uhsdr_display_config* cfg, void* stream, uhsdr_display_handle* out)
{
    return display_create(num_channels, cfg, false, stream, out);
}

extern "C" uhsdr_status uhsdr_display_create_host(int32_t num_channels, const uhsdr_display_config* cfg, uhsdr_display_handle* out)
{
    return display_create(num_channels, cfg, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_display_destroy(uhsdr_display_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

// the state is read back by uhsdr_display_state, so the old stream drains first
extern "C" uhsdr_status uhsdr_display_set_stream(uhsdr_display_handle h, void* stream) { return arena_set_stream(h, "display", stream, true); }

extern "C" uhsdr_status uhsdr_display_synchronize(uhsdr_display_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}

extern "C" uhsdr_status uhsdr_display_process_avg(uhsdr_display_handle h, const float* avg, const float* edge, int32_t frames,
                                                  const uhsdr_display_io* io)
{
    if (!h || !avg) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0) { uhsdr_set_error("display: %d frames", frames); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, false, "display", "uhsdr_display_process_avg_host")) return UHSDR_ARGUMENT_ERROR;
    if ((uintptr_t)avg & 15) { uhsdr_set_error("display: avg must be 16-byte aligned"); return UHSDR_ARGUMENT_ERROR; }
    if (frames == 0) return UHSDR_OK;
    const DisplayArgs a = display_args(h, io, frames);
    if (!h->plan.reads_edge) edge = nullptr;
    const dim3 grid((h->C + DISPLAY_WAVES - 1) / DISPLAY_WAVES), block(64 * DISPLAY_WAVES);
    const size_t lds = sizeof(float) * DISPLAY_WAVES * 2 * (size_t)h->plan.fft_len;
    if (h->plan.fft_len == 256) hipLaunchKernelGGL(display_frames<256>, grid, block, lds, h->stream, a, avg, edge);
    else hipLaunchKernelGGL(display_frames<512>, grid, block, lds, h->stream, a, avg, edge);
    HIPCHK(hipGetLastError());
    return UHSDR_OK;
}

// Every channel on the CPU: the same steps, the frame by one thread (display_frame)
extern "C" uhsdr_status uhsdr_display_process_avg_host(uhsdr_display_handle h, const float* avg, const float* edge, int32_t frames,
                                                       const uhsdr_display_io* io)
{
    if (!h || !avg) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0) { uhsdr_set_error("display: %d frames", frames); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, true, "display", "uhsdr_display_process_avg")) return UHSDR_ARGUMENT_ERROR;
    const uhsdr_display_io none = {};
    if (!io) io = &none;
    if (!h->plan.reads_edge) edge = nullptr;
    const int L = h->plan.fft_len, W = h->plan.width;
    const size_t C = (size_t)h->C;
    float row[UHSDR_DISPLAY_MAX_WIDTH];
    for (size_t c = 0; c < C; c++)
    {
        float offset = h->state[c], min1 = h->state[C + c];
        for (int32_t f = 0; f < frames; f++)
        {
            const size_t at = c * frames + f;
            min1 = display_frame(&h->plan, &offset, avg + at * L, edge ? edge[at] : 0.0f, row, io->scope ? io->scope + at * W : nullptr,
                                 io->wfall ? io->wfall + at * W : nullptr);
            if (io->offset) io->offset[at] = offset;
            if (io->min) io->min[at] = min1;
        }
        h->state[c] = offset;
        h->state[C + c] = min1;
    }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_display_state(uhsdr_display_handle h, float* offset, float* min)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const size_t C = (size_t)h->C;
    float* const dst[2] = { offset, min };
    if (!h->host) HIPCHK(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 2; k++)
    {
        if (!dst[k]) continue;
        const float* src = h->state + k * C;
        if (h->host) memcpy(dst[k], src, sizeof(float) * C);
        else HIPCHK(hipMemcpy(dst[k], src, sizeof(float) * C, hipMemcpyDeviceToHost));
    }
    return UHSDR_OK;
}
