// Signal meter: batched display frames, a wave per channel (uhsdr_meter.h has the frame's steps).
//
// meter_frames: a workgroup of four waves runs four channels, each wave its channel's frames in
// order with the channel's state (eleven words) in registers from the first frame to the last.  A
// frame's row of L = 256 or 512 floats comes in as one 16-byte load per lane (two at 512), whole
// lines, into the wave's own L floats of LDS; no workgroup barrier.  Then meter_wave_frame: the SNAP
// search as a wave reduction, the passband's sum as the serial loop the reference has (its order is
// mandatory), the logarithm, the averagers and the S-unit search, all lanes alike; lane 0 writes the
// frame's outputs.  The next frame's loads are issued before this frame's arithmetic and land in
// registers, so the row in LDS is rewritten only after its readers.
//
// The shape is that of the spectrum kernel, whose epilogue runs the same meter_wave_frame on the
// magnitudes it has staged in LDS (uhsdr_spectrum.hip); DESIGN.md 4 and 5 have the reason and the count.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_dsp.h"
#include "uhsdr_meter.h"
#include "uhsdr_meter_host.h"

constexpr int METER_WAVES = 4;

template <int L>
__global__ __launch_bounds__(64 * METER_WAVES) void meter_frames(MeterArgs a, const float* __restrict__ mag)
{
    extern __shared__ __attribute__((aligned(16))) float meter_rows[];       // [METER_WAVES][L]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * METER_WAVES + w;
    if (c >= a.C) return;                        // whole wave; no workgroup barrier below
    constexpr int Q = L / 256;                   // 16-byte pieces per lane
    float* row = meter_rows + w * L;
    const float* __restrict__ src = mag + (size_t)c * a.F * L;
    const uint8_t* __restrict__ cw = a.io.cw_signal ? a.io.cw_signal + (size_t)c * a.F : nullptr;
    meter_state s;
    meter_state_load(s, a.state, a.C, c);
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
        for (int q = 0; q < Q; q++) *(float4*)(row + 4 * (lane + 64 * q)) = make_float4(next[4 * q], next[4 * q + 1], next[4 * q + 2], next[4 * q + 3]);
        const int key = cw ? cw[f] : 0;
        fetch(f + 1 < a.F ? f + 1 : f);          // the last frame again instead of a read past the rows
        wave_sync();
        meter_wave_frame(a.plan, s, row, key, lane);
        if (lane == 0) meter_write(a.io, s, (size_t)c * a.F + f);
        wave_sync();                             // the row's readers are done before the next frame lands
    }
    if (lane == 0) meter_state_store(s, a.state, a.C, c);
}

static size_t meter_layout(uhsdr_meter_s* h, char* base)
{
    ArenaCarver m{base, 0};
    h->d_plan = m.take<uhsdr_meter_plan>(1);
    h->tables = m.off;
    h->state = m.take<uint32_t>((size_t)METER_STATE_WORDS * h->C);
    return m.off;
}

// averages and outputs 0, freq_old 1e7 (the firmware's static initialisers)
extern "C" uhsdr_status uhsdr_meter_reset(uhsdr_meter_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = h->zero_state();
    if (st != UHSDR_OK) return st;
    const size_t C = (size_t)h->C;
    uint32_t* freq_old = h->state + 4 * C;       // meter_state's fifth word
    const float init = METER_FREQ_OLD_INIT;
    uint32_t bits;
    memcpy(&bits, &init, 4);
    if (h->host) { for (size_t c = 0; c < C; c++) freq_old[c] = bits; return UHSDR_OK; }
    uint32_t* image = (uint32_t*)malloc(sizeof(uint32_t) * C);
    if (!image) { uhsdr_set_error("meter: host allocation failed"); return UHSDR_DEVICE_ERROR; }
    for (size_t c = 0; c < C; c++) image[c] = bits;
    hipError_t e = hipMemcpyAsync(freq_old, image, sizeof(uint32_t) * C, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    free(image);
    HIPCHK(e);
    return UHSDR_OK;
}

static uhsdr_status meter_create(int32_t num_channels, const uhsdr_meter_config* cfg, bool host, void* stream, uhsdr_meter_handle* out)
{
    if (!out || !cfg || num_channels < 1) { uhsdr_set_error("meter: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_meter_plan plan;
    uhsdr_status st = uhsdr_meter_plan_build(cfg, &plan);
    if (st != UHSDR_OK) return st;
    uhsdr_meter_s* h = new (std::nothrow) uhsdr_meter_s();
    if (!h) { uhsdr_set_error("meter: host allocation of the handle failed"); return UHSDR_DEVICE_ERROR; }
    h->C = num_channels;
    h->plan = plan;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = meter_layout(h, nullptr);
    st = h->alloc("meter");
    if (st == UHSDR_OK)
    {
        meter_layout(h, (char*)h->mem);
        st = h->upload_tables("meter", [&](char* image) { memcpy(image, &h->plan, sizeof h->plan); });
    }
    if (st == UHSDR_OK) st = uhsdr_meter_reset(h);
    if (st != UHSDR_OK) { uhsdr_meter_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_meter_create(int32_t num_channels, const uhsdr_meter_config* cfg, void* stream, uhsdr_meter_handle* out)
{
    return meter_create(num_channels, cfg, false, stream, out);
}

extern "C" uhsdr_status uhsdr_meter_create_host(int32_t num_channels, const uhsdr_meter_config* cfg, uhsdr_meter_handle* out)
{
    return meter_create(num_channels, cfg, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_meter_destroy(uhsdr_meter_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

// the state is read back by uhsdr_meter_state, so the old stream drains first
extern "C" uhsdr_status uhsdr_meter_set_stream(uhsdr_meter_handle h, void* stream) { return arena_set_stream(h, "meter", stream, true); }

extern "C" uhsdr_status uhsdr_meter_synchronize(uhsdr_meter_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}

extern "C" uhsdr_status uhsdr_meter_process_mag(uhsdr_meter_handle h, const float* mag, int32_t frames, const uhsdr_meter_io* io)
{
    if (!h || !mag) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0) { uhsdr_set_error("meter: %d frames", frames); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, false, "meter", "uhsdr_meter_process_mag_host")) return UHSDR_ARGUMENT_ERROR;
    if ((uintptr_t)mag & 15) { uhsdr_set_error("meter: mag must be 16-byte aligned"); return UHSDR_ARGUMENT_ERROR; }
    if (frames == 0) return UHSDR_OK;
    const MeterArgs a = meter_args(h, io, frames);
    const dim3 grid((h->C + METER_WAVES - 1) / METER_WAVES), block(64 * METER_WAVES);
    const size_t lds = sizeof(float) * METER_WAVES * (size_t)h->plan.fft_len;
    if (h->plan.fft_len == 256) hipLaunchKernelGGL(meter_frames<256>, grid, block, lds, h->stream, a, mag);
    else hipLaunchKernelGGL(meter_frames<512>, grid, block, lds, h->stream, a, mag);
    HIPCHK(hipGetLastError());
    return UHSDR_OK;
}

// Every channel on the CPU: the same steps, the frame by one thread (meter_frame)
extern "C" uhsdr_status uhsdr_meter_process_mag_host(uhsdr_meter_handle h, const float* mag, int32_t frames, const uhsdr_meter_io* io)
{
    if (!h || !mag) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0) { uhsdr_set_error("meter: %d frames", frames); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, true, "meter", "uhsdr_meter_process_mag")) return UHSDR_ARGUMENT_ERROR;
    const uhsdr_meter_io none = {};
    if (!io) io = &none;
    const int L = h->plan.fft_len;
    const size_t C = (size_t)h->C;
    for (size_t c = 0; c < C; c++)
    {
        meter_state s;
        uint32_t w[METER_STATE_WORDS];
        for (int k = 0; k < METER_STATE_WORDS; k++) w[k] = h->state[k * C + c];
        memcpy(&s, w, sizeof s);
        for (int32_t f = 0; f < frames; f++)
        {
            const size_t at = c * frames + f;
            meter_frame(&h->plan, &s, mag + at * L, io->cw_signal ? io->cw_signal[at] : 0);
            if (io->dbm_cur) io->dbm_cur[at] = s.dbm_cur;
            if (io->dbmhz_cur) io->dbmhz_cur[at] = s.dbmhz_cur;
            if (io->dbm) io->dbm[at] = s.dbm;
            if (io->dbmhz) io->dbmhz[at] = s.dbmhz;
            if (io->s_count) io->s_count[at] = s.s_count;
            if (io->snap_carrier_freq) io->snap_carrier_freq[at] = s.snap;
        }
        memcpy(w, &s, sizeof s);
        for (int k = 0; k < METER_STATE_WORDS; k++) h->state[k * C + c] = w[k];
    }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_meter_state(uhsdr_meter_handle h, float* dbm_cur, float* dbmhz_cur, float* dbm, float* dbmhz, int32_t* s_count,
                                          uint32_t* snap_carrier_freq)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const size_t C = (size_t)h->C;
    void* const dst[6] = { dbm_cur, dbmhz_cur, dbm, dbmhz, s_count, snap_carrier_freq };
    if (!h->host) HIPCHK(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 6; k++)
    {
        if (!dst[k]) continue;
        const uint32_t* src = h->state + (5 + k) * C;        // the outputs follow meter_state's five words of history
        if (h->host) memcpy(dst[k], src, sizeof(uint32_t) * C);
        else HIPCHK(hipMemcpy(dst[k], src, sizeof(uint32_t) * C, hipMemcpyDeviceToHost));
    }
    return UHSDR_OK;
}
