// Noise blanker: batched frames, channel == lane (uhsdr_nb.h has the frame's steps).
//
// nb_frames: a one-wave workgroup runs 64 channels.  Every sum of the frame has a fixed order, so a
// channel's frame is one lane's serial work and the parallelism is across channels.  The working
// buffers (154 floats) and the filtered frames (128 floats) of the 64 channels lie in LDS as
// [sample][lane] with a pitch of 65 words: 73320 bytes, dynamic LDS, two workgroups per CU.  A lane
// walks its own column, word 65 s + lane: the same s in all lanes is 64 consecutive words, no bank
// conflict.  The rows of in and out are [C][stride]; a wave loads and stores them row by row, 64
// consecutive floats per instruction, and writes sample s of row r to word 65 s + r: s runs with
// the lane, so a half wave lands on 32 different banks again.  That is the transpose; without the
// odd pitch its writes would put a half wave on one bank.
//
// Per frame and lane: 11 autocorrelation sums (1353 multiply-adds, 8 samples of all lags per pass
// over 18 loaded samples), the Levinson recursion (about 100), the two 11-tap filters fused (2816,
// eight outputs at a time with the ten samples before them in registers, pass 1's result never
// stored), the variance (256), the search (115 LDS reads and compares) and at most five repairs of
// 140 multiply-adds each.  The search and the repairs diverge: a wave runs the search until its
// last lane has stopped and as many repairs as its busiest lane, with the lanes' addresses apart.
// The state (the last 26 floats of the working buffer, field-major [26][C], and the two counters)
// is loaded once per launch and stored once.
//
// Lanes past the last channel stay in the loop for the barriers and the row transfers (which run
// over the rows that exist) and skip the frame's arithmetic.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_nb.h"

constexpr int NB_WG = 64;
constexpr int NB_PITCH = NB_WG + 1;
constexpr size_t NB_LDS_BYTES = sizeof(float) * (NB_WB + NB_FRAME) * NB_PITCH;

struct NbArena
{
    int32_t C;
    float* keep;                        // [NB_KEEP][C]: the working buffer's last 26 floats
    int32_t* last;                      // [C]: places repaired in the last frame
    uint32_t* total;                    // [C]: places repaired since the reset
};

__global__ __launch_bounds__(NB_WG) void nb_frames(NbArena a, int nb_setting, const float* in, float* out, int frames, int stride)
{
    extern __shared__ __attribute__((aligned(16))) float nb_lds[];
    float* const WB = nb_lds;
    float* const TS = nb_lds + NB_WB * NB_PITCH;
    const int lane = threadIdx.x, c0 = blockIdx.x * NB_WG, c = c0 + lane;
    const bool live = c < a.C;
    const int rows = a.C - c0 < NB_WG ? a.C - c0 : NB_WG;
    float* const wb = WB + lane;
    float* const ts = TS + lane;
    int32_t last = 0;
    uint32_t total = 0;
    if (live)
    {
        for (int k = 0; k < NB_KEEP; k++) wb[k * NB_PITCH] = a.keep[(size_t)k * a.C + c];
        last = a.last[c];
        total = a.total[c];
    }
    for (int f = 0; f < frames; f++)
    {
        {
            const float* src = in + (size_t)c0 * stride + (size_t)f * NB_FRAME + lane;    // c0 + r < C, 128 f + 64 + lane < 128 frames <= stride
            float* dst = WB + (NB_KEEP + lane) * NB_PITCH;
#pragma unroll 8
            for (int r = 0; r < rows; r++)
            {
                dst[r] = src[(size_t)r * stride];
                dst[64 * NB_PITCH + r] = src[(size_t)r * stride + 64];
            }
        }
        __syncthreads();
        if (live)
        {
            last = nb_frame(wb, NB_PITCH, ts, NB_PITCH, nb_setting);
            total += (uint32_t)last;
        }
        __syncthreads();
        {
            float* dst = out + (size_t)c0 * stride + (size_t)f * NB_FRAME + lane;
            const float* src = WB + (NB_LEAD + lane) * NB_PITCH;
#pragma unroll 8
            for (int r = 0; r < rows; r++)
            {
                dst[(size_t)r * stride] = src[r];
                dst[(size_t)r * stride + 64] = src[64 * NB_PITCH + r];
            }
        }
        __syncthreads();
        if (live)
            for (int k = 0; k < NB_KEEP; k++) wb[k * NB_PITCH] = wb[(NB_FRAME + k) * NB_PITCH];
        __syncthreads();                // the next frame's rows land on what was just read
    }
    if (live)
    {
        for (int k = 0; k < NB_KEEP; k++) a.keep[(size_t)k * a.C + c] = wb[k * NB_PITCH];
        a.last[c] = last;
        a.total[c] = total;
    }
}

struct uhsdr_nb_s : ArenaMem
{
    NbArena a;
    uhsdr_nb_config cfg;
};

static size_t nb_layout(NbArena& a, char* base)
{
    const size_t C = (size_t)a.C;
    ArenaCarver m{base, 0};
    a.keep = m.take<float>(NB_KEEP * C);
    a.last = m.take<int32_t>(C);
    a.total = m.take<uint32_t>(C);
    return m.off;
}

extern "C" void uhsdr_nb_config_default(uhsdr_nb_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->nb_setting = 8;
}

// the firmware's working_buffer is never cleared; here a fresh blanker starts from silence
extern "C" uhsdr_status uhsdr_nb_reset(uhsdr_nb_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    return h->zero_state();
}

static uhsdr_status nb_create(int32_t num_channels, const uhsdr_nb_config* cfg, bool host, void* stream, uhsdr_nb_handle* out)
{
    if (!out || !cfg || num_channels < 1) { uhsdr_set_error("nb: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->nb_setting < 1 || cfg->nb_setting > NB_MAX_SETTING)
    { uhsdr_set_error("nb: nb_setting %d outside 1..15", cfg->nb_setting); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_nb_s* h = new (std::nothrow) uhsdr_nb_s();
    if (!h) { uhsdr_set_error("nb: host allocation of the handle failed"); return UHSDR_DEVICE_ERROR; }
    h->a.C = num_channels;
    h->cfg = *cfg;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->tables = 0;
    h->bytes = nb_layout(h->a, nullptr);
    uhsdr_status st = h->alloc("nb");
    if (st == UHSDR_OK)
    {
        nb_layout(h->a, (char*)h->mem);
        st = h->zero_state();
    }
    if (st == UHSDR_OK && !host)
    {
        // more than the 64 KiB a kernel gets without asking
        const hipError_t e = hipFuncSetAttribute((const void*)nb_frames, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NB_LDS_BYTES);
        if (e != hipSuccess) { uhsdr_set_error("nb: %zu bytes of LDS refused: %s", NB_LDS_BYTES, hipGetErrorString(e)); st = UHSDR_DEVICE_ERROR; }
    }
    if (st != UHSDR_OK) { uhsdr_nb_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nb_create(int32_t num_channels, const uhsdr_nb_config* cfg, void* stream, uhsdr_nb_handle* out)
{
    return nb_create(num_channels, cfg, false, stream, out);
}

extern "C" uhsdr_status uhsdr_nb_create_host(int32_t num_channels, const uhsdr_nb_config* cfg, uhsdr_nb_handle* out)
{
    return nb_create(num_channels, cfg, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_nb_destroy(uhsdr_nb_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nb_set_stream(uhsdr_nb_handle h, void* stream) { return arena_set_stream(h, "nb", stream, false); }

extern "C" uhsdr_status uhsdr_nb_synchronize(uhsdr_nb_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}

static uhsdr_status nb_check_run(uhsdr_nb_handle h, const float* in, float* out, int32_t frames, int32_t stride)
{
    if (!h || !in || !out) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0 || stride < 0 || (int64_t)frames * NB_FRAME > stride)
    { uhsdr_set_error("nb: %d frames of %d samples do not fit a row of %d", frames, NB_FRAME, stride); return UHSDR_LENGTH_ERROR; }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nb_process_frames(uhsdr_nb_handle h, const float* in, float* out, int32_t frames, int32_t stride)
{
    const uhsdr_status st = nb_check_run(h, in, out, frames, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, false, "nb", "uhsdr_nb_process_frames_host")) return UHSDR_ARGUMENT_ERROR;
    if (frames == 0) return UHSDR_OK;
    const int grid = (h->a.C + NB_WG - 1) / NB_WG;
    hipLaunchKernelGGL(nb_frames, dim3(grid), dim3(NB_WG), NB_LDS_BYTES, h->stream, h->a, h->cfg.nb_setting, in, out, frames, stride);
    HIPCHK(hipGetLastError());
    return UHSDR_OK;
}

// One channel on the CPU: the same frame function over a plain working buffer
extern "C" uhsdr_status uhsdr_nb_process_frames_host(uhsdr_nb_handle h, const float* in, float* out, int32_t frames, int32_t stride)
{
    const uhsdr_status st = nb_check_run(h, in, out, frames, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, true, "nb", "uhsdr_nb_process_frames")) return UHSDR_ARGUMENT_ERROR;
    if (frames == 0) return UHSDR_OK;
    const NbArena& a = h->a;
    for (int32_t c = 0; c < a.C; c++)
    {
        float wb[NB_WB], ts[NB_FRAME];
        for (int k = 0; k < NB_KEEP; k++) wb[k] = a.keep[(size_t)k * a.C + c];
        for (int32_t f = 0; f < frames; f++)
        {
            memcpy(wb + NB_KEEP, in + (size_t)c * stride + (size_t)f * NB_FRAME, sizeof(float) * NB_FRAME);
            a.last[c] = nb_frame(wb, 1, ts, 1, h->cfg.nb_setting);
            a.total[c] += (uint32_t)a.last[c];
            memcpy(out + (size_t)c * stride + (size_t)f * NB_FRAME, wb + NB_LEAD, sizeof(float) * NB_FRAME);
            memmove(wb, wb + NB_FRAME, sizeof(float) * NB_KEEP);
        }
        for (int k = 0; k < NB_KEEP; k++) a.keep[(size_t)k * a.C + c] = wb[k];
    }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nb_state(uhsdr_nb_handle h, int32_t* last_count, uint32_t* total_count)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const size_t C = (size_t)h->a.C;
    if (h->host)
    {
        if (last_count) memcpy(last_count, h->a.last, sizeof(int32_t) * C);
        if (total_count) memcpy(total_count, h->a.total, sizeof(uint32_t) * C);
        return UHSDR_OK;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (last_count) HIPCHK(hipMemcpy(last_count, h->a.last, sizeof(int32_t) * C, hipMemcpyDeviceToHost));
    if (total_count) HIPCHK(hipMemcpy(total_count, h->a.total, sizeof(uint32_t) * C, hipMemcpyDeviceToHost));
    return UHSDR_OK;
}
