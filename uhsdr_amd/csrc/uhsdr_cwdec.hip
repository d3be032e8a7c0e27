// CW decoder back end: batched Morse-to-text, channel == lane (uhsdr_cwdec.h has the step).
//
// cw_decode: a wave's 64 channels load their scalars from the field-major arena, each lane runs its
// own state machine over the launch's blocks and stores the scalars back.  The step is branchy and
// short; lanes diverge, so nothing is shared between them: no LDS, no barriers, and workgroups of one
// wave, which spreads C / 64 independent waves over the CUs and lets each retire on its own (131072
// channels are 2048 waves, two per SIMD).  The 256-entry state ring and the 40-entry data buffer stay
// in global memory as 32-bit elements [entry][C]: lanes that sit at the same ring position -- the
// common case, neighbouring channels keyed alike or idle -- touch one 256-byte line, and a lane that
// does not costs one dword access, where a [C][256] layout would cost a line per lane always.
#include <hip/hip_runtime.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_cwdec.h"

constexpr int CWDEC_WG = 64;

__global__ __launch_bounds__(CWDEC_WG) void cw_decode(CwDecArena a, const uint8_t* __restrict__ state, int blocks, int stride,
                                                      int offset, int step, int blocksize, int spikecancel)
{
    const int c = blockIdx.x * CWDEC_WG + threadIdx.x;
    if (c >= a.C) return;
    cwdec_run_channel(a, c, state + (size_t)c * stride, blocks, offset, step, blocksize, spikecancel);
}

struct uhsdr_cwdec_s : ArenaMem
{
    CwDecArena a;
    int blocksize, spikecancel;
};

static size_t cwdec_layout(CwDecArena& a, char* base)
{
    const size_t C = (size_t)a.C;
    ArenaCarver m{base, 0};
    a.ring = m.take<uint32_t>(CWDEC_SIG_SIZE * C);
    a.data = m.take<uint32_t>(CWDEC_DATA_SIZE * C);
    a.iscal = m.take<int32_t>(CWD_I_COUNT * C);
    a.fscal = m.take<float>(CWD_F_COUNT * C);
    a.total = m.take<uint32_t>(C);
    a.text = m.take<uint8_t>(C * (size_t)a.text_capacity);
    a.wpm = m.take<uint8_t>(C);
    return m.off;
}

// every static of the firmware's decoder starts at zero
extern "C" uhsdr_status uhsdr_cwdec_reset(uhsdr_cwdec_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    return h->zero_state();
}

static uhsdr_status cwdec_create(int32_t num_channels, int32_t blocksize, int32_t spikecancel, int32_t text_capacity, bool host, void* stream,
                                 uhsdr_cwdec_handle* out)
{
    if (!out || num_channels < 1) { uhsdr_set_error("cwdec: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    if (blocksize < 8 || blocksize > 128) { uhsdr_set_error("cwdec: blocksize %d not 8 .. 128", blocksize); return UHSDR_ARGUMENT_ERROR; }
    if (spikecancel < 0 || spikecancel > 2) { uhsdr_set_error("cwdec: spikecancel %d not 0 .. 2", spikecancel); return UHSDR_ARGUMENT_ERROR; }
    if (text_capacity < 8) { uhsdr_set_error("cwdec: text_capacity %d below 8", text_capacity); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_cwdec_s* h = new (std::nothrow) uhsdr_cwdec_s();
    if (!h) return UHSDR_DEVICE_ERROR;
    h->a.C = num_channels;
    h->a.text_capacity = text_capacity;
    h->blocksize = blocksize;
    h->spikecancel = spikecancel;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = cwdec_layout(h->a, nullptr);
    uhsdr_status st = h->alloc("cwdec");
    if (st == UHSDR_OK)
    {
        cwdec_layout(h->a, (char*)h->mem);
        st = h->zero_state();
    }
    if (st != UHSDR_OK) { uhsdr_cwdec_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwdec_create(int32_t num_channels, int32_t blocksize, int32_t spikecancel, int32_t text_capacity,
                                           void* stream, uhsdr_cwdec_handle* out)
{
    return cwdec_create(num_channels, blocksize, spikecancel, text_capacity, false, stream, out);
}

extern "C" uhsdr_status uhsdr_cwdec_create_host(int32_t num_channels, int32_t blocksize, int32_t spikecancel, int32_t text_capacity,
                                                uhsdr_cwdec_handle* out)
{
    return cwdec_create(num_channels, blocksize, spikecancel, text_capacity, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_cwdec_destroy(uhsdr_cwdec_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    delete h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwdec_set_stream(uhsdr_cwdec_handle h, void* stream) { return arena_set_stream(h, "cwdec", stream, false); }

static uhsdr_status cwdec_check_run(uhsdr_cwdec_handle h, const uint8_t* state, int32_t blocks, int64_t span, int32_t stride)
{
    if (!h || !state) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    return arena_check_row("cwdec", "blocks", blocks, span, stride);
}

// block b of a channel is state[c * stride + offset + b * step] (the RX chain's signal row holds one
// byte per call and a block completes every few calls; the public entry has offset 0, step 1)
uhsdr_status uhsdr_cwdec_launch(uhsdr_cwdec_handle h, const uint8_t* state, int32_t blocks, int32_t stride, int32_t offset, int32_t step)
{
    if (offset < 0 || step < 1) { uhsdr_set_error("cwdec: bad offset / step"); return UHSDR_ARGUMENT_ERROR; }
    const uhsdr_status st = cwdec_check_run(h, state, blocks, blocks ? (int64_t)offset + (int64_t)(blocks - 1) * step + 1 : 0, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, false, "cwdec", "uhsdr_cwdec_process_host")) return UHSDR_ARGUMENT_ERROR;
    if (blocks == 0) return UHSDR_OK;
    const int grid = (h->a.C + CWDEC_WG - 1) / CWDEC_WG;
    hipLaunchKernelGGL(cw_decode, dim3(grid), dim3(CWDEC_WG), 0, h->stream, h->a, state, blocks, stride, offset, step,
                       h->blocksize, h->spikecancel);
    HIPCHK(hipGetLastError());
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwdec_process(uhsdr_cwdec_handle h, const uint8_t* state, int32_t blocks, int32_t stride)
{
    return uhsdr_cwdec_launch(h, state, blocks, stride, 0, 1);
}

extern "C" uhsdr_status uhsdr_cwdec_process_host(uhsdr_cwdec_handle h, const uint8_t* state, int32_t blocks, int32_t stride)
{
    const uhsdr_status st = cwdec_check_run(h, state, blocks, blocks, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, true, "cwdec", "uhsdr_cwdec_process")) return UHSDR_ARGUMENT_ERROR;
    for (int32_t c = 0; c < h->a.C; c++)
        cwdec_run_channel(h->a, c, state + (size_t)c * stride, blocks, 0, 1, h->blocksize, h->spikecancel);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwdec_outputs(uhsdr_cwdec_handle h, uint8_t** text, uint32_t** total, uint8_t** wpm)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    if (text) *text = h->a.text;
    if (total) *total = h->a.total;
    if (wpm) *wpm = h->a.wpm;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_cwdec_synchronize(uhsdr_cwdec_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}

extern "C" int32_t uhsdr_cwdec_char_id(uint32_t code) { return cwdec_char_id(code); }
