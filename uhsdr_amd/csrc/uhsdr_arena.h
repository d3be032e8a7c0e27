/*
 * The memory behind a per-channel module's handle: one allocation, host or device, with the
 * module's tables at its head and the per-channel state after them.  Host code only: no kernel and
 * no device symbol lives here, so including it changes no device code object.
 *
 * What the modules share is here: carving the allocation, allocating and releasing it, uploading
 * the tables, zeroing the state, waiting for the stream, and the refusals every entry point starts
 * with.  What a reset means beyond zeroing, and whether set_stream drains the old stream, stays
 * with each module.
 */
#ifndef UHSDR_ARENA_H
#define UHSDR_ARENA_H

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "uhsdr_internal.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { uhsdr_set_error("%s: %s", #x, hipGetErrorString(e_)); return UHSDR_DEVICE_ERROR; } } while (0)

// Hands out consecutive 256-byte granules of one allocation.  A null base sizes only: every take
// returns null and `off` ends at the bytes needed.
struct ArenaCarver
{
    char* base;
    size_t off;
    template <class T> T* take(size_t count)
    {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (sizeof(T) * count + 255) & ~(size_t)255;
        return p;
    }
};

struct ArenaMem
{
    void* mem;           // the allocation: [0, tables) the tables, [tables, bytes) the state
    size_t bytes, tables;
    bool host;           // in host memory (the _create_host handles)
    hipStream_t stream;

    uhsdr_status alloc(const char* who)
    {
        if (host)
        {
            mem = calloc(1, bytes);
            if (!mem) { uhsdr_set_error("%s: host allocation of %zu bytes failed", who, bytes); return UHSDR_DEVICE_ERROR; }
            return UHSDR_OK;
        }
        const hipError_t e = hipMalloc(&mem, bytes);
        if (e != hipSuccess)
        {
            mem = nullptr;
            uhsdr_set_error("%s: device allocation of %zu bytes failed: %s", who, bytes, hipGetErrorString(e));
            return UHSDR_DEVICE_ERROR;
        }
        return UHSDR_OK;
    }

    // fill(char* image) writes the first `tables` bytes: in place, or into a zeroed host image that
    // goes up in one synchronous copy
    template <class Fill> uhsdr_status upload_tables(const char* who, Fill fill)
    {
        if (host) { fill((char*)mem); return UHSDR_OK; }
        char* image = (char*)calloc(1, tables);
        if (!image) { uhsdr_set_error("%s: host allocation of %zu bytes failed", who, tables); return UHSDR_DEVICE_ERROR; }
        fill(image);
        const hipError_t e = hipMemcpy(mem, image, tables, hipMemcpyHostToDevice);
        free(image);
        if (e != hipSuccess) { uhsdr_set_error("%s: table upload failed: %s", who, hipGetErrorString(e)); return UHSDR_DEVICE_ERROR; }
        return UHSDR_OK;
    }

    // everything behind the tables to zero, on the handle's stream
    uhsdr_status zero_state()
    {
        if (host) memset((char*)mem + tables, 0, bytes - tables);
        else HIPCHK(hipMemsetAsync((char*)mem + tables, 0, bytes - tables, stream));
        return UHSDR_OK;
    }

    uhsdr_status synchronize()
    {
        if (!host) HIPCHK(hipStreamSynchronize(stream));
        return UHSDR_OK;
    }

    // after the work enqueued; a handle whose allocation failed has nothing to release
    void release()
    {
        if (host) free(mem);
        else if (mem)
        {
            (void)hipStreamSynchronize(stream);
            (void)hipFree(mem);
        }
        mem = nullptr;
    }
};

// `drain`: wait for the old stream before leaving it.  The modules whose host side reads device
// state back (the text queues) pass true; the decoders' set_stream runs on every call of the
// receive chain and only stores the stream.
static inline uhsdr_status arena_set_stream(ArenaMem* m, const char* who, void* stream, bool drain)
{
    if (!m || m->host) { uhsdr_set_error("%s: not a device handle", who); return UHSDR_ARGUMENT_ERROR; }
    if (drain && (hipStream_t)stream != m->stream) HIPCHK(hipStreamSynchronize(m->stream));
    m->stream = (hipStream_t)stream;
    return UHSDR_OK;
}

// n items whose last one lies `span` elements into a row of `stride`
static inline uhsdr_status arena_check_row(const char* who, const char* what, int32_t n, int64_t span, int32_t stride)
{
    if (n < 0 || stride < 0 || span > stride) { uhsdr_set_error("%s: %d %s do not fit a row of %d", who, n, what, stride); return UHSDR_LENGTH_ERROR; }
    return UHSDR_OK;
}

// an entry point for host handles refuses a device handle and the other way round; `use` names the right call
static inline bool arena_wrong_kind(const ArenaMem* m, bool want_host, const char* who, const char* use)
{
    if (m->host != want_host) uhsdr_set_error("%s: %s handle, use %s", who, m->host ? "host" : "device", use);
    return m->host != want_host;
}

#endif
