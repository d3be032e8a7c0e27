/*
 * The host side of a handle that owns per-channel text queues (uhsdr_digiq.h): what the RTTY and
 * BPSK modulators (uhsdr_digimod.hip) and the CW generator (uhsdr_cwgen.hip) have in common.
 */
#ifndef UHSDR_DIGIMOD_HOST_H
#define UHSDR_DIGIMOD_HOST_H

#include <hip/hip_runtime.h>

#include "uhsdr_internal.h"
#include "uhsdr_digiq.h"

struct DigiMod
{
    DigiModArena a;
    void* mem;           // one allocation behind the arena: the tables, then the state
    size_t bytes;
    bool host;           // state in host memory
    hipStream_t stream;
    uint32_t t;          // samples since reset
    // the producer's side of a device handle's queues, kept on the host: the put counters, the
    // queues' bytes, and room for the consumed counters read back at a put
    uint32_t* h_put;
    uint32_t* h_consumed;
    uint8_t* h_text;
};

// Appends to every channel's queue what fits of its row.  The free space of a queue depends on what
// the consumer has taken, so a device handle waits for the work enqueued and reads the counters back.
uhsdr_status dm_put_text(DigiMod* h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted);
uhsdr_status dm_set_stream(DigiMod* h, void* stream);
uhsdr_status dm_synchronize(DigiMod* h);

#endif
