/*
 * The host side of a handle that owns per-channel text queues (uhsdr_digiq.h): what the RTTY and
 * BPSK modulators (uhsdr_digimod.hip) and the CW generator (uhsdr_cwgen.hip) have in common.
 */
#ifndef UHSDR_DIGIMOD_HOST_H
#define UHSDR_DIGIMOD_HOST_H

#include "uhsdr_arena.h"
#include "uhsdr_digiq.h"

struct DigiMod : ArenaMem
{
    DigiModArena a;
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
// the host's side of a device handle's queues, after the allocation and before the reset
uhsdr_status dm_alloc_queues(DigiMod* h, const char* who);
// the allocation after the work enqueued, and the host's side of the queues
void dm_free(DigiMod* h);
// What is enqueued on the old stream reads and writes the state and the queues: the new stream's
// work, and a put_text that waits for the new stream only, must come after it.  So these drain.
static inline uhsdr_status dm_set_stream(DigiMod* h, void* stream) { return arena_set_stream(h, "digimod", stream, true); }
static inline uhsdr_status dm_synchronize(DigiMod* h) { return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR; }

#endif
