/*
 * The signal meter's handle, for the two sources that launch its frame: uhsdr_meter.hip (the
 * stand-alone kernel, the host twin, the handle's life) and uhsdr_spectrum.hip (the epilogue of the
 * spectrum kernel).  Host code only.
 */
#ifndef UHSDR_METER_HOST_H
#define UHSDR_METER_HOST_H

#include "uhsdr_arena.h"
#include "uhsdr_meter.h"

struct uhsdr_meter_s : ArenaMem
{
    int32_t C;
    uhsdr_meter_plan plan;              // the host's copy
    uhsdr_meter_plan* d_plan;           // the tables of the allocation: the plan where the kernels read it
    uint32_t* state;                    // [METER_STATE_WORDS][C]
};

// the kernel arguments of a call that runs F frames per channel; io null: no rows
static inline MeterArgs meter_args(const uhsdr_meter_s* h, const uhsdr_meter_io* io, int F)
{
    MeterArgs a = {};
    a.plan = h->d_plan;
    a.state = h->state;
    if (io) a.io = *io;
    a.C = h->C;
    a.F = F;
    return a;
}

#endif
