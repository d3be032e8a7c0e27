/*
 * The display stage's handle, for the two sources that launch its frame: uhsdr_display.hip (the
 * stand-alone kernel, the host twin, the handle's life) and uhsdr_spectrum.hip (the epilogue of the
 * spectrum kernel).  Host code only.
 */
#ifndef UHSDR_DISPLAY_HOST_H
#define UHSDR_DISPLAY_HOST_H

#include "uhsdr_arena.h"
#include "uhsdr_display.h"

struct uhsdr_display_s : ArenaMem
{
    int32_t C;
    uhsdr_display_plan plan;            // the host's copy
    uhsdr_display_plan* d_plan;         // the tables of the allocation: the plan where the kernels read it
    float* state;                       // [DISPLAY_STATE_WORDS][C]: offset, min
};

// the kernel arguments of a call that runs F frames per channel; io null: no rows
static inline DisplayArgs display_args(const uhsdr_display_s* h, const uhsdr_display_io* io, int F)
{
    DisplayArgs a = {};
    a.plan = h->d_plan;
    a.state = h->state;
    if (io) a.io = *io;
    a.C = h->C;
    a.F = F;
    return a;
}

#endif
