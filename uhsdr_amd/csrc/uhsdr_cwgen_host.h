/*
 * The CW generator's handle, for the two files that launch its kernels: uhsdr_cwgen.hip (cwgen_gen,
 * stand-alone) and uhsdr_tx.hip (tx_cw, inside the transmit chain).
 */
#ifndef UHSDR_CWGEN_HOST_H
#define UHSDR_CWGEN_HOST_H

#include "uhsdr_digimod_host.h"
#include "uhsdr_cwgen.h"

struct uhsdr_cwgen_s : DigiMod
{
    CwGenArena ca;          // ca.m is kept equal to a
    CwGenParams p;
    uint8_t* flags;         // [C][flag_blocks], the last call's
    int32_t flag_blocks;
};

// room for the flags of a call of `blocks` blocks; a larger call than any before allocates anew
uhsdr_status cg_flags_room(uhsdr_cwgen_s* h, int32_t blocks);

#endif
