/*
 * arm_bitreversal_32 in C for the noise-reduction recorders (tools/nr/nr.mk links it into both):
 * arm_cfft_f32 calls it, and the reference has it as ARM assembly only.  Restated from that listing
 * (arm_bitreversal2.S:136-180, CM7 branch), as oracle/ref/ref_spectrum.c did: (bitRevLen + 1) >> 2
 * iterations of two swaps each, the table entries being byte offsets of 8-byte complex values.
 */
#include <stdint.h>

void arm_bitreversal_32(uint32_t* w, const uint16_t len, const uint16_t* tab)
{
    for (uint32_t it = 0; it < (uint32_t)((len + 1) >> 2); ++it)
        for (int s = 0; s < 2; ++s)
        {
            const uint32_t a = tab[4 * it + 2 * s] >> 2, b = tab[4 * it + 2 * s + 1] >> 2;
            uint32_t t = w[a]; w[a] = w[b]; w[b] = t;
            t = w[a + 1]; w[a + 1] = w[b + 1]; w[b + 1] = t;
        }
}
