/*
 * Fixture recorder for the signal meter, first of two translation units: the reference's
 * ui_spectrum.c, included where it lies, for its static UiSpectrum_CalculateDBm.
 *
 * The file assembles on x86 once __DSB is empty.  Lbin, Ubin and posbin are locals of
 * UiSpectrum_CalculateDBm; the only macro the function expands after it has clamped them is
 * SCOPE_PREAMP_GAIN, so that macro is given a comma expression here that notes the three and then
 * yields the reference's own value.  Nothing else of the function changes.  Nothing of this program
 * or its output other than the recorded data is committed.
 */
#include "uhsdr_board.h"
#include "arm_math.h"
#undef __DSB
#define __DSB() ((void)0)
#include "ui_spectrum.h"

int MeterRec_bins[3];
static inline int MeterRec_note(float lbin, float ubin, int posbin)
{
    MeterRec_bins[0] = (int)lbin;
    MeterRec_bins[1] = (int)ubin;
    MeterRec_bins[2] = posbin;
    return SCOPE_PREAMP_GAIN;
}
static const int MeterRec_gain = SCOPE_PREAMP_GAIN;
#undef SCOPE_PREAMP_GAIN
#define SCOPE_PREAMP_GAIN (MeterRec_note(Lbin, Ubin, posbin), MeterRec_gain)

#include "ui_spectrum.c"

void MeterRec_CalculateDBm(void) { UiSpectrum_CalculateDBm(); }
