// Kernel-variant tables of uhsdr_rx.hip (included there with <...>, so tools/isa/ can put a
// P48-only table of the same name first on the include path for quick ISA builds).
static const FrontVariant kFront[] = {
    FRONT_V(89, 43, 4, false, 16), FRONT_V(89, 43, 4, false, 8),     // wide SSB/CW  (P48-54)
    FRONT_V(89, 4, 2, false, 16), FRONT_V(89, 4, 2, false, 8),       // 24 ksps SSB   (P55-65)
    FRONT_V(83, 199, 4, true, 16), FRONT_V(83, 199, 4, true, 8),     // narrow SSB/CW (P4-47)
    FRONT_V(89, 0, 4, true, 16), FRONT_V(89, 0, 4, true, 8),         // AM / SAM, 12 ksps (P66-82)
    FRONT_V(89, 0, 2, true, 16), FRONT_V(89, 0, 2, true, 8),         // AM / SAM, 24 ksps (P83-86)
    FRONT_V(89, 0, 1, false, 16), FRONT_V(89, 0, 1, false, 8),       // FM, 48 ksps Hilbert pair (P1-3)
    // OVI40 stereo (DEMOD_SSBSTEREO / DEMOD_IQ with use_stereo): two channels out
    FRONT_ST(89, 43, 4, false, 16), FRONT_ST(89, 43, 4, false, 8),
    FRONT_ST(89, 4, 2, false, 16), FRONT_ST(89, 4, 2, false, 8),
    FRONT_ST(83, 199, 4, true, 16), FRONT_ST(83, 199, 4, true, 8),
};
#undef FRONT_V
#undef FRONT_ST

#define BACK_V(pre, aa, L, ph, w, dm) { pre, aa, L, ph, w, dm, rx_back<pre, aa, L, ph, w, dm>, rx_back_fused<pre, aa, L, ph, w, dm>, \
    fused_nodc_of<pre, aa, L, ph, w, dm>(), fused_ssb_of<pre, aa, L, ph, w, dm>(), pers_of<pre, aa, L, ph, w, dm>(), \
    tap_of<pre, aa, L, ph, w, dm>(), fused_tap_of<pre, aa, L, ph, w, dm>() }
static const BackVariant kBack[] = {
    // SSB / CW / DIGI
    BACK_V(10, 6, 4, 1, 49, DM_NONE), BACK_V(10, 0, 4, 4, 49, DM_NONE), BACK_V(0, 0, 2, 8, 97, DM_NONE),
    BACK_V(0, 6, 2, 2, 97, DM_NONE), BACK_V(10, 0, 2, 8, 97, DM_NONE), BACK_V(8, 0, 2, 8, 97, DM_NONE),
    BACK_V(8, 6, 2, 2, 97, DM_NONE),
    // AM / SAM paths P66-86
    BACK_V(10, 0, 4, 4, 49, DM_AM), BACK_V(10, 6, 4, 1, 49, DM_AM), BACK_V(10, 0, 2, 8, 97, DM_AM),
    BACK_V(8, 0, 2, 8, 97, DM_AM), BACK_V(8, 6, 2, 2, 97, DM_AM),
    BACK_V(10, 0, 4, 4, 49, DM_SAM), BACK_V(10, 6, 4, 1, 49, DM_SAM), BACK_V(10, 0, 2, 8, 97, DM_SAM),
    BACK_V(8, 0, 2, 8, 97, DM_SAM), BACK_V(8, 6, 2, 2, 97, DM_SAM),
    BACK_V(10, 0, 4, 4, 49, DM_SAM_SB), BACK_V(10, 6, 4, 1, 49, DM_SAM_SB), BACK_V(10, 0, 2, 8, 97, DM_SAM_SB),
    BACK_V(8, 0, 2, 8, 97, DM_SAM_SB), BACK_V(8, 6, 2, 2, 97, DM_SAM_SB),
};
// FM: its own kernel (squelch lattice stages)
static const BackVariant kBackFm = { 0, 0, 1, 1, 0, DM_FM, rx_fm<6>, nullptr };
#undef BACK_V

// OVI40 stereo back ends (rx_back_stereo): SSB stereo / IQ families, and SAM stereo
#define BACK_ST(pre, aa, L, ph, w, dm) { pre, aa, L, ph, w, dm, rx_back_stereo<pre, aa, L, ph, w, dm>, rx_back_stereo<pre, aa, L, ph, w, dm> }
static const BackVariant kBackStereo[] = {
    BACK_ST(10, 6, 4, 1, 49, DM_NONE), BACK_ST(10, 0, 4, 4, 49, DM_NONE), BACK_ST(0, 0, 2, 8, 97, DM_NONE),
    BACK_ST(0, 6, 2, 2, 97, DM_NONE), BACK_ST(10, 0, 2, 8, 97, DM_NONE), BACK_ST(8, 0, 2, 8, 97, DM_NONE),
    BACK_ST(8, 6, 2, 2, 97, DM_NONE),
    BACK_ST(10, 0, 4, 4, 49, DM_SAM_ST), BACK_ST(10, 6, 4, 1, 49, DM_SAM_ST), BACK_ST(10, 0, 2, 8, 97, DM_SAM_ST),
    BACK_ST(8, 0, 2, 8, 97, DM_SAM_ST), BACK_ST(8, 6, 2, 2, 97, DM_SAM_ST),
};
#undef BACK_ST

// LMS auto notch (+ the AM / SAM demodulator ahead of it): decimation L, demodulator DM
static const NotchVariant kNotch[] = {
    { 4, DM_NONE, rx_notch<4, DM_NONE> }, { 2, DM_NONE, rx_notch<2, DM_NONE> },
    { 4, DM_AM, rx_notch<4, DM_AM> }, { 2, DM_AM, rx_notch<2, DM_AM> },
    { 4, DM_SAM, rx_notch<4, DM_SAM> }, { 2, DM_SAM, rx_notch<2, DM_SAM> },
    { 4, DM_SAM_SB, rx_notch<4, DM_SAM_SB> }, { 2, DM_SAM_SB, rx_notch<2, DM_SAM_SB> },
    { 4, DM_SAM_ST, rx_notch<4, DM_SAM_ST> }, { 2, DM_SAM_ST, rx_notch<2, DM_SAM_ST> },
};

// one front pass + back end per wave: the SSB / CW / DIGI families of kFront x kBack (DM_NONE)
static const ChainVariant kChain[] = {
    CHAIN_V(89, 43, 4, false, 10, 6, 1, 49),             // wide SSB, 12 ksps (P48 ...)
    CHAIN_V(89, 43, 4, false, 10, 0, 4, 49),
    CHAIN_V(83, 199, 4, true, 10, 6, 1, 49),             // narrow SSB / CW, 12 ksps
    CHAIN_V(83, 199, 4, true, 10, 0, 4, 49),
    CHAIN_V(89, 4, 2, false, 0, 0, 8, 97),               // 24 ksps SSB
    CHAIN_V(89, 4, 2, false, 0, 6, 2, 97),
    CHAIN_V(89, 4, 2, false, 10, 0, 8, 97),
    CHAIN_V(89, 4, 2, false, 8, 0, 8, 97),
    CHAIN_V(89, 4, 2, false, 8, 6, 2, 97),
};

// the back end split around the noise reduction stage (uhsdr_rx_set_nr): the 12 ksps SSB / CW / DIGI back ends
static const NrStageVariant kNrStage[] = { NR_V(10, 6, 1, 49), NR_V(10, 0, 4, 49) };
