// tools/isa_stats.sh, tools/build_ref_variant.sh: only the P48 SSB instances of uhsdr_rx.hip's
// variant tables, so one kernel's ISA compiles in seconds (-Itools/isa ahead of -Iuhsdr_amd/csrc).
static const FrontVariant kFront[] = { FRONT_V(89, 43, 4, false, 8) };
#define BACK_V(pre, aa, L, ph, w, dm) { pre, aa, L, ph, w, dm, rx_back<pre, aa, L, ph, w, dm>, rx_back_fused<pre, aa, L, ph, w, dm>, \
    fused_nodc_of<pre, aa, L, ph, w, dm>(), fused_ssb_of<pre, aa, L, ph, w, dm>(), pers_of<pre, aa, L, ph, w, dm>(), \
    tap_of<pre, aa, L, ph, w, dm>(), fused_tap_of<pre, aa, L, ph, w, dm>() }
static const BackVariant kBack[] = { BACK_V(10, 6, 4, 1, 49, DM_NONE) };
static const BackVariant kBackFm = { 0, 0, 1, 1, 0, DM_FM, rx_fm<6>, nullptr };
static const BackVariant kBackStereo[] = { { 10, 6, 4, 1, 49, DM_NONE, nullptr, nullptr } };
static const NotchVariant kNotch[] = { { 4, DM_NONE, nullptr } };
static const ChainVariant kChain[] = { CHAIN_V(89, 43, 4, false, 10, 6, 1, 49) };
static const NrStageVariant kNrStage[] = { NR_V(10, 6, 1, 49) };
#undef BACK_V
#undef FRONT_V
#undef FRONT_ST
