/*
 * uhsdr.h -- C ABI of the MI355X-native UHSDR RX DSP hot path (libuhsdr_amd.so).
 *
 * Drop-in boundary for the reference firmware's per-block receive chain
 * (SURVEY.md §8(b)):
 *
 *   reference                                             this ABI
 *   ---------------------------------------------------   --------------------------------
 *   AudioDriver_SetProcessingChain(dmod_mode, reset)      uhsdr_rx_plan_build()  (host setup,
 *     drivers/audio/audio_driver.c:1093-1251                restates the chain selection,
 *   AudioFilter_SetRxHilbertAndDecimationFIR()              filter tables, biquad designers
 *     drivers/audio/audio_filter.c:1134-1223                and AGC parameter math)
 *   AudioAgc_SetupAgcWdsp(rate, remove_dc)
 *     drivers/audio/audio_agc.c:126-339
 *   AudioDriver_Init() + SetProcessingChain()             uhsdr_rx_create() / uhsdr_rx_reset()
 *     audio_driver.c:677-704                                (zeroes all per-channel state)
 *   AudioDriver_I2SCallback(audio, iq, dst, 32)           uhsdr_rx_process()  -- C channels x
 *     audio_driver.c:2962-3049 ->                           N frames per call, N % 32 == 0,
 *   AudioDriver_RxProcessor(iq, audio, 32, mute)            one call == N/32 consecutive ISR
 *     audio_driver.c:2603-2942                              invocations on every channel
 *
 * Buffers follow the firmware's DMA formats, channel-major:
 *   iq    : IqSample_t    {int32 l (I), int32 r (Q)}  [C][N]  (audio_driver.h:44-52)
 *   audio : float         adb.a_buffer[1]             [C][N]  (audio_driver.h:147-157)
 *   dst   : AudioSample_t {int32 l, int32 r}           [C][N]  codec frames (audio_driver.c:2911-2923)
 * Device pointers are HIP device allocations.  Status codes follow CMSIS arm_status
 * (CMSIS/Include/arm_math.h:375-382): 0 success, -1 argument error, -2 length error.
 *
 * Threading: a handle is not re-entrant (like the ISR, audio_driver.c:1804-1806); calls on
 * one handle are ordered on the handle's HIP stream.  Different handles are independent.
 */
#ifndef UHSDR_H
#define UHSDR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UHSDR_ABI_VERSION 9

typedef enum
{
    UHSDR_OK = 0,                 /* ARM_MATH_SUCCESS */
    UHSDR_ARGUMENT_ERROR = -1,    /* ARM_MATH_ARGUMENT_ERROR */
    UHSDR_LENGTH_ERROR = -2,      /* ARM_MATH_LENGTH_ERROR: N % 32 != 0, bad sizes */
    UHSDR_UNSUPPORTED = -10,      /* mode / filter path not implemented on the device yet */
    UHSDR_DEVICE_ERROR = -11,     /* HIP runtime error */
    UHSDR_TIMEOUT = -12           /* a bounded device-side poll gave up (the pipelined device hand-off,
                                     uhsdr_rx_set_pipelined 2): outputs and handle state are invalid
                                     until uhsdr_rx_reset */
} uhsdr_status;

/* sam_sideband_t, drivers/audio/audio_driver.h:181-190 (STEREO: USE_TWO_CHANNEL_AUDIO, OVI40) */
enum { UHSDR_SAM_SIDEBAND_BOTH = 0, UHSDR_SAM_SIDEBAND_LSB = 1, UHSDR_SAM_SIDEBAND_USB = 2,
       UHSDR_SAM_SIDEBAND_STEREO = 3 };

/* DemodModes_t, hardware/uhsdr_board.h:72-85 (SSBSTEREO / IQ: USE_TWO_CHANNEL_AUDIO, OVI40) */
enum { UHSDR_DEMOD_USB = 0, UHSDR_DEMOD_LSB = 1, UHSDR_DEMOD_CW = 2, UHSDR_DEMOD_AM = 3,
       UHSDR_DEMOD_SAM = 4, UHSDR_DEMOD_FM = 5, UHSDR_DEMOD_DIGI = 6, UHSDR_DEMOD_SSBSTEREO = 7,
       UHSDR_DEMOD_IQ = 8 };

/* FREQ_IQ_CONV_*, drivers/audio/audio_driver.h:520-526 */
enum { UHSDR_IQ_CONV_OFF = 0, UHSDR_IQ_CONV_P6KHZ = 1, UHSDR_IQ_CONV_M6KHZ = 2,
       UHSDR_IQ_CONV_P12KHZ = 3, UHSDR_IQ_CONV_M12KHZ = 4 };

/* ts.dsp.active bits honoured by the chain (drivers/audio/audio_driver.h:195-200) */
#define UHSDR_DSP_NOTCH_ENABLE  0x04      /* LMS auto notch (AudioDriver_NotchFilter) */
#define UHSDR_DSP_MNOTCH_ENABLE 0x10
#define UHSDR_DSP_MPEAK_ENABLE  0x20

#define UHSDR_IQ_BLOCK_SIZE 32        /* IQ_BLOCK_SIZE, hardware/uhsdr_board_config.h:217 */
#define UHSDR_FILTER_PATH_NUM 87      /* AUDIO_FILTER_PATH_NUM, audio_filter.h:139 */
#define UHSDR_MAX_FIR_TAPS 200        /* IQ_RX_NUM_TAPS_MAX (199 rounded) */
#define UHSDR_MAX_DEC_TAPS 96         /* 89-tap AM tables reused as decimator */
#define UHSDR_MAX_LATTICE 10          /* IIR_RXAUDIO_NUM_STAGES_MAX */
#define UHSDR_MAX_INTERP 16
#define UHSDR_AGC_RING 192            /* AGC_WDSP_RB_SIZE, audio_agc.c:19 */

/*
 * User-facing receiver configuration: the subset of TransceiverState `ts` /
 * AudioDriverState `ads` / agc_wdsp_conf that the RX chain reads.  Defaults
 * (uhsdr_rx_config_default) are the firmware's, drivers/ui/ui_configuration.c:70-230.
 */
typedef struct uhsdr_rx_config
{
    int32_t dmod_mode;            /* ts.dmod_mode */
    int32_t filter_path;          /* ts.filter_path_mem[mode][0]: index into FilterPathInfo */
    int32_t iq_freq_mode;         /* ts.iq_freq_mode */
    int32_t iq_auto_correction;   /* ts.iq_auto_correction */
    float   iq_gain_i;            /* ts.rx_adj_gain_var.i */
    float   iq_gain_q;            /* ts.rx_adj_gain_var.q */
    float   iq_phase_balance;     /* ads.iq_phase_balance_rx */
    int32_t dsp_active;           /* ts.dsp.active (MNOTCH / MPEAK bits) */
    int32_t notch_frequency;      /* ts.dsp.notch_frequency */
    int32_t peak_frequency;       /* ts.dsp.peak_frequency */
    int32_t bass_gain;            /* ts.dsp.bass_gain */
    int32_t treble_gain;          /* ts.dsp.treble_gain */
    int32_t cw_lsb;               /* ts.cw_lsb */
    int32_t digi_lsb;             /* ts.digi_lsb */
    int32_t agc_mode;             /* agc_wdsp_conf.mode */
    int32_t agc_slope;            /* agc_wdsp_conf.slope */
    int32_t agc_thresh;           /* agc_wdsp_conf.thresh */
    int32_t agc_hang_enable;      /* agc_wdsp_conf.hang_enable */
    int32_t agc_hang_time;        /* agc_wdsp_conf.hang_time (500) */
    int32_t agc_hang_thresh;      /* agc_wdsp_conf.hang_thresh (45) */
    int32_t agc_tau_decay[6];     /* agc_wdsp_conf.tau_decay[] */
    int32_t agc_tau_hang_decay;   /* agc_wdsp_conf.tau_hang_decay */
    int32_t sam_sideband;         /* ads.sam_sideband: 0 both, 1 LSB, 2 USB (audio_driver.h:181-190) */
    int32_t sam_pll_fmax;         /* ads.pll_fmax_int (2500) */
    int32_t sam_zeta;             /* ads.zeta_int, zeta x 100 (65) */
    int32_t sam_omega_n;          /* ads.omegaN_int (250) */
    int32_t fade_leveler;         /* ads.fade_leveler (1) */
    int32_t fm_sql_threshold;     /* ts.fm_sql_threshold (FM_SQUELCH_DEFAULT 12, audio_driver.h:449) */
    int32_t fm_deviation_5k;      /* FLAGS2_FM_MODE_DEVIATION_5KHZ (RadioManagement_FmDevIs5khz) */
    int32_t cw_sidetone_freq;     /* ts.cw_sidetone_freq (750): the CW decoder's Goertzel frequency */
    int32_t cw_decoder_blocksize; /* cw_decoder_config.blocksize (88, 8..128, cw_decoder.h:12-13) */
    int32_t cw_decoder_thresh;    /* cw_decoder_config.thresh (32000, cw_decoder.h:15-17) */
    int32_t cw_decoder_noisecancel; /* cw_decoder_config.noisecancel_enable (1) */
    /* ABI 2 */
    int32_t notch_mu;             /* ts.dsp.notch_mu (DSP_NOTCH_MU_DEFAULT 10, 0..40): LMS auto notch
                                     convergence; the notch runs with UHSDR_DSP_NOTCH_ENABLE in dsp_active */
    int32_t fm_tone_det;          /* ts.fm_subaudible_tone_det_select: 0 off, else index into
                                     fm_subaudible_tone_table (FM subaudible tone detector) */
    int32_t beep_frequency;       /* ts.beep_frequency (DEFAULT_BEEP_FREQUENCY 1000 Hz) */
    int32_t beep_loudness;        /* ts.beep_loudness (DEFAULT_BEEP_LOUDNESS 10) */
    int32_t stereo_enable;        /* ts.stereo_enable: two-channel audio in DEMOD_SSBSTEREO, DEMOD_IQ and
                                     SAM with UHSDR_SAM_SIDEBAND_STEREO (audio_driver.c:2618) */
    /* ABI 3 */
    int32_t board;                /* UHSDR_BOARD_OVI40 (default: USE_TWO_CHANNEL_AUDIO, the oracle's build)
                                     or UHSDR_BOARD_MCHF (single-channel audio, UI_BRD_MCHF) */
    int32_t spkr_gain;            /* ts.rx_gain[RX_AUDIO_SPKR].value (mcHF: a software gain above
                                     CODEC_SPEAKER_MAX_VOLUME 16, audio_driver.c:2880-2885) */
    int32_t reserved[9];
} uhsdr_rx_config;

/* the UI board the firmware is built for (hardware/uhsdr_board_config.h:16-24): its output stage
   (audio_driver.c:2856-2897).  OVI40 (USE_TWO_CHANNEL_AUDIO): a_buffer[1] x10 in place, a_buffer[0]
   its copy (or the second channel), key beep on both.  mcHF (no USE_TWO_CHANNEL_AUDIO): a_buffer[0]
   = 10 x a_buffer[1] (line out), a_buffer[1] the speaker channel with the software gain
   (spkr_gain / 2.5 - 5.35, ui_driver.c:3083-3092) above volume 16, key beep on a_buffer[1] only; no
   two-channel modes (DEMOD_SSBSTEREO / DEMOD_IQ unsupported, no SAM_SIDEBAND_STEREO). */
enum { UHSDR_BOARD_OVI40 = 0, UHSDR_BOARD_MCHF = 1 };

/* AudioAgc_SetupAgcWdsp() results (audio_agc.c:126-339) */
typedef struct uhsdr_agc_plan
{
    int32_t mode;                 /* 5 == fixed gain (AGC off) */
    int32_t hang_enable;
    int32_t remove_dc;
    int32_t ring_buffsize;        /* 192 */
    int32_t attack_buffsize;      /* ceilf(rate * n_tau * tau_attack): 49 at 12 ksps */
    int32_t out_index0;           /* -1 */
    int32_t in_index0;            /* (attack_buffsize + out_index0) % ring_buffsize */
    int32_t hang_counter_init;    /* (int)(hangtime * sample_rate) */
    float   sample_rate;
    float   fixed_gain, attack_mult, decay_mult, fast_decay_mult, fast_backmult;
    float   onemfast_backmult, hang_backmult, onemhang_backmult, hang_decay_mult;
    float   pop_ratio, hang_level, min_volts, inv_max_input, out_target, slope_constant;
    float   hangtime, hang_thresh, var_gain, max_gain, inv_out_target;
} uhsdr_agc_plan;

/*
 * Resolved processing chain (what SetProcessingChain leaves in the driver's instances).
 * Built on the host; uploaded once per handle; read-only for the kernels.
 */
typedef struct uhsdr_rx_plan
{
    int32_t dmod_mode, filter_path, lsb;
    int32_t decimation_rate;      /* ads.decimation_rate */
    int32_t decimated_freq;       /* ads.decimated_freq */
    int32_t use_decimated_iq;     /* audio_driver.c:2718-2720 */
    int32_t iq_auto_correction;
    float   iq_gain_i, iq_gain_q, iq_phase_balance;
    int32_t freq_shift_hz;        /* AudioDriver_GetTranslateFreq(), audio_driver.c:445-464 */
    int32_t shift_kind;           /* 0 none, 1 Fs/4 exchange, 2 recursive oscillator */
    int32_t shift_up;             /* dir == FREQ_SHIFT_UP (freq_shift.c:324) */
    float   osc_cos, osc_sin;     /* FreqShift_Approx_Prepare, freq_shift.c:40-52 */
    int32_t hilbert_taps;         /* 0 => Hilbert skipped (AM/SAM) */
    float   hilbert_i[UHSDR_MAX_FIR_TAPS];
    float   hilbert_q[UHSDR_MAX_FIR_TAPS];
    int32_t dec_taps;
    float   dec[UHSDR_MAX_DEC_TAPS];
    int32_t pre_stages;
    float   pre_k[UHSDR_MAX_LATTICE];
    float   pre_v[UHSDR_MAX_LATTICE + 1];
    int32_t interp_L, interp_phase;  /* INTERPOLATE_RX: L, phaseLength (quirk: numTaps/L) */
    float   interp[UHSDR_MAX_INTERP];
    int32_t aa_stages;
    float   aa_k[UHSDR_MAX_LATTICE];
    float   aa_v[UHSDR_MAX_LATTICE + 1];
    float   biquad1[20];          /* IIR_biquad_1: 4 stages {b0,b1,b2,a1,a2} */
    float   biquad2[5];           /* IIR_biquad_2: 1 stage */
    float   post_agc_scale;       /* audio_driver.c:2513-2524 */
    float   line_out_scale;       /* LINE_OUT_SCALING_FACTOR, audio_driver.h:396 (mcHF: 1, see below) */
    uhsdr_agc_plan agc;
    /* AM / SAM (AudioDriver_DemodSAM, audio_driver.c:1990-2166) */
    float   dec_q[UHSDR_MAX_DEC_TAPS];  /* DECIMATE_RX_Q taps: the path's Q table for AM/SAM (audio_filter.c:1167-1176) */
    int32_t sam_sideband, fade_leveler;
    /* AudioDriver_SetSamPllParameters, audio_driver.c:709-745 */
    float   sam_omega_min, sam_omega_max, sam_g1, sam_g2;
    float   fade_mtauR, fade_onem_mtauR, fade_mtauI, fade_onem_mtauI;
    /* FM (AudioDriver_DemodFM, audio_driver.c:1544-1737) */
    float   fm_scale;             /* FM_RX_SCALING_2K5 10000 or _5K 5000 (audio_driver.c:1494-1495) */
    int32_t fm_sql_threshold;
    int32_t sq_stages;            /* IIR_Squelch_HPF = IIR_15k_hpf (audio_driver.c:481-484) */
    float   sq_k[UHSDR_MAX_LATTICE];
    float   sq_v[UHSDR_MAX_LATTICE + 1];
    /* CW decoder front end (CwDecode_RxProcessor, cw_decoder.c:383-397, 182-316): Goertzel per
       block on a_buffer[0] after biquad_1, in CW / AM / SAM at 12 ksps (audio_driver.c:2550-2557) */
    int32_t cw_enabled, cw_blocksize, cw_noisecancel;
    float   cw_thresh;
    float   cw_r, cw_cos, cw_sin;     /* AudioFilter_CalcGoertzel (audio_filter.c:1281-1288) */
    /* ABI 2 */
    /* LMS auto notch: AudioDriver_NotchFilter (audio_driver.c:1746-1763) -> arm_lms_norm_f32 on
       a_buffer[0] at the decimated rate, before the pre-filter (:2443-2456); set up at :1166-1186 */
    int32_t notch_enabled;        /* DSP_NOTCH_ENABLE, not in CW, not in SAM at 24 ksps */
    int32_t notch_taps;           /* ts.dsp.notch_numtaps (DSP_NOTCH_NUMTAPS_DEFAULT 64) */
    int32_t notch_delay_len;      /* ts.dsp.notch_delaybuf_len (DSP_NOTCH_DELAYBUF_DEFAULT 128) */
    float   notch_mu;             /* log10f(((notch_mu + 1.0) / 1500.0) + 1.0) */
    /* FM subaudible tone detector (audio_driver.c:1665-1734), Goertzels of
       AudioManagement_CalcSubaudibleDetFreq (audio_management.c:313-326): FM_HIGH, FM_LOW, FM_CTR */
    int32_t tone_det_enabled;
    float   tone_r[3], tone_cos[3], tone_sin[3];
    /* key beep: softdds step and loudness (AudioManagement_KeyBeepPrepare, audio_management.c:354-363) */
    uint32_t beep_step;
    float   beep_scale;
    /* OVI40 two-channel audio (use_stereo, audio_driver.c:2618): 0 mono, 1 SSB stereo
       (a_buffer[0] = I + Q, [1] = I - Q), 2 IQ (a_buffer[0] = I, [1] = Q), 3 SAM stereo */
    int32_t stereo;
    int16_t dds_table[1024];      /* softdds DDS_TABLE (softdds/dds_table.c) */
    /* ABI 3: output stage of the board (uhsdr_rx_config.board).  line_out_scale above is
       LINE_OUT_SCALING_FACTOR on OVI40 (a_buffer[1] x10 in place) and 1 on mcHF, where a_buffer[0]
       = line_out0_scale (LINE_OUT_SCALING_FACTOR) x biquad_2's output and a_buffer[1] = spkr_scale
       (the speaker's software gain, 1 at volume <= 16) x the same */
    int32_t single_channel;       /* 1: mcHF output stage */
    float   line_out0_scale;
    float   spkr_scale;
    int32_t reserved[29];
} uhsdr_rx_plan;

typedef struct uhsdr_rx_s* uhsdr_rx_handle;

/* ---- host setup layer ---- */
void         uhsdr_rx_config_default(uhsdr_rx_config* cfg);
uhsdr_status uhsdr_rx_plan_build(const uhsdr_rx_config* cfg, uhsdr_rx_plan* plan);
/* 1 if the device chain implements this plan, 0 otherwise */
int          uhsdr_rx_plan_supported(const uhsdr_rx_plan* plan);
/* 1 if uhsdr_rx_set_precision accepts UHSDR_PRECISION_FMA for this plan: the Hilbert-first
 * families whose FMA output was measured within 1e-5 normwise of the reference
 * (tools/fma_sweep.py, tests/test_gpu_fma.py), 0 otherwise */
int          uhsdr_rx_plan_fma_ok(const uhsdr_rx_plan* plan);

/* ---- batched device chain ---- */
/* stream: hipStream_t to order all work of this handle on (NULL = default stream). */
uhsdr_status uhsdr_rx_create(const uhsdr_rx_config* cfg, int32_t num_channels, int32_t frames_per_call,
                             void* stream, uhsdr_rx_handle* out);
uhsdr_status uhsdr_rx_reset(uhsdr_rx_handle h);
/* iq, audio, dst: device pointers ([C][N][2] int32, [C][N] f32, [C][N][2] int32).
   audio or dst may be NULL (not written).  Asynchronous on the handle's stream. */
uhsdr_status uhsdr_rx_process(uhsdr_rx_handle h, const int32_t* iq, float* audio, int32_t* dst);
/* OVI40 two-channel modes (plan.stereo != 0): audio = adb.a_buffer[1] (channel 0, codec left),
   audio0 = adb.a_buffer[0] (channel 1, codec right), dst = both channels {l, r}; either may be
   NULL.  Without stereo on OVI40, audio0 is not written (a_buffer[0] is a copy of a_buffer[1]);
   on mcHF (uhsdr_rx_config.board) audio0 gets a_buffer[0], the line-out channel. */
uhsdr_status uhsdr_rx_process_stereo(uhsdr_rx_handle h, const int32_t* iq, float* audio, float* audio0, int32_t* dst);
/* Same with host buffers: copies in, processes, copies out, synchronises. */
uhsdr_status uhsdr_rx_process_host(uhsdr_rx_handle h, const int32_t* iq, float* audio, int32_t* dst);
uhsdr_status uhsdr_rx_get_plan(uhsdr_rx_handle h, uhsdr_rx_plan* plan);
uhsdr_status uhsdr_rx_set_stream(uhsdr_rx_handle h, void* stream);
uhsdr_status uhsdr_rx_destroy(uhsdr_rx_handle h);

/* Wait until every call enqueued on the handle has finished (both streams when pipelined). */
uhsdr_status uhsdr_rx_synchronize(uhsdr_rx_handle h);

/* Pipelined mode (off by default).  On: rx_back runs on a private side stream and the
   decimated hand-off rotates over three buffers, so rx_front runs up to two calls ahead of rx_back —
   the streaming throughput of back-to-back ISR calls is max(front, back) instead of the sum.
   Results are identical; only their completion point moves: the audio / dst / CW outputs of
   a call are complete after uhsdr_rx_synchronize(), or for work enqueued on the handle's
   stream after uhsdr_rx_join() (which orders the handle stream after every rx_back issued
   so far).  The caller must not overwrite an output buffer still being written: reuse across
   calls is safe (rx_back launches are ordered on the side stream).  Replaces nothing in the
   reference (the firmware runs one ISR at a time); uhsdr_rx_process_host joins itself.
   enable = 1: each rx_back waits for its rx_front through a cross-stream event.
   enable = 2 (device hand-off): rx_front stores the decimated hand-off write-through and each of
   its waves, once its stores have completed, bumps an arrival counter of its 64-channel group;
   rx_back -- the wave-pipeline back end without a demodulator or notch (SSB / CW / DIGI), while
   its grid is at most half the CUs -- polls its group's counter on the device and reads the
   hand-off with L1-bypassing sc1 loads: no cross-stream wait and no extra kernel per call, so the
   side stream's back ends run back to back.  When the next call's front has already arrived, a
   back-end launch also runs its first pipeline roles ahead into that call instead of draining
   (bit-identical; the next launch then starts without a pipeline fill).  Other calls keep the
   event.
   enable = 3 (persistent back end): the device hand-off, and one rx_back launch runs call after
   call -- wave-pipeline back ends without the CW decoder and with calls of 256+ frames; others as
   enable = 2.  Each uhsdr_rx_process writes the call's descriptor (its hand-off buffer, outputs and
   key beep) into host-mapped memory and grants the call to the running launch, which takes it with
   its state in registers; a launch that finds no grant when it needs the next call ends (the host
   then starts a new one with the next call).  uhsdr_rx_join, uhsdr_rx_synchronize, uhsdr_rx_reset
   and every mode or schedule change end the running launch after the calls granted so far, so a
   device-wide synchronisation (or join) completes without further calls.  The host waits in
   uhsdr_rx_process before refilling a hand-off buffer the back end has not read yet (8 calls
   back).  Same failure contract as enable = 2 (a give-up inside a launch poisons the call it
   waited for, and may poison the end of the call before it).  A running launch waits for fronts
   enqueued after it, so the handle's side stream (made at the first uhsdr_rx_set_pipelined) must not
   share a hardware queue with the handle's stream: HIP spreads streams over GPU_MAX_HW_QUEUES queues
   (4 by default), so make the handle before other streams of the process (a shared queue shows as a
   give-up, UHSDR_TIMEOUT, never as silent output).  Any other enable value returns
   UHSDR_ARGUMENT_ERROR.
   Failure contract of the device hand-off.  The poll is bounded (uhsdr_rx_set_handoff_bound,
   default 2^24 polls: seconds).  If rx_back gives up -- the handle's stream held the call's
   rx_front back that long behind other work, or a profiler serialised the two streams' dispatches
   -- then (1) that launch is poisoned: every frame of the call's audio is NaN (its codec frames
   carry what the reference's float -> int32 conversion makes of NaN, 0), so it cannot pass for
   output; (2) the handle's host-mapped failure word is set, and from
   then on uhsdr_rx_process, uhsdr_rx_join and uhsdr_rx_synchronize return UHSDR_TIMEOUT (join
   reports it once the give-up has happened, synchronize always after the calls before it); (3)
   uhsdr_rx_handoff_timeouts returns 1; (4) uhsdr_rx_reset clears the word and the poisoned state.
   Under a profiler that serialises dispatches (rocprofv3 --pmc) use enable = 1. */
uhsdr_status uhsdr_rx_set_pipelined(uhsdr_rx_handle h, int32_t enable);
/* Poll bound of the device hand-off (polls of >= 128 shader cycles each); for tests of the
   failure contract.  0 is UHSDR_ARGUMENT_ERROR.  A running persistent launch keeps the bound it
   started with. */
uhsdr_status uhsdr_rx_set_handoff_bound(uhsdr_rx_handle h, uint32_t polls);
/* 1 if a device hand-off poll gave up since the last uhsdr_rx_reset, else 0; -1 on error.
   Synchronises. */
int32_t      uhsdr_rx_handoff_timeouts(uhsdr_rx_handle h);

/* Arithmetic of the FIR dot products in rx_front (Hilbert pair, decimators, AM/FM I/Q filters).
   EXACT (default): a rounded multiply then a rounded add per tap, in tap order -- the binary32
   sequence of CMSIS arm_fir_f32 / arm_fir_decimate_f32 as the reference builds them, so every
   output is bit-identical to the reference chain.  FMA: one fused multiply-add per tap
   (v_pk_fma_f32), half the VALU issue; outputs within north_star's 1e-5 normwise relative
   tolerance of the reference (max|diff| / max|ref| per channel), not bit-identical.  The
   recursive stages (lattices, AGC, biquads, demodulators) always run the reference sequence.
   FMA is accepted only on the Hilbert-first families (wide SSB / CW / DIGI at 12 and 24 ksps,
   FM), where it stays within 1e-5; the decimate-first families (narrow SSB / CW, AM, SAM)
   amplify the FIR rounding difference past 1e-5 (1.3e-5 .. 1.8e-5 measured), so there the call
   returns UHSDR_UNSUPPORTED and the handle stays EXACT.
   Takes effect from the next uhsdr_rx_process. */
enum { UHSDR_PRECISION_EXACT = 0, UHSDR_PRECISION_FMA = 1 };
uhsdr_status uhsdr_rx_set_precision(uhsdr_rx_handle h, int32_t precision);
int32_t      uhsdr_rx_get_precision(uhsdr_rx_handle h);   /* -1 for a null handle */
uhsdr_status uhsdr_rx_join(uhsdr_rx_handle h);

/* Kernel schedule of a call (a launch-shape choice: outputs are bit-identical under every one).
 *   AUTO        (default) SPLIT_FUSED from 131072 channels on, else SPLIT_PIPE; CHAIN only
 *               when requested
 *   SPLIT_PIPE  rx_front, then rx_back: one wave per back-end stage, a pipeline over 32-frame
 *               calls (short per-call critical path: small batches)
 *   SPLIT_FUSED rx_front, then rx_back_fused: every back-end stage in one wave per 64 channels
 *   CHAIN       rx_chain: one kernel, each wave runs the front passes of its 64 channels and then
 *               their back end, the decimated hand-off kept in LDS (large batches).  SSB / CW /
 *               DIGI mono paths (no notch, no stereo, not AM / SAM / FM) with one front pass per
 *               call; elsewhere UHSDR_UNSUPPORTED.  Also refused: call sizes whose channels per
 *               front wave, 64 / (frames_per_call / 8) rounded down, do not divide 64 -- 96-frame
 *               (5) and 160-frame (3) calls; every power of two, 192 and 224 are taken.
 * Stereo, AM / SAM / FM and the LMS notch have their own back-end kernels and ignore SPLIT_*.
 * Returns UHSDR_UNSUPPORTED (handle unchanged) for a schedule the handle's path cannot run.
 * Takes effect from the next uhsdr_rx_process; get returns the resolved schedule. */
enum { UHSDR_SCHEDULE_AUTO = 0, UHSDR_SCHEDULE_SPLIT_PIPE = 1, UHSDR_SCHEDULE_SPLIT_FUSED = 2,
       UHSDR_SCHEDULE_CHAIN = 3 };
uhsdr_status uhsdr_rx_set_schedule(uhsdr_rx_handle h, int32_t schedule);
int32_t      uhsdr_rx_get_schedule(uhsdr_rx_handle h);    /* -1 for a null handle */
/* FIR outputs per lane of the front passes: 8 (default: more waves per batch) or 16 (fewer LDS
   window reads per MAC); UHSDR_UNSUPPORTED when the call size does not admit it (the handle keeps
   its block).  Bit-identical.  May be changed between calls in every mode of
   uhsdr_rx_set_pipelined.  Once the handle has used the device hand-off or the persistent back
   end (modes 2, 3), a change waits for every call enqueued so far, on both streams, and ends a
   running persistent launch: the hand-off's arrival counters count front waves, whose number
   changes with the block, so they restart.  In the serial mode and with the event hand-off it
   costs no synchronisation.  A handle on the CHAIN schedule falls back to the split kernels when
   rx_chain cannot run the new block. */
uhsdr_status uhsdr_rx_set_front_block(uhsdr_rx_handle h, int32_t outputs_per_lane);

/* ---- status side outputs: the RX chain's signals to the control plane ----
 * ADC clip indicators (audio_driver.c:2660-2676): per channel, the sticky flags ads.adc_clip /
 * ads.adc_half_clip / ads.adc_quarter_clip, set when |I| >> 16 of any frame exceeds
 * ADC_CLIP_WARN_THRESHOLD (4096, audio_driver.h:81) / its half / its quarter -- the S-meter's
 * red indicator and the auto RF-gain trigger / release.  The firmware's UI reads and clears
 * them; here the kernels OR the bits of every frame they process into clip[c] (device memory,
 * [C] uint32, the caller zeroes it and clears it after reading).  NULL (default) = not computed.
 * The level is a signed int32 as in the reference: abs(INT32_MIN) wraps to INT32_MIN, the shift
 * keeps it negative, and so a sample of exactly -2^31 raises no flag (the compiled reference's
 * behaviour); -(2^31-1) and 2^31-1 raise all three. */
#define UHSDR_ADC_CLIP          1
#define UHSDR_ADC_HALF_CLIP     2
#define UHSDR_ADC_QUARTER_CLIP  4
uhsdr_status uhsdr_rx_set_clip_output(uhsdr_rx_handle h, uint32_t* clip);
/* Twin-peaks I/Q fault detector (AudioDriver_RxHandleTwinpeaks, audio_driver.c:2173-2248), run
 * per 32-frame call with automatic I/Q correction: 1000 calls of settling, then 50 calls of the
 * Moseley & Slump phase estimate asin(teta1 / teta3), smoothed; more than 22.5 degrees requests a
 * codec restart, the fourth consecutive one declares the fault uncorrectable.  Per channel state
 * ts.twinpeaks_tested (hardware/uhsdr_board.h:647-651), WAIT after create / reset
 * (src/uhsdr_main.c:339). */
enum { UHSDR_TWINPEAKS_SAMPLING = 0, UHSDR_TWINPEAKS_DONE = 1, UHSDR_TWINPEAKS_WAIT = 2,
       UHSDR_TWINPEAKS_UNCORRECTABLE = 3, UHSDR_TWINPEAKS_CODEC_RESTART = 4 };
/* copies the C states (int32) to `state` (device memory), ordered on the handle's stream */
uhsdr_status uhsdr_rx_twinpeaks_state(uhsdr_rx_handle h, int32_t* state);
/* the UI's acknowledgement after it restarted the codec (ui_driver.c:7422-7426): every channel in
 * CODEC_RESTART goes back to WAIT; ordered on the handle's stream */
uhsdr_status uhsdr_rx_twinpeaks_rearm(uhsdr_rx_handle h);

/* ---- device memory for plain-C hosts (no HIP headers needed) ---- */
void*        uhsdr_device_alloc(uint64_t bytes);             /* NULL on failure */
void         uhsdr_device_free(void* p);
uhsdr_status uhsdr_copy_to_device(void* dst, const void* src, uint64_t bytes);
uhsdr_status uhsdr_copy_to_host(void* dst, const void* src, uint64_t bytes);

/* ================================ transmit ================================
 * TxProcessor_Run (drivers/audio/tx_processor.c:891-1078) for SSB (USB / LSB) voice:
 *   codec audio frames -> mic gain -> TX band-pass lattice -> bass/treble biquads ->
 *   ALC compressor with its 288-sample look-ahead delay -> 201-tap Hilbert pair ->
 *   FreqShift -> I/Q gain + phase -> int32 IQ frames for the DAC.
 * AM voice (TxProcessor_AM, :715-800, dispatch :1000-1008): the same voice chain with
 *   AM_ALC_GAIN_CORRECTION, the Hilbert pair, both sidebands plus carrier
 *   (I - Q + 2 * AM_CARRIER_LEVEL, Q - I - 2 * AM_CARRIER_LEVEL), FreqShift.
 * FM voice: the voice chain, pre-emphasis and the softdds modulator (:534-588).
 * USB I/Q source (TX_AUDIO_DIGIQ, :950-961): the input frames are the I/Q itself, straight to the
 *   final gain / phase stage (not in CW or TUNE, where the voice path runs as usual).
 * One uhsdr_tx_process call == N/32 TX-mode AudioDriver_I2SCallback invocations per channel.
 */
#define UHSDR_TX_HILBERT_TAPS 201    /* iq_tx_wide, drivers/audio/filters/iq_tx_filter.h:22 */
#define UHSDR_TX_DELAY 320           /* AUDIO_DELAY_BUFSIZE, audio_driver.h:516 */

/* TX_AUDIO_*, hardware/uhsdr_board.h:128-132 (DIG: USB audio in place of the codec's, no bass /
   treble; DIGIQ: USB I/Q).  Modes: UHSDR_DEMOD_USB / LSB (SSB voice), UHSDR_DEMOD_AM and
   UHSDR_DEMOD_FM (both need iq_freq_mode != OFF like the reference, tx_processor.c:1000-1011) */
enum { UHSDR_TX_AUDIO_MIC = 0, UHSDR_TX_AUDIO_LINEIN_L = 1, UHSDR_TX_AUDIO_LINEIN_R = 2, UHSDR_TX_AUDIO_DIG = 3,
       UHSDR_TX_AUDIO_DIGIQ = 4 };

typedef struct uhsdr_tx_config
{
    int32_t dmod_mode;            /* ts.dmod_mode: UHSDR_DEMOD_USB, _LSB, _AM, _FM, _DIGI (uhsdr_tx_set_rtty_mod) or _CW (uhsdr_tx_set_cw_keyer) */
    int32_t iq_freq_mode;         /* ts.iq_freq_mode */
    int32_t audio_source;         /* ts.tx_audio_source: MIC, LINEIN_L, LINEIN_R, DIG, DIGIQ */
    int32_t mic_gain_mult;        /* ts.tx_mic_gain_mult (codec.c:313-321) */
    int32_t mic_boost;            /* ts.tx_mic_boost */
    int32_t comp_level;           /* ts.tx_comp_level: -1 off, 0..12 presets, 13 = stored values */
    int32_t alc_decay;            /* ts.alc_decay (EEPROM, used by comp_level 13) */
    int32_t alc_postfilt_gain;    /* ts.alc_tx_postfilt_gain (EEPROM, used by comp_level 13) */
    int32_t tx_filter;            /* ts.tx_filter: 0/1 soprano, 2 tenor, 3 bass */
    int32_t bass_gain;            /* ts.dsp.tx_bass_gain */
    int32_t treble_gain;          /* ts.dsp.tx_treble_gain */
    int32_t filter_disable;       /* FLAGS1_SSB_TX_FILTER_DISABLE (SSB) / FLAGS1_AM_TX_FILTER_DISABLE (AM) */
    float   power_factor;         /* ts.tx_power_factor */
    float   gain_i, gain_q;       /* ts.tx_adj_gain_var[trans].i / .q */
    float   phase_balance;        /* ads.iq_phase_balance_tx[trans] */
    int32_t fm_deviation_5k;      /* FLAGS2_FM_MODE_DEVIATION_5KHZ: FM transmit deviation 5 kHz (else 2.5) */
    int32_t fm_subaudible_tone;   /* ts.fm_subaudible_tone_gen_select: index into fm_subaudible_tone_table, 0 = off */
    int32_t fm_tone_burst_mode;   /* ts.fm_tone_burst_mode: 0 off, 1 1750 Hz, 2 2135 Hz (fm_tone_burst_freq,
                                     audio_management.c:328), sent while uhsdr_tx_set_tone_burst is on */
    int32_t digi_lsb;             /* ts.digi_lsb: UHSDR_DEMOD_DIGI transmits on the lower sideband */
    int32_t cw_lsb;               /* ts.cw_lsb: UHSDR_DEMOD_CW exchanges I and Q (tx_processor.c:860-863) */
    /* the keyer of UHSDR_DEMOD_CW, as uhsdr_cwgen_config (defaults IAM_B, 20 wpm, weight 100, rx_delay 8, 750 Hz) */
    int32_t cw_keyer_mode, cw_keyer_speed, cw_keyer_weight, cw_paddle_reverse, cw_rx_delay, cw_sidetone_freq;
    int32_t reserved[5];
} uhsdr_tx_config;

typedef struct uhsdr_tx_plan
{
    int32_t dmod_mode, lsb, audio_source;
    float   in_gain;              /* gain_calc of TxProcessor_AudioBufferFill (tx_processor.c:354-381) */
    int32_t apply_in_gain;        /* gain_calc != 1.0 */
    int32_t run_lattice, run_biquad;
    int32_t lat_stages;
    float   lat_k[UHSDR_MAX_LATTICE];
    float   lat_v[UHSDR_MAX_LATTICE + 1];
    float   biquad[15];           /* IIR_TX_biquad: treble shelf 1700 Hz, bass shelf 300 Hz, passthrough */
    int32_t comp_on;              /* ts.tx_comp_level > -1 */
    float   postfilt_gain;        /* alc_tx_postfilt_gain_var / 2.0 + 0.5 */
    float   alc_decay;            /* ads.alc_decay (audio_management.c:15-19) */
    float   alc_gain_scaling;     /* SSB_ALC_GAIN_CORRECTION */
    float   hilbert_i[UHSDR_TX_HILBERT_TAPS + 7];   /* already swapped for LSB (tx_processor.c:477-478) */
    float   hilbert_q[UHSDR_TX_HILBERT_TAPS + 7];
    int32_t freq_shift_hz, shift_kind, shift_up;
    float   osc_cos, osc_sin;
    float   final_i_gain, final_q_gain;   /* tx_power_factor * tx_adj_gain_var * SSB_GAIN_COMP * 2^16 */
    float   phase_balance;
    /* FM transmit (TxProcessor_FM, tx_processor.c:534-588): pre-emphasis, optional sub-audible
       tone from a softdds NCO, 16-bit accumulator NCO over the softdds sine table */
    int32_t fm;
    float   fm_mod_mult;          /* 2 with 5 kHz deviation, else 1 */
    uint32_t fm_word;             /* (65536 * |translate_freq|) / 48000 */
    int32_t fm_swap;              /* translate_freq < 0: I and Q buffers exchanged */
    int32_t fm_sub_on;
    uint32_t fm_sub_step;         /* softdds_stepForSampleRate(tone, 48000) (softdds.c:26-32) */
    float   fm_sub_scale;         /* FM_SUBAUDIBLE_TONE_AMPLITUDE_SCALING * fm_mod_mult */
    int16_t dds_table[1024];      /* DDS_TABLE, softdds/dds_table.c */
    /* softdds tones: TUNE (AudioManagement_SetSidetoneForDemodMode, audio_management.c:377-404:
       SSB_TUNE_FREQ 750 Hz, two-tone + 1950 Hz) and the FM tone burst (LoadToneBurstMode :339-349) */
    uint32_t tune_step[2];
    uint32_t tone_burst_step;
    float   tone_burst_scale;     /* FM_TONE_BURST_AMPLITUDE_SCALING * fm_mod_mult */
    int32_t am;                   /* TxProcessor_AM: both sidebands + carrier after the Hilbert pair */
    int32_t digiq;                /* TX_AUDIO_DIGIQ: the input frames are I/Q for the final stage */
    float   digiq_i_gain, digiq_q_gain;   /* final gains with iq_gain_comp 1.0 (tx_processor.c:924); CW runs with these */
    int32_t cw;                   /* UHSDR_DEMOD_CW: TxProcessor_CW, lsb = cw_lsb */
    int32_t cw_keyer_mode, cw_keyer_speed, cw_keyer_weight, cw_paddle_reverse, cw_rx_delay, cw_sidetone_freq;
    int32_t reserved[17];
} uhsdr_tx_plan;

typedef struct uhsdr_tx_s* uhsdr_tx_handle;

void         uhsdr_tx_config_default(uhsdr_tx_config* cfg);
uhsdr_status uhsdr_tx_plan_build(const uhsdr_tx_config* cfg, uhsdr_tx_plan* plan);
/* audio: device AudioSample_t [C][N][2] int32 in; iq: device IqSample_t [C][N][2] int32 out;
   a0: optional device f32 [C][N], the compressed audio (adb.a_buffer[0]) */
uhsdr_status uhsdr_tx_create(const uhsdr_tx_config* cfg, int32_t num_channels, int32_t frames_per_call,
                             void* stream, uhsdr_tx_handle* out);
uhsdr_status uhsdr_tx_reset(uhsdr_tx_handle h);
uhsdr_status uhsdr_tx_process(uhsdr_tx_handle h, const int32_t* audio, int32_t* iq, float* a0);
uhsdr_status uhsdr_tx_get_plan(uhsdr_tx_handle h, uhsdr_tx_plan* plan);
uhsdr_status uhsdr_tx_destroy(uhsdr_tx_handle h);
/* pipelined mode (no reference counterpart; off by default): tx_iq -- the Hilbert pair, FreqShift
 * and DAC frames -- runs on a private side stream and the compressed-audio hand-off rotates over
 * two buffers, so tx_voice of call k+1 (one lane per channel, latency-bound) overlaps tx_iq of
 * call k.  Outputs are bit-identical; iq of a call is complete once uhsdr_tx_join has ordered the
 * handle's stream after the side stream (then synchronize that stream as usual). */
uhsdr_status uhsdr_tx_set_pipelined(uhsdr_tx_handle h, int32_t enable);
int32_t      uhsdr_tx_get_pipelined(uhsdr_tx_handle h);
uhsdr_status uhsdr_tx_join(uhsdr_tx_handle h);
/* Arithmetic of the 201-tap Hilbert pair in tx_iq (no reference counterpart; EXACT by default).
   EXACT: a rounded multiply then a rounded add per tap, in tap order -- arm_fir_f32's binary32
   sequence, bit-identical DAC frames.  FMA: one fused multiply-add per tap (v_pk_fma_f32), half
   the pair's VALU issue; the DAC frames stay within north_star's 1e-5 normwise relative tolerance
   (max|diff| / max|ref| per channel) of the reference.  The voice chain (lattice, biquads, ALC)
   and FM always run the reference sequence: the pair's output feeds no recursion, so its rounding
   difference is not amplified (every SSB / AM mode and frequency translation measured, tests/
   test_gpu_tx_precision.py).  Takes effect from the next uhsdr_tx_process. */
uhsdr_status uhsdr_tx_set_precision(uhsdr_tx_handle h, int32_t precision);
int32_t      uhsdr_tx_get_precision(uhsdr_tx_handle h);   /* -1 for a null handle */
/* TxProcessor_PrepareRun (tx_processor.c:63-66): clear the ALC look-ahead delay line only,
   the first time back to TX; all other TX state carries on */
uhsdr_status uhsdr_tx_prepare_run(uhsdr_tx_handle h);
/* TUNE (ts.tune with ts.tune_tone_mode): from the next uhsdr_tx_process on, the transmitter's audio
   is the softdds tone instead of the codec input (TxProcessor_AudioBufferFill, tx_processor.c:344-347;
   softdds_runIQ into one buffer keeps the quadrature sample), the TX filters and the post-filter
   gain are skipped (:444-447, :179), the ALC runs.  Entering and leaving TUNE reconfigures the
   tone generator with its phase reset (AudioManagement_SetSidetoneForDemodMode, as
   RadioManagement_SwitchTxRx does, radio_management.c:1035).  Common to all channels. */
enum { UHSDR_TUNE_OFF = 0, UHSDR_TUNE_SINGLE = 1, UHSDR_TUNE_TWO = 2 };
uhsdr_status uhsdr_tx_set_tune(uhsdr_tx_handle h, int32_t tune);
/* FM tone burst ("whistle-up", ads.fm_conf.tone_burst_active, tx_processor.c:555-564): while on,
   the fm_tone_burst_mode tone replaces the sub-audible tone in the FM modulator.  No effect for
   SSB or with fm_tone_burst_mode 0. */
uhsdr_status uhsdr_tx_set_tone_burst(uhsdr_tx_handle h, int32_t active);
/* DIGI transmit (dmod_mode UHSDR_DEMOD_DIGI; ts.dvmode with digital_mode RTTY or BPSK,
   tx_processor.c:973-983): the handle owns one modulator (uhsdr_rttymod_* / uhsdr_pskmod_* below,
   arguments as their create) and an int16 row [C][N].  With a modulator on, uhsdr_tx_process
   ignores `audio` (may be null) and runs TxProcessor_Rtty / TxProcessor_Psk (:811-845): N modulator
   samples per channel, the TX lattice (TxProcessor_FilterAudio(true, false): no bass / treble
   biquads, no input gain, no ALC), TxProcessor_SSB(..., 0, ts.digi_lsb): the Hilbert pair, swapped
   for digi_lsb, and no frequency translation whatever iq_freq_mode says, then the final stage with
   iq_gain_comp SSB_GAIN_COMP (RTTY) or 1.0 (BPSK).  a0 is a_buffer[0] after the lattice.  The
   transmitter is at zero IF in these modes (radio_management.c:587-605), so gain_i, gain_q and
   phase_balance of the config are the firmware's IQ_TRANS_OFF values.  The modulator kernel runs
   first on the handle's stream, the lattice in a kernel of its own that reads the row; tx_iq,
   pipelined mode and the FMA precision work as for SSB.
   One modulator at a time: enabling one while the other is on is UHSDR_ARGUMENT_ERROR, as are all
   five calls on a handle of another mode.  A DIGI handle without a modulator refuses
   uhsdr_tx_process, and uhsdr_tx_set_tune is refused on a DIGI handle (the firmware's dvmode branch
   never looks at ts.tune); the USB I/Q source is refused for DIGI at create.  uhsdr_tx_reset resets
   the modulator (queues emptied, StartTX / PrepareTx); uhsdr_tx_prepare_run does not touch it.
   mod_put_text, mod_start (StartTX / PrepareTx) and mod_outputs are the modulator's put_text,
   start_tx / prepare_tx and outputs.  Not built: the keyer as text entry
   (TxProcessor_CwInputForDigitalModes with a keyer mode other than STRAIGHT) and the OVI40 sidetone. */
typedef struct uhsdr_cwgen_s* uhsdr_cwgen_handle;
/* CW transmit (dmod_mode UHSDR_DEMOD_CW; TxProcessor_CW, tx_processor.c:856-888, :985-988): the handle
   owns one CW generator (uhsdr_cwgen_* below) with the config's keyer settings.  uhsdr_tx_process
   ignores `audio` (it may be null) and runs one kernel, tx_cw: the keyer, tone and envelope of every
   32-frame block, the exchange of I and Q unless cw_lsb (the generator's sine goes to Q in USB), a0 =
   the generator's I while the signal is active and 0 otherwise, and the final stage with iq_gain_comp
   1.0 (gain_i / gain_q are the IQ_TRANS_OFF gains: CW transmits at zero IF whatever iq_freq_mode says),
   the phase balance and the int32 DAC frames.  No lattice, ALC, Hilbert pair or frequency shift.
     set_cw_keyer(text_capacity, echo_capacity)  creates the generator (again: a fresh one)
     cw_keys(keys)     device uint8 [C][N/32], read by the following uhsdr_tx_process calls
     cw_put_text, cw_set_speed, cw_outputs   as uhsdr_cwgen_put_text / _set_speed / _outputs
   uhsdr_tx_set_tune (any mode but OFF): the continuous 750 Hz tone, every block active, the keyer
   stands still and the key bytes are not looked at; the tone's phase restarts at 0 on entering and
   on leaving.  uhsdr_tx_reset resets the keyer; uhsdr_tx_prepare_run leaves it alone.
   uhsdr_tx_set_pipelined and uhsdr_tx_set_precision are accepted and change nothing (one kernel, no
   FIR).  UHSDR_ARGUMENT_ERROR: these calls on a handle of another mode, the modulator calls on a CW
   handle, uhsdr_tx_process before set_cw_keyer or, outside TUNE, before cw_keys, and the USB I/Q
   source with CW at create.
   Not built: the keyer as text entry for RTTY / BPSK, CAT keying, the OVI40 sidetone, uhsdr_i2s_*
   with a CW transmitter, PTT sequencing (the TX-on / TX-off flags are outputs). */
uhsdr_status uhsdr_tx_set_cw_keyer(uhsdr_tx_handle h, int32_t text_capacity, int32_t echo_capacity);
uhsdr_status uhsdr_tx_cw_keys(uhsdr_tx_handle h, const uint8_t* keys);
uhsdr_status uhsdr_tx_cw_put_text(uhsdr_tx_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted);
uhsdr_status uhsdr_tx_cw_set_speed(uhsdr_tx_handle h, int32_t speed, int32_t weight);
uhsdr_status uhsdr_tx_cw_outputs(uhsdr_tx_handle h, uint8_t** flags, uint32_t** consumed, uint8_t** echo, uint32_t** echo_total, uint8_t** state);
uhsdr_status uhsdr_tx_set_rtty_mod(uhsdr_tx_handle h, int32_t enable, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                   int32_t text_capacity);
uhsdr_status uhsdr_tx_set_psk_mod(uhsdr_tx_handle h, int32_t enable, int32_t speed_idx, int32_t text_capacity);
uhsdr_status uhsdr_tx_mod_put_text(uhsdr_tx_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted);
uhsdr_status uhsdr_tx_mod_start(uhsdr_tx_handle h);
uhsdr_status uhsdr_tx_mod_outputs(uhsdr_tx_handle h, uint32_t** consumed, uint32_t** txoff_at, uint8_t** state);
int32_t      uhsdr_sizeof_tx_config(void);
int32_t      uhsdr_sizeof_tx_plan(void);

/* ---- the firmware's ISR entry for one transceiver ----
 * AudioDriver_I2SCallback(audio, iq, audioDst, blockSize) (audio_driver.c:2962-3049) with the
 * firmware's own DMA half-buffers in host memory: AudioSample_t / IqSample_t = {int32 l, r}.
 * One receiver (uhsdr_rx_* with 1 channel) and optionally one transmitter (uhsdr_tx_*), both
 * with frames_per_call = block_size (32 on the firmware).
 *   RX (txrx_mode 0): iq in, codec frames out in `audio`.  The first call after TX, and while
 *       the input-mute counter runs, the firmware silences iq in place, still runs the chain
 *       and mutes the output (AudioDriver_IqFillSilence, RxProcessor external_mute :2845-2853).
 *   TX (txrx_mode 1): mic / line frames in `audio`, DAC I/Q out in `iq`, the codec sidetone in
 *       `audioDst` (zero for the voice modes, tx_processor.c:154-163, radio_management.c:450).
 *       The first call after RX runs TxProcessor_PrepareRun and, like a counted input mute,
 *       silences `audio` and skips the chain (external_mute: "do nothing", :946-949), so the I/Q
 *       out is zero and the TX state does not advance.
 * A call is synchronous: outputs are in the host buffers on return. */
/* ---- batched arm_fir_f32 (CMSIS FilteringFunctions/arm_fir_f32.c:482-560) ----
 * C channels, one shared tap set (CMSIS order, time-reversed), each channel's T-1 carried samples
 * on the device; one call == arm_fir_f32(S_c, src_c, dst_c, B) on every channel.  C5's long
 * narrow filter and the north_star's FIR-as-GEMM:
 *   UHSDR_FIR_EXACT  bit-identical to arm_fir_f32 (VALU, the reference's operation order)
 *   UHSDR_FIR_MFMA   the FIR as a GEMM on v_mfma_f32_16x16x4_f32 (fused multiply-adds in tap
 *                    order: within 1e-5 relative of the reference, not bit-identical)
 * block_size B: a multiple of 256.  src / dst: device f32 [C][B]. */
enum { UHSDR_FIR_EXACT = 0, UHSDR_FIR_MFMA = 1 };
typedef struct uhsdr_fir_s* uhsdr_fir_handle;

uhsdr_status uhsdr_fir_create(const float* coeffs, int32_t num_taps, int32_t num_channels, int32_t block_size,
                              int32_t mode, void* stream, uhsdr_fir_handle* out);
uhsdr_status uhsdr_fir_reset(uhsdr_fir_handle h);
uhsdr_status uhsdr_fir_process(uhsdr_fir_handle h, const float* src, float* dst);
uhsdr_status uhsdr_fir_synchronize(uhsdr_fir_handle h);
uhsdr_status uhsdr_fir_destroy(uhsdr_fir_handle h);
/* waves per workgroup of the FIR kernel (results do not depend on it): EXACT 1, 2 or 4 (default
 * 2); MFMA 1 .. 16 (default: as many as one workgroup's LDS holds, up to 16).
 * UHSDR_ARGUMENT_ERROR for another value, UHSDR_LENGTH_ERROR when that many windows do not fit
 * one workgroup's LDS (the setting is then unchanged). */
uhsdr_status uhsdr_fir_set_waves(uhsdr_fir_handle h, int32_t waves);
int32_t uhsdr_fir_get_waves(uhsdr_fir_handle h);

typedef struct uhsdr_i2s_s* uhsdr_i2s_handle;

uhsdr_status uhsdr_i2s_create(const uhsdr_rx_config* rx, const uhsdr_tx_config* tx /* NULL: receive only */,
                              int32_t block_size, void* stream, uhsdr_i2s_handle* out);
uhsdr_status uhsdr_i2s_set_txrx_mode(uhsdr_i2s_handle h, int32_t txrx_mode);   /* ts.txrx_mode: 0 RX, 1 TX */
uhsdr_status uhsdr_i2s_set_input_mute(uhsdr_i2s_handle h, int32_t calls);      /* ts.audio_processor_input_mute_counter */
uhsdr_status uhsdr_i2s_callback(uhsdr_i2s_handle h, int32_t* audio, int32_t* iq, int32_t* audioDst, int16_t blockSize);
uhsdr_status uhsdr_i2s_destroy(uhsdr_i2s_handle h);

/* ---- spectrum display ----
 * Replaces the no-zoom producer AudioDriver_SpectrumNoZoomProcessSamples (audio_driver.c:
 * 1811-1851: I/Q-corrected samples into an interleaved [Q, I] ring) and the consumer
 * UiSpectrum_RedrawSpectrum states 0-3 (drivers/ui/lcd/ui_spectrum.c:1350-1446): Hann window,
 * arm_cfft_f32 (CMSIS TransformFunctions/arm_cfft_f32.c:574-632), arm_cmplx_mag_f32 and the IIR
 * average clamped at 1.  Batched semantics: every fft_len consecutive input samples of a channel
 * (counted from reset) form one display frame; the firmware's main loop snapshots the ring at
 * arbitrary times, the batch takes it exactly when fft_len new samples have arrived.
 * The I/Q correction runs on the handle's own copy of the auto-correction state (it depends only
 * on the input), so a spectrum handle beside an RX handle sees what the firmware's ring sees.
 * magnify > 0 replaces the producer with the zoom one (AudioDriver_SpectrumZoomProcessSamples,
 * audio_driver.c:1860-1909): corrected I/Q, translated by iq_freq_mode (FreqShift), low-passed
 * and decimated by 2^magnify, so a display frame spans fft_len * 2^magnify input frames.
 */
#define UHSDR_SPECTRUM_MAX_LEN 1024
#define UHSDR_SPECTRUM_MAX_BITREV 1800   /* ARMBITREVINDEXTABLE1024_TABLE_LENGTH, arm_common_tables.h:96 */

typedef struct uhsdr_spectrum_config
{
    int32_t fft_len;              /* 256 (320x240), 512 (480x320 / 800x480: ui_spectrum.c:966-984) or 1024 */
    int32_t spectrum_filter;      /* ts.spectrum_filter 1..20, default 4 (ui_spectrum.h:143-145) */
    int32_t iq_auto_correction;   /* ts.iq_auto_correction, as uhsdr_rx_config */
    float   iq_gain_i, iq_gain_q; /* ts.rx_adj_gain_var.i / .q */
    float   iq_phase_balance;     /* ads.iq_phase_balance_rx */
    int32_t magnify;              /* sd.magnify 0..5: zoom 2^magnify (0: no zoom, ui_spectrum.c) */
    int32_t iq_freq_mode;         /* ts.iq_freq_mode: the translation the zoom producer sees */
    int32_t reserved[8];
} uhsdr_spectrum_config;

typedef struct uhsdr_spectrum_plan
{
    int32_t fft_len;
    int32_t window_formula;       /* 0: x *= window[i] (von_Hann_512/1024 tables, USE_PREDEFINED_WINDOW_DATA);
                                     1: x = 0.5 * ((window[i]) * x) with window = 1 - arm_cos_f32(2 pi i / (2L - 1))
                                        (ui_spectrum.c:403-406; no 2048-float table exists) */
    int32_t iq_auto_correction;
    float   iq_gain_i, iq_gain_q, iq_phase_balance;
    float   filt_factor;          /* 1 / (float)spectrum_filter (ui_spectrum.c:1434) */
    int32_t bitrev_len;           /* S->bitRevLength */
    float   window[2 * UHSDR_SPECTRUM_MAX_LEN];    /* per float of the interleaved [Q, I] frame */
    float   twiddle[2 * UHSDR_SPECTRUM_MAX_LEN];   /* twiddleCoef_<L> (arm_common_tables.c) */
    uint16_t bitrev[UHSDR_SPECTRUM_MAX_BITREV];    /* armBitRevIndexTable<L>: byte-offset swap pairs */
    uint16_t perm[UHSDR_SPECTRUM_MAX_LEN];         /* bin k of the output = butterfly result perm[k] */
    uint16_t iperm[UHSDR_SPECTRUM_MAX_LEN];        /* butterfly result p lands in bin iperm[p] */
    float   tw_lane[8][64][2];    /* the first-stage twiddles each of 64 lanes uses, laid out per lane
                                     (same values as twiddle[]; device read coalescing only) */
    /* zoom producer (AudioDriver_SpectrumZoomProcessSamples, audio_driver.c:1860-1909), magnify > 0:
       after I/Q correction and FreqShift, I and Q each through IIR_biquad_Zoom_FFT_I/_Q (4 stages,
       mag_coeffs[magnify]) and DECIMATE_ZOOM_FFT_I/_Q (FirZoomFFTDecimate[magnify]) */
    int32_t magnify;
    int32_t zoom_decimation;      /* 2^magnify */
    int32_t zoom_taps;
    int32_t freq_shift_hz, shift_kind, shift_up;   /* as uhsdr_rx_plan */
    float   osc_cos, osc_sin;
    float   zoom_biquad[20];
    float   zoom_fir[8];
    int32_t reserved[16];
} uhsdr_spectrum_plan;

typedef struct uhsdr_spectrum_s* uhsdr_spectrum_handle;

void         uhsdr_spectrum_config_default(uhsdr_spectrum_config* cfg);
uhsdr_status uhsdr_spectrum_plan_build(const uhsdr_spectrum_config* cfg, uhsdr_spectrum_plan* plan);
/* frames_per_call N: a multiple of 32 and either a multiple of fft_len (N/L display frames per
   call) or a divisor of it (one frame every L/N calls); otherwise UHSDR_LENGTH_ERROR. */
uhsdr_status uhsdr_spectrum_create(const uhsdr_spectrum_config* cfg, int32_t num_channels, int32_t frames_per_call,
                                   void* stream, uhsdr_spectrum_handle* out);
uhsdr_status uhsdr_spectrum_reset(uhsdr_spectrum_handle h);
/* iq: device IqSample_t [C][N][2] int32 (the RX input).  mag / avg: optional device f32
   [C][F][L], F = max(1, N/L): per completed frame sd.FFT_MagData and sd.FFT_AVGData (natural
   FFT bin order, as arm_cfft_f32 leaves them).  *frames (optional) = frames completed by this
   call (0 .. F); nothing is written to mag / avg when it is 0. */
uhsdr_status uhsdr_spectrum_process(uhsdr_spectrum_handle h, const int32_t* iq, float* mag, float* avg,
                                    int32_t* frames);
uhsdr_status uhsdr_spectrum_get_plan(uhsdr_spectrum_handle h, uhsdr_spectrum_plan* plan);
uhsdr_status uhsdr_spectrum_destroy(uhsdr_spectrum_handle h);
int32_t      uhsdr_sizeof_spectrum_config(void);
int32_t      uhsdr_sizeof_spectrum_plan(void);

/* CW decoder front end outputs of the following uhsdr_rx_process calls (device pointers, either
   may be NULL): signal = ads.CW_signal after every 32-frame call, uint8 [C][N/32];
   energy = the Goertzel energy of every CW block completed, f32 [C][uhsdr_rx_cw_blocks_max(h)],
   the first uhsdr_rx_cw_blocks_last(h) of them valid after a call. */
uhsdr_status uhsdr_rx_set_cw_outputs(uhsdr_rx_handle h, uint8_t* signal, float* energy);
int32_t      uhsdr_rx_cw_blocks_max(uhsdr_rx_handle h);
int32_t      uhsdr_rx_cw_blocks_last(uhsdr_rx_handle h);

/* ---- CW decoder back end: Morse to text ----
 * What CW_Decode_exe does after the mark/space decision of a block (drivers/audio/cw/cw_decoder.c:
 * 326-375 and the decoder proper, :409-1078): the state-change ring, timing initialisation, data
 * recognition, character identification, word-space and error correction, and the WPM estimate.
 * One decoder per channel, every static of the firmware's starting at zero; results are exact to
 * the reference.  blocksize 8..128 is cw_decoder_config.blocksize (samples at 12 ksps per block),
 * spikecancel 0 off / 1 spike / 2 short, text_capacity >= 8; anything else UHSDR_ARGUMENT_ERROR.
 * Outputs (owned by the handle; device pointers for a device handle, host pointers for a host one):
 *   text  uint8 [C][text_capacity], a ring: character number k of a channel is at k % text_capacity,
 *         exactly the bytes UiDriver_TextMsgPutChar receives (prosigns spelled out, '#', spaces)
 *   total uint32 [C], characters emitted since reset
 *   wpm   uint8 [C], cw_decoder_config.speed after the last block (0: not synchronised) */
typedef struct uhsdr_cwdec_s* uhsdr_cwdec_handle;

uhsdr_status uhsdr_cwdec_create(int32_t num_channels, int32_t blocksize, int32_t spikecancel, int32_t text_capacity,
                                void* stream, uhsdr_cwdec_handle* out);
/* the same decoder with its state in host memory, for uhsdr_cwdec_process_host (no device call) */
uhsdr_status uhsdr_cwdec_create_host(int32_t num_channels, int32_t blocksize, int32_t spikecancel, int32_t text_capacity,
                                     uhsdr_cwdec_handle* out);
uhsdr_status uhsdr_cwdec_reset(uhsdr_cwdec_handle h);
uhsdr_status uhsdr_cwdec_set_stream(uhsdr_cwdec_handle h, void* stream);
/* state: uint8 [C][stride], one byte per CW block (ads.CW_signal, non-zero = mark), device memory;
   decodes `blocks` <= stride blocks of every channel, stream-ordered */
uhsdr_status uhsdr_cwdec_process(uhsdr_cwdec_handle h, const uint8_t* state, int32_t blocks, int32_t stride);
/* the same step function on the CPU over host arrays, for a handle of uhsdr_cwdec_create_host */
uhsdr_status uhsdr_cwdec_process_host(uhsdr_cwdec_handle h, const uint8_t* state, int32_t blocks, int32_t stride);
uhsdr_status uhsdr_cwdec_outputs(uhsdr_cwdec_handle h, uint8_t** text, uint32_t** total, uint8_t** wpm);
uhsdr_status uhsdr_cwdec_synchronize(uhsdr_cwdec_handle h);
uhsdr_status uhsdr_cwdec_destroy(uhsdr_cwdec_handle h);
/* CwGen_CharacterIdFunc (cw_gen.c:756): the character of a code of two bits per element (10 dot,
   11 dash, first element highest); 0xfe for the empty code, 0xff when unknown */
int32_t      uhsdr_cwdec_char_id(uint32_t code);

/* Text decoding inside the RX chain: with enable != 0 the handle owns a decoder (blocksize from the
   plan) and every uhsdr_rx_process decodes the CW blocks that call completed, after its back end.
   Only for plan.cw_enabled with dmod_mode CW, where the firmware decodes (cw_decoder.c:355);
   otherwise UHSDR_ARGUMENT_ERROR.  uhsdr_rx_reset resets the decoder.  Outputs as above. */
uhsdr_status uhsdr_rx_set_cw_text(uhsdr_rx_handle h, int32_t enable, int32_t spikecancel, int32_t text_capacity);
uhsdr_status uhsdr_rx_cw_text_outputs(uhsdr_rx_handle h, uint8_t** text, uint32_t** total, uint8_t** wpm);

/* ---- RTTY decoder: Baudot to text, one decoder per channel ----
 * What the firmware runs on every 12 ksps sample in DEMOD_DIGI with digital_mode RTTY
 * (Rtty_Demodulator_ProcessSample, drivers/audio/rtty.c): mark and space band-passes, the
 * automatic threshold correction (or the plain difference with atc_disable), the low-pass, the bit
 * DPLL, the start-bit search, Baudot framing and the letters / figures tables.  Exact to the
 * reference: the same bytes at the same samples.
 *   shift_idx    0 .. 5: 85, 170, 200, 425, 450, 850 Hz (mark 915 Hz, space 915 Hz + shift)
 *   speed_idx    0 .. 1: 45.45 and 50 baud (264 and 240 samples per bit)
 *   stopbits_idx 0 .. 2: 1, 1.5 and 2 stop bits
 *   text_capacity >= 8
 * Outputs (device memory, or host memory for a host handle), valid once the work enqueued is complete:
 *   text  uint8 [C][text_capacity], a ring: character k of a channel is at k % text_capacity;
 *         exactly the bytes UiDriver_TextMsgPutChar receives, '\0', '\a', '\r' and '\n' included
 *         (LTRS and FIGS only switch the table)
 *   total uint32 [C], characters emitted since reset
 * The RTTY modulator (Rtty_Modulator_GenSample) is uhsdr_rttymod_* below.
 * Not built: text decoding of any kind in the uhsdr_i2s_* stream. */
typedef struct uhsdr_rtty_s* uhsdr_rtty_handle;

uhsdr_status uhsdr_rtty_create(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                               int32_t atc_disable, int32_t text_capacity, void* stream, uhsdr_rtty_handle* out);
/* the same decoder with its state in host memory, for uhsdr_rtty_process_host (no device call) */
uhsdr_status uhsdr_rtty_create_host(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                    int32_t atc_disable, int32_t text_capacity, uhsdr_rtty_handle* out);
uhsdr_status uhsdr_rtty_reset(uhsdr_rtty_handle h);
uhsdr_status uhsdr_rtty_set_stream(uhsdr_rtty_handle h, void* stream);
/* samples: f32 [C][stride], 12 ksps, device memory; decodes n <= stride samples of every channel,
   stream-ordered */
uhsdr_status uhsdr_rtty_process(uhsdr_rtty_handle h, const float* samples, int32_t n, int32_t stride);
/* the same step function on the CPU over host arrays, for a handle of uhsdr_rtty_create_host */
uhsdr_status uhsdr_rtty_process_host(uhsdr_rtty_handle h, const float* samples, int32_t n, int32_t stride);
uhsdr_status uhsdr_rtty_outputs(uhsdr_rtty_handle h, uint8_t** text, uint32_t** total);
uhsdr_status uhsdr_rtty_synchronize(uhsdr_rtty_handle h);
uhsdr_status uhsdr_rtty_destroy(uhsdr_rtty_handle h);

/* ---- BPSK decoder: varicode to text, one decoder per channel ----
 * What the firmware runs on every 12 ksps sample in DEMOD_DIGI with digital_mode BPSK
 * (Psk_Demodulator_ProcessSample, drivers/audio/psk.c): the band-pass around the 500 Hz carrier,
 * the mixer and its running sum over one carrier period, the bit decision per symbol and varicode
 * framing.  Like the firmware it has no carrier or timing recovery.  Exact to the reference: the
 * same bytes at the same samples.
 *   speed_idx    0 .. 2: BPSK31, BPSK63, BPSK125
 *   text_capacity >= 8
 * Outputs (device memory, or host memory for a host handle), valid once the work enqueued is complete:
 *   text   uint8 [C][text_capacity], a ring: character k of a channel is at k % text_capacity;
 *          exactly the bytes UiDriver_TextMsgPutChar receives, '*' for a code that is no character
 *   total  uint32 [C], characters emitted since reset
 *   symbol float [C], rx_last_symbol: the averaged phase at the last bit decision, the firmware's
 *          tuning quantity
 * The modulator (Psk_Modulator_GenSample) is uhsdr_pskmod_* below.
 * Not built: QPSK. */
typedef struct uhsdr_psk_s* uhsdr_psk_handle;

uhsdr_status uhsdr_psk_create(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, void* stream, uhsdr_psk_handle* out);
/* the same decoder with its state in host memory, for uhsdr_psk_process_host (no device call) */
uhsdr_status uhsdr_psk_create_host(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, uhsdr_psk_handle* out);
uhsdr_status uhsdr_psk_reset(uhsdr_psk_handle h);
uhsdr_status uhsdr_psk_set_stream(uhsdr_psk_handle h, void* stream);
/* samples: f32 [C][stride], 12 ksps, device memory; decodes n <= stride samples of every channel,
   stream-ordered */
uhsdr_status uhsdr_psk_process(uhsdr_psk_handle h, const float* samples, int32_t n, int32_t stride);
/* the same step function on the CPU over host arrays, for a handle of uhsdr_psk_create_host */
uhsdr_status uhsdr_psk_process_host(uhsdr_psk_handle h, const float* samples, int32_t n, int32_t stride);
uhsdr_status uhsdr_psk_outputs(uhsdr_psk_handle h, uint8_t** text, uint32_t** total, float** symbol);
uhsdr_status uhsdr_psk_synchronize(uhsdr_psk_handle h);
uhsdr_status uhsdr_psk_destroy(uhsdr_psk_handle h);

/* ---- RTTY and BPSK modulators: text to 48 ksps audio, one modulator per channel ----
 * What the firmware's transmit path generates per sample in DEMOD_DIGI: Rtty_Modulator_GenSample
 * (drivers/audio/rtty.c: Baudot framing with LTRS / FIGS only at a change of set, idle LTRS, two
 * softdds tones with the phase-continuous change between them) and Psk_Modulator_GenSample
 * (drivers/audio/psk.c: preamble, varicode, the raised envelope at phase reversals, postamble after
 * EOT).  Exact to the reference: the same int16 at every sample.  Pure integer arithmetic.
 *   rttymod: shift_idx, speed_idx, stopbits_idx as uhsdr_rtty_create (space = 915 Hz + shift, mark =
 *            915 Hz; 1.5 and 2 stop bits both send two)
 *   pskmod:  speed_idx as uhsdr_psk_create
 *   text_capacity >= 8: the size of a channel's text queue, which models the firmware's ring
 *            (uhsdr_digi_buffer.c).  One slot stays free: text_capacity - 1 characters fit.
 * create and reset leave a modulator as a fresh firmware leaves it after the modem's init and
 * Rtty_Modulator_StartTX / Psk_Modulator_PrepareTx, with an empty queue: RTTY idles on LTRS, BPSK
 * starts its preamble.  start_tx / prepare_tx are these two calls alone, on every channel,
 * stream-ordered; they keep the queue and what the firmware's calls keep.
 * put_text: text = host uint8 [C][stride], len = host int32 [C] with 0 <= len[c] <= stride.  Appends to
 * every channel's queue what fits of its len[c] bytes and reports that count in accepted [C] (host,
 * may be null).  It is ordered after the work already enqueued: on a device handle it synchronises
 * the handle's stream to learn how much each modulator has taken, and returns with the text in place.
 * Byte 0x04 (EOT) requests TX-off: RTTY in the sample that takes it, going on with the text behind
 * it; BPSK after its postamble, where the modulator turns OFF and stays silent until prepare_tx.
 * process: audio = int16 [C][stride], device memory (host memory for process_host); writes n <= stride
 * samples of every channel, stream-ordered.
 * Outputs (device memory, or host memory for a host handle), valid once the work enqueued is complete:
 *   consumed uint32 [C], characters taken from the queue since reset (what the firmware echoes to
 *            UiDriver_TextMsgPutChar)
 *   txoff_at uint32 [C], the index since reset of the first sample in which the channel requested
 *            TX-off (RadioManagement_Request_TxOff), 0xffffffff if none.  The index is 32 bits wide:
 *            it wraps after 2^32 samples, 24.9 hours at 48 ksps, and a request in sample
 *            0xffffffff reads as none; reset before that where txoff_at matters
 *   state    uint8 [C], BPSK: 0 OFF, 1 PREAMBLE, 2 ACTIVE, 3 POSTAMBLE, 4 INACTIVE; RTTY: 0
 * set_stream waits for the work enqueued on the stream the handle held, so the new stream's work
 * and put_text are ordered after it.
 * Inside the transmit chain (TxProcessor_Rtty / TxProcessor_Psk): uhsdr_tx_set_rtty_mod /
 * uhsdr_tx_set_psk_mod above.
 * Not built: a QPSK modulator (the firmware has none), the firmware's consumer tag on the ring, the
 * CW generator / keyer as a text source (the keyer itself is uhsdr_cwgen_* below), FreeDV. */
typedef struct uhsdr_rttymod_s* uhsdr_rttymod_handle;
typedef struct uhsdr_pskmod_s* uhsdr_pskmod_handle;

uhsdr_status uhsdr_rttymod_create(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                  int32_t text_capacity, void* stream, uhsdr_rttymod_handle* out);
/* the same modulator with its state in host memory, for uhsdr_rttymod_process_host (no device call) */
uhsdr_status uhsdr_rttymod_create_host(int32_t num_channels, int32_t shift_idx, int32_t speed_idx, int32_t stopbits_idx,
                                       int32_t text_capacity, uhsdr_rttymod_handle* out);
uhsdr_status uhsdr_rttymod_reset(uhsdr_rttymod_handle h);
uhsdr_status uhsdr_rttymod_start_tx(uhsdr_rttymod_handle h);
uhsdr_status uhsdr_rttymod_put_text(uhsdr_rttymod_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted);
uhsdr_status uhsdr_rttymod_process(uhsdr_rttymod_handle h, int16_t* audio, int32_t n, int32_t stride);
uhsdr_status uhsdr_rttymod_process_host(uhsdr_rttymod_handle h, int16_t* audio, int32_t n, int32_t stride);
uhsdr_status uhsdr_rttymod_outputs(uhsdr_rttymod_handle h, uint32_t** consumed, uint32_t** txoff_at, uint8_t** state);
uhsdr_status uhsdr_rttymod_set_stream(uhsdr_rttymod_handle h, void* stream);
uhsdr_status uhsdr_rttymod_synchronize(uhsdr_rttymod_handle h);
uhsdr_status uhsdr_rttymod_destroy(uhsdr_rttymod_handle h);

uhsdr_status uhsdr_pskmod_create(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, void* stream, uhsdr_pskmod_handle* out);
uhsdr_status uhsdr_pskmod_create_host(int32_t num_channels, int32_t speed_idx, int32_t text_capacity, uhsdr_pskmod_handle* out);
uhsdr_status uhsdr_pskmod_reset(uhsdr_pskmod_handle h);
uhsdr_status uhsdr_pskmod_prepare_tx(uhsdr_pskmod_handle h);
uhsdr_status uhsdr_pskmod_put_text(uhsdr_pskmod_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted);
uhsdr_status uhsdr_pskmod_process(uhsdr_pskmod_handle h, int16_t* audio, int32_t n, int32_t stride);
uhsdr_status uhsdr_pskmod_process_host(uhsdr_pskmod_handle h, int16_t* audio, int32_t n, int32_t stride);
uhsdr_status uhsdr_pskmod_outputs(uhsdr_pskmod_handle h, uint32_t** consumed, uint32_t** txoff_at, uint8_t** state);
uhsdr_status uhsdr_pskmod_set_stream(uhsdr_pskmod_handle h, void* stream);
uhsdr_status uhsdr_pskmod_synchronize(uhsdr_pskmod_handle h);
uhsdr_status uhsdr_pskmod_destroy(uhsdr_pskmod_handle h);

/* ---- CW generator: key lines and text to 48 ksps I/Q, one keyer per channel ----
 * What the firmware's CwGen_Process (drivers/audio/cw/cw_gen.c) produces per 32-sample block: the
 * straight key or the iambic A / B / Ultimatic keyer, the softdds tone while an element is keyed,
 * the key-click envelope on both edges, text from the queue keyed as Morse, and the characters the
 * keyer recognises printed to an echo ring.  Exact to the reference: the same binary32 I and Q at
 * every sample, the same state after every block.  Integer arithmetic except the envelope product.
 * The settings are handle-wide, as the firmware's are one set per transceiver:
 *   keyer_mode 0 IAM_B, 1 IAM_A, 2 STRAIGHT, 3 ULTIMATE; keyer_speed 5 .. 48 wpm; keyer_weight
 *   50 .. 150; paddle_reverse; rx_delay 0 .. 50 (the break time is rx_delay * 50 + 1 blocks);
 *   sidetone_freq 400 .. 1000 Hz
 *   text_capacity >= 8: a channel's text queue, as the modulators' (one slot stays free)
 *   echo_capacity >= 8: a channel's echo ring
 * The firmware's surroundings are fixed: the transmitter is in TX in DEMOD_CW throughout, no text
 * entry, no CAT keying, the text ring's consumer is CW.  create and reset leave every channel as
 * CwGen_Init leaves a fresh keyer there (idle, all timers 0), the tone's phase at 0, the queue and the
 * echo empty.  set_speed is CwGen_SetSpeed with a new speed and weight; it takes effect with the next
 * process call, also in the middle of a character.  put_text as uhsdr_rttymod_put_text.
 * process: keys = uint8 [C][n/32], one byte per block, bit 0 the DIT line and bit 1 the DAH/PTT line,
 * constant over the block; i, q = f32 [C][stride]; n a multiple of 32, n <= stride; device memory
 * (host memory for process_host), stream-ordered.  In the block where a line closes (0 -> 1 against
 * the block before, across calls; after reset both are open) the effects of the firmware's key
 * interrupt run first: the text queue is emptied, the character being sent is dropped, and the
 * Ultimatic keyer notes which paddle came first.  i and q are CwGen_Process' buffers (I the sine, Q
 * the cosine); in a block where it returns false they are written as zeros, which is what the
 * transmit chain sends then.
 * Outputs (device memory, or host memory for a host handle), valid once the work enqueued is complete:
 *   flags      uint8 [C][n/32] of the last call: bit 0 CwGen_Process returned true, bit 1
 *              RadioManagement_Request_TxOn and bit 2 RadioManagement_Request_TxOff was called in the
 *              block.  The buffer grows with the largest call: ask again after a larger one
 *   consumed   uint32 [C], characters taken from the queue since reset, those a key closure
 *              discarded included
 *   echo       uint8 [C][echo_capacity], echo_total uint32 [C]: the bytes the firmware hands to
 *              UiDriver_TextMsgPutChar (a character, the four bytes "<XX>" of a prosign, '*' for an
 *              unknown code, the word space), byte k at k % echo_capacity
 *   state      uint8 [C], ps.cw_state (0 IDLE, 1 DIT_CHECK, 3 DAH_CHECK, 4 KEY_DOWN, 5 KEY_UP, 6 PAUSE,
 *              7 WAIT); in STRAIGHT mode ps.key_timer (3 rising, 2 on, 1 falling, 0 off)
 * peek: the keyer's words, uint32 [rows][C] (port_state, cw_state, key_timer, break_timer,
 * space_timer, sm_tbl_ptr, ultim, cw_char, sending_char, the DDS accumulator, the key lines of the
 * block before), for tests and diagnosis only: the rows and their order are not part of the
 * interface and may change with any version; ask for `rows` and do not store the layout.
 * Reference oddities kept: a character without a code is taken from the queue and dropped; cw_char
 * wraps at 32 bits and anything above 50000 prints '*'; the straight key ignores paddle_reverse; the
 * tone's phase is never reset by the keyer.
 * Inside the transmit chain (TxProcessor_CW): uhsdr_tx_set_cw_keyer above.
 * Not built: the keyer as text entry for RTTY / BPSK, CAT keying, the OVI40 sidetone, the
 * RX-mode call of CwGen_Process, any PTT sequencing (the TX-on / TX-off requests are outputs). */
typedef struct
{
    int32_t keyer_mode, keyer_speed, keyer_weight, paddle_reverse, rx_delay, sidetone_freq;
} uhsdr_cwgen_config;
#define UHSDR_CW_KEYER_IAM_B    0
#define UHSDR_CW_KEYER_IAM_A    1
#define UHSDR_CW_KEYER_STRAIGHT 2
#define UHSDR_CW_KEYER_ULTIMATE 3

uhsdr_status uhsdr_cwgen_create(int32_t num_channels, const uhsdr_cwgen_config* cfg, int32_t text_capacity, int32_t echo_capacity,
                                void* stream, uhsdr_cwgen_handle* out);
/* the same generator with its state in host memory, for uhsdr_cwgen_process_host (no device call) */
uhsdr_status uhsdr_cwgen_create_host(int32_t num_channels, const uhsdr_cwgen_config* cfg, int32_t text_capacity, int32_t echo_capacity,
                                     uhsdr_cwgen_handle* out);
uhsdr_status uhsdr_cwgen_reset(uhsdr_cwgen_handle h);
uhsdr_status uhsdr_cwgen_set_speed(uhsdr_cwgen_handle h, int32_t speed, int32_t weight);
uhsdr_status uhsdr_cwgen_put_text(uhsdr_cwgen_handle h, const uint8_t* text, const int32_t* len, int32_t stride, int32_t* accepted);
uhsdr_status uhsdr_cwgen_process(uhsdr_cwgen_handle h, const uint8_t* keys, float* i, float* q, int32_t n, int32_t stride);
uhsdr_status uhsdr_cwgen_process_host(uhsdr_cwgen_handle h, const uint8_t* keys, float* i, float* q, int32_t n, int32_t stride);
uhsdr_status uhsdr_cwgen_outputs(uhsdr_cwgen_handle h, uint8_t** flags, uint32_t** consumed, uint8_t** echo, uint32_t** echo_total, uint8_t** state);
uhsdr_status uhsdr_cwgen_peek(uhsdr_cwgen_handle h, uint32_t** words, int32_t* rows);
uhsdr_status uhsdr_cwgen_set_stream(uhsdr_cwgen_handle h, void* stream);
uhsdr_status uhsdr_cwgen_synchronize(uhsdr_cwgen_handle h);
uhsdr_status uhsdr_cwgen_destroy(uhsdr_cwgen_handle h);

/* ---- Spectral noise reduction: 12 / 6 ksps audio in, the same audio with the noise reduced ----
 * The firmware's spectral_noise_reduction_3 (drivers/audio/audio_nr.c:1841-2195), one instance per
 * channel: half-overlapping 256-sample frames under a square-root Hann window, arm_cfft_f32, an MMSE
 * noise estimate with a speech-presence probability, the Ephraim-Malah gain inside the filter's
 * pass band, a smoothing of the gains over NN bins against musical noise, the inverse transform,
 * the window again and overlap-add.  Exact to the reference: the same binary32 output at every
 * sample and the same NN in every frame, with the double-precision intermediates where the C
 * promotes to double.  The settings are handle-wide, as ts and nr_params are one per transceiver:
 *   alpha                 nr_params.alpha, 0 .. 1 (uhsdr_nr_alpha_from_strength: the firmware's
 *                         0.799 + nr_strength / 1000.0)
 *   asnr                  NR2.asnr 2 .. 30 dB, default 30
 *   width                 NR2.width 1 .. 5, default 4: NN is at most 1 + 2 * width
 *   power_threshold_int   NR2.power_threshold_int 10 .. 100, default 40
 *   width_hz, offset_hz   FilterInfo[ts.filters_p->id].width and ts.filters_p->offset, 0 .. 65535:
 *                         the pass band whose bins [VAD_low, VAD_high) are weighted
 *   sample_rate           6000 (nr_params.NR_decimation_active) or 12000, the rate of the frames;
 *                         uhsdr_nr_process decides it as the firmware does and ignores this field
 * create and reset leave every channel as a fresh noise reduction (every static zero, first_time 1):
 * the first 20 frames pass unchanged while the noise floor is averaged.
 * process_frames: in, out = f32 [C][stride], `frames` frames of 128 samples each per row, frames *
 * 128 <= stride, device memory (host memory for process_frames_host), stream-ordered; in and out
 * must not overlap.  A frame's output is the overlap-add of its first half with the frame before,
 * so it lags the input by 128 samples.
 * process: the 12 ksps stream around it, AudioDriver_RxProcessorNoiseReduction (audio_driver.c:
 * 2328-2434): below a filter width of 2701 Hz the 4-tap 2:1 decimator in front and the 40-tap 1:2
 * interpolator with the factor 2.0 behind; 128-sample frames are collected, and their results come
 * out after the output FIFO's latency of two frames (silence until then).  The firmware runs the
 * frame stage in its main loop; here that loop never falls behind (AudioNr_HandleNoiseReduction
 * after every block).  n: samples per row, a multiple of 8 (the firmware's block of 32 codec frames
 * at 12 ksps), n <= stride; anything else is UHSDR_LENGTH_ERROR.  in and out must not overlap here
 * either: the input is read again after the output is written.  A handle is used either through
 * process_frames or through process from a reset on.
 * state: per channel, into host arrays of num_channels (null: not wanted), after everything
 * enqueued: first_time (1 fresh, 2 averaging, 3 running), NN of the last frame and its power_ratio.
 * Reference oddities kept: the upper half is weighted at bin 255 - b, not 256 - b; the smoothing's
 * upper-edge loop overwrites part of the middle loop's result; a negative lower band edge wraps
 * through uint8_t to VAD_low 126, an empty band in which nothing is weighted; a restart keeps no
 * state here, while the firmware keeps its last overlap half.  The smoothing loops index relative to
 * the band and leave the firmware's arrays for a narrow or extreme one: a configuration is refused
 * with UHSDR_ARGUMENT_ERROR unless, for M = 1 + 2 * width, VAD_high >= 2 M - 1 and VAD_low + M / 2
 * + M - 2 <= 127 (width 4: VAD_high >= 17, VAD_low <= 116), or the band is empty.  A frame whose
 * band holds no power has a NaN power_ratio, which the C converts to int (undefined); here that
 * frame has NN = 1.
 * The noise blanker in front (uhsdr_nb_* below has the blanker itself): AudioNr_RunNoiseReduction runs
 * alt_noise_blanking on every collected frame, in place, before spectral_noise_reduction_3, and the
 * firmware offers NR alone, NB alone and NB followed by NR.
 *   nb_setting            0 (default): no blanker; 1 .. 15: ts.dsp.nb_setting, the blanker runs on
 *                         every frame before the noise reduction, as a launch of its own
 *   nr_bypass             0 (default); 1: the firmware's NB-only setting, the frame is copied
 *                         through behind the blanker and no noise reduction state moves.  With
 *                         nb_setting 0 it is refused (UHSDR_ARGUMENT_ERROR): the firmware does not
 *                         enter the stream at all then
 * process, process_host, process_frames and process_frames_host honour both; reset clears the
 * blanker too; with both 0 every call enqueues exactly what it enqueued before they existed.  With
 * the blanker on, a frame's output lags by 13 samples more.
 * Inside the RX chain: uhsdr_rx_set_nr, at the end of this header.
 * Not built: the LMS noise reduction, the #if 0 notch code. */
typedef struct uhsdr_nr_config
{
    float   alpha;
    int32_t asnr, width, power_threshold_int;
    int32_t width_hz, offset_hz;
    int32_t sample_rate;
    int32_t nb_setting, nr_bypass;
    int32_t reserved[7];
} uhsdr_nr_config;
typedef struct uhsdr_nr_s* uhsdr_nr_handle;

void         uhsdr_nr_config_default(uhsdr_nr_config* cfg);
float        uhsdr_nr_alpha_from_strength(int32_t nr_strength);
/* VAD_low and VAD_high of a configuration, or the status uhsdr_nr_create would give */
uhsdr_status uhsdr_nr_band(const uhsdr_nr_config* cfg, int32_t* vad_low, int32_t* vad_high);
uhsdr_status uhsdr_nr_create(int32_t num_channels, const uhsdr_nr_config* cfg, void* stream, uhsdr_nr_handle* out);
/* the same noise reduction with its state in host memory, for the _host calls (no device call) */
uhsdr_status uhsdr_nr_create_host(int32_t num_channels, const uhsdr_nr_config* cfg, uhsdr_nr_handle* out);
uhsdr_status uhsdr_nr_reset(uhsdr_nr_handle h);
uhsdr_status uhsdr_nr_set_stream(uhsdr_nr_handle h, void* stream);
uhsdr_status uhsdr_nr_process_frames(uhsdr_nr_handle h, const float* in, float* out, int32_t frames, int32_t stride);
uhsdr_status uhsdr_nr_process_frames_host(uhsdr_nr_handle h, const float* in, float* out, int32_t frames, int32_t stride);
uhsdr_status uhsdr_nr_process(uhsdr_nr_handle h, const float* in, float* out, int32_t n, int32_t stride);
uhsdr_status uhsdr_nr_process_host(uhsdr_nr_handle h, const float* in, float* out, int32_t n, int32_t stride);
uhsdr_status uhsdr_nr_state(uhsdr_nr_handle h, int32_t* first_time, int32_t* nn, float* power_ratio);
uhsdr_status uhsdr_nr_synchronize(uhsdr_nr_handle h);
uhsdr_status uhsdr_nr_destroy(uhsdr_nr_handle h);
/* For tests and diagnosis only, not for the signal path (it builds its tables on every call):
   arm_cfft_f32(&arm_cfft_sR_f32_len256, x, inverse, 1) on 256 interleaved complex values in host
   memory, the transform of the host twin (tests/test_icfft_host.py pins it against the reference) */
uhsdr_status uhsdr_nr_cfft256_host(float* x, int32_t inverse);

/* Digital-mode tap of the RX chain: tap = device f32 [C][N/4], written by every following
   uhsdr_rx_process with a_buffer[0] after biquad_1, the sample the firmware hands its modems
   (audio_driver.c:2537-2557); null turns it off.  Available where the firmware runs them: a 12 ksps
   path of the SSB / CW / DIGI back-end family (mono), in every schedule; anything else gives
   UHSDR_ARGUMENT_ERROR.  Launches with a tap run kernel instances of their own; with the tap on,
   pipelined mode 3 (the persistent back end) runs as mode 2, as it does with the CW front end. */
uhsdr_status uhsdr_rx_set_digi_tap(uhsdr_rx_handle h, float* tap);
/* RTTY text inside the RX chain: with enable != 0 the handle owns a decoder (arguments as
   uhsdr_rtty_create) and a tap row, unless the caller set one, and every uhsdr_rx_process decodes the
   call's N/4 samples after the kernel that wrote them, on its stream.  Only for dmod_mode
   UHSDR_DEMOD_DIGI on a path that has the tap; otherwise UHSDR_ARGUMENT_ERROR.  uhsdr_rx_reset
   resets the decoder.  Outputs as uhsdr_rtty_outputs. */
uhsdr_status uhsdr_rx_set_rtty_text(uhsdr_rx_handle h, int32_t enable, int32_t shift_idx, int32_t speed_idx,
                                    int32_t stopbits_idx, int32_t atc_disable, int32_t text_capacity);
uhsdr_status uhsdr_rx_rtty_text_outputs(uhsdr_rx_handle h, uint8_t** text, uint32_t** total);
/* BPSK text inside the RX chain, as uhsdr_rx_set_rtty_text (arguments as uhsdr_psk_create, outputs
   as uhsdr_psk_outputs).  The firmware's digital_mode is one value: enabling BPSK text while RTTY
   text is on, or RTTY text while BPSK text is on, is UHSDR_ARGUMENT_ERROR; turn the other off first. */
uhsdr_status uhsdr_rx_set_psk_text(uhsdr_rx_handle h, int32_t enable, int32_t speed_idx, int32_t text_capacity);
uhsdr_status uhsdr_rx_psk_text_outputs(uhsdr_rx_handle h, uint8_t** text, uint32_t** total, float** symbol);

/* Key beep (AudioManagement_KeyBeep, audio_management.c:368-375 -> the softdds tone added to the
   output at audio_driver.c:2891-2898): the beep's DDS accumulator restarts at 0 and the tone
   (config beep_frequency / beep_loudness) is added to every channel's output for the next
   `calls` 32-frame calls (the firmware's ts.beep_timing countdown, here counted in ISR calls);
   0 stops a running beep.  Like the firmware's single key beep, it is common to all channels. */
uhsdr_status uhsdr_rx_key_beep(uhsdr_rx_handle h, int32_t calls);

/* ---- diagnostics ---- */
const char*  uhsdr_version(void);
/* UHSDR_ABI_VERSION the library was built with: a binding compares it with the header it mirrors
   (a stale library would otherwise ignore config words it does not know) */
int32_t      uhsdr_abi_version(void);
/* sizeof(uhsdr_rx_config), sizeof(uhsdr_rx_plan): lets FFI bindings check their layouts */
int32_t      uhsdr_sizeof_config(void);
int32_t      uhsdr_sizeof_plan(void);
const char*  uhsdr_last_error(void);
/* number of kernel slots uhsdr_rx_kernel_times reports: rx_front, rx_back (any back-end kernel),
   rx_chain; a call enqueues rx_front + rx_back, or rx_chain alone */
int32_t      uhsdr_rx_kernel_count(uhsdr_rx_handle h);
/* Per-kernel device timing: while enabled (enable = k > 0), every k-th uhsdr_rx_process call
   (the 1st, (k+1)-th, ...) brackets each kernel with hipEvents on the stream it runs on; k = 1
   times every call.  Sampling keeps the event records' own host and device cost (~30 us per
   bracketed call) out of a throughput measurement.  uhsdr_rx_kernel_times() synchronises and
   returns, per kernel, the summed milliseconds and launch count of the timed calls since the
   last enable. */
uhsdr_status uhsdr_rx_enable_timing(uhsdr_rx_handle h, int32_t enable);
int32_t      uhsdr_rx_kernel_times(uhsdr_rx_handle h, float* total_ms, int32_t* launches, int32_t max_kernels);
const char*  uhsdr_rx_kernel_name(int32_t index);

/* ---- Noise blanker: 12 / 6 ksps audio in, the same audio with impulses repaired ----
 * The firmware's alt_noise_blanking (drivers/audio/audio_nr.c:2210-2535), one instance per channel,
 * on the 128-sample frames of the noise reduction: an order-10 LPC analysis of the frame
 * (autocorrelation, Levinson-Durbin), the inverse filter and its matched filter, a threshold of
 * (16 - nb_setting) * 0.5 * sqrt(variance * power of the coefficients) on the result, and up to five
 * places per frame where seven samples are replaced by the weighted forward and backward
 * predictions.  Exact to the reference: the same binary32 output at every sample.
 *   nb_setting   ts.dsp.nb_setting, 1 .. 15 (MAX_NB_SETTING), default 8; a higher setting lowers
 *                the threshold.  The firmware's 0 means off; anything outside 1 .. 15 is
 *                UHSDR_ARGUMENT_ERROR
 * process_frames: in, out = f32 [C][stride], `frames` frames of 128 samples each per row, frames *
 * 128 <= stride, device memory (host memory for process_frames_host), stream-ordered.  in == out is
 * allowed, the firmware works in place; any other overlap is the caller's error.  The blanker keeps
 * the last 26 samples, so a frame's output lags the input by 13 samples.
 * state: per channel, into host arrays of num_channels (null: not wanted), after everything
 * enqueued: the places repaired in the last frame (0 .. 5) and since the last reset.  The
 * firmware keeps the count in a local; this is the activity a host would show.
 * Reference oddities kept: nothing is clamped; a silent frame, or one whose autocorrelation
 * overflows, has a NaN threshold, nothing compares above it and the samples pass; the search skips
 * the filtered samples 0 .. 12 and a repair lies 10 samples before its hit.  create and reset start
 * from a cleared working buffer, while the firmware never clears its static, not even when the noise
 * reduction restarts (as with the NR's overlap half above).
 * Inside the RX chain: uhsdr_rx_set_nr below.
 * Not built: the old time-domain blanker of audio_driver.c:1278, the blanker in uhsdr_i2s_*. */
typedef struct uhsdr_nb_config
{
    int32_t nb_setting;
    int32_t reserved[7];
} uhsdr_nb_config;
typedef struct uhsdr_nb_s* uhsdr_nb_handle;

void         uhsdr_nb_config_default(uhsdr_nb_config* cfg);
uhsdr_status uhsdr_nb_create(int32_t num_channels, const uhsdr_nb_config* cfg, void* stream, uhsdr_nb_handle* out);
/* the same blanker with its state in host memory, for the _host call (no device call) */
uhsdr_status uhsdr_nb_create_host(int32_t num_channels, const uhsdr_nb_config* cfg, uhsdr_nb_handle* out);
uhsdr_status uhsdr_nb_reset(uhsdr_nb_handle h);
uhsdr_status uhsdr_nb_set_stream(uhsdr_nb_handle h, void* stream);
uhsdr_status uhsdr_nb_process_frames(uhsdr_nb_handle h, const float* in, float* out, int32_t frames, int32_t stride);
uhsdr_status uhsdr_nb_process_frames_host(uhsdr_nb_handle h, const float* in, float* out, int32_t frames, int32_t stride);
uhsdr_status uhsdr_nb_state(uhsdr_nb_handle h, int32_t* last_count, uint32_t* total_count);
uhsdr_status uhsdr_nb_synchronize(uhsdr_nb_handle h);
uhsdr_status uhsdr_nb_destroy(uhsdr_nb_handle h);

/* ---- Noise reduction and blanker inside the RX chain ----
 * The firmware runs both on a_buffer[0] between the AGC and the post-AGC scale whenever the
 * decimated rate is 12 ksps and DSP NR or the blanker is on (RxProcessor_DemodAudioPostprocessing,
 * audio_driver.c:2501-2510), so biquad_1, the modems, the CW front end, the interpolator and the
 * anti-alias lattice see the noise-reduced sample.
 * set_nr: cfg non-null turns the stage on with a fresh noise reduction and blanker (as
 * uhsdr_nr_create / uhsdr_nr_reset), owned by the handle; null turns it off and frees it.  cfg is
 * uhsdr_nr_config as above: nb_setting and nr_bypass select NR alone (0, 0), NB then NR (1 .. 15, 0)
 * and NB alone (1 .. 15, 1); width_hz and offset_hz state FilterInfo[ts.filters_p->id].width and
 * ts.filters_p->offset; sample_rate is ignored, as in uhsdr_nr_process (below 2701 Hz the frames run
 * at 6 ksps).  Every refusal of uhsdr_nr_create is passed on before anything changes, the band judged
 * at the rate the stream runs.  With the stage on, a call enqueues on the handle's stream: the
 * front, rx_notch where the plan has one, a head kernel (pre-filter lattice, AGC) that writes
 * a_buffer[0] to a [C][N/4] row of the handle, uhsdr_nr_process from that row to a second one, a tail
 * kernel (scale, biquad_1, CW front end, digital-mode tap, interpolator, anti-alias lattice, biquad_2,
 * the board's output stage), then the text decoders.  With it off, a call enqueues exactly what it
 * enqueued before the stage existed.  The main loop never falls behind, as in uhsdr_nr_process.
 * Accepted: a 12 ksps path of the SSB / CW / DIGI back-end family, mono, no DC removal in the AGC,
 * either board, with or without codec frames, key beep, LMS auto notch, CW front end and CW text,
 * digital-mode tap, RTTY or BPSK text.  UHSDR_ARGUMENT_ERROR: 24 ksps, AM / SAM, FM and stereo paths,
 * UHSDR_SCHEDULE_CHAIN, any pipelined mode, FMA precision; and while the stage is on,
 * uhsdr_rx_set_pipelined(1 .. 3), uhsdr_rx_set_schedule(CHAIN) and uhsdr_rx_set_precision(FMA).
 * uhsdr_rx_reset resets the stage, uhsdr_rx_destroy frees it, uhsdr_rx_set_stream moves it.
 * With the stage on, a caller's row for uhsdr_rx_set_digi_tap must be 16-byte aligned, like the audio
 * rows (the tail kernel stores it in 16-byte pieces); a row that is not gives UHSDR_ARGUMENT_ERROR from
 * whichever of the two calls comes second.
 * nr_state: per channel into host arrays of num_channels (null: not wanted), after everything
 * enqueued: uhsdr_nr_state's three, and uhsdr_nb_state's two (zero with the blanker off).
 * Not built: the stage in the wave pipeline's pipelined modes, the persistent back end or rx_chain,
 * on AM / SAM, 24 ksps or stereo paths, in uhsdr_i2s_*, the leaky-LMS noise reduction, a main loop
 * that falls behind. */
uhsdr_status uhsdr_rx_set_nr(uhsdr_rx_handle h, const uhsdr_nr_config* cfg);
uhsdr_status uhsdr_rx_nr_state(uhsdr_rx_handle h, int32_t* first_time, int32_t* nn, float* power_ratio, int32_t* nb_last,
                               uint32_t* nb_total);

/* ---- Signal meter: display frames of sd.FFT_MagData in, dBm, dBm/Hz, S-units and SNAP carrier out ----
 * What the firmware's front panel shows of a channel's strength and tuning, one instance per channel,
 * once per completed display frame and in this order: UiSpectrum_CalculateDBm with
 * UiSpectrum_CalculateSnap (drivers/ui/lcd/ui_spectrum.c:1876-2123), the attack / decay averagers of
 * RadioManagement_HandleIqGainAndSMeter and the S-unit search of UiDriver_HandleSMeter
 * (drivers/ui/ui_driver.c:4629-4696).  The firmware runs the three on timers of its own main loop;
 * here every frame gets exactly one of each.  Exact to the reference: the same bits in all six outputs.
 *   fft_len            256 or 512: the display's bins, sd.spec_len (the firmware's fft_iq_len 512 / 1024),
 *                      as in uhsdr_spectrum_config.  1024 is UHSDR_ARGUMENT_ERROR: the firmware has
 *                      no such frame, so its dBm constant is undefined there
 *   magnify            sd.magnify, 0 .. 5;  iq_freq_mode  ts.iq_freq_mode (both as uhsdr_spectrum_config)
 *   dmod_mode, filter_path, sam_sideband, cw_lsb, digi_lsb, cw_sidetone_freq
 *                      as in uhsdr_rx_config; the path gives FilterInfo[].width and the path's offset
 *   digital_mode       ts.digital_mode as UHSDR_DIGITAL_MODE_*; only BPSK matters (is_demod_psk)
 *   dbm_constant       ts.dbm_constant, -100 .. 100, default 0
 *   attack_alpha, decay_alpha   sm.config.alphaSplit, 1 .. 100, defaults 50 / 5 (audio_driver.h:293-296)
 *   snap_enable        cw_decoder_config.snap_enable, default 1 (cw_decoder.c:63)
 *   tune_old           df.tune_old in Hz, one value for the handle
 * A configuration whose passband bins do not satisfy 0 <= Lbin <= Ubin <= fft_len - 1 after the
 * firmware's two clamps (it would index outside sd.FFT_Samples) is UHSDR_ARGUMENT_ERROR.
 * SNAP runs in CW (on the frames whose cw_signal byte is non-zero), AM, SAM and DIGI with BPSK while
 * snap_enable is set; on every other frame snap_carrier_freq keeps its last value (0 after a reset).
 * process_mag: mag = f32 [C][frames][fft_len], frames of FFT_MagData in natural bin order as
 * uhsdr_spectrum_process writes them, device memory (host memory for process_mag_host), stream-ordered;
 * io (null: no output but the state) holds optional rows, each [C][frames], null: not wanted.
 * state: the last outputs per channel into host arrays of num_channels (null: not wanted) after
 * everything enqueued.  reset: averages and outputs 0, freq_old 1e7 as the firmware starts.
 * Reference oddities kept: a passband without a sample above zero "finds" bin 1; a NaN never wins
 * the search; NaN and infinities pass through the sum and the interpolation as they come; a passband
 * of one bin (Lbin == Ubin, as the clamp at 0 gives for CW on the lower sideband with the 300 Hz filter
 * centred on 900 Hz at magnify 5) has a dBm/Hz term of 10 log10(0), finite with Math_log10f_fast; dbm above the
 * table's end is S-count 33.  Defined here, not kept: with the maximum in the last bin the firmware
 * reads one float behind sd.FFT_Samples, here that neighbour is 0; (ulong)help_freq of a NaN, a
 * negative value or one of 2^32 and above is undefined in C, here it is 0.
 * Not built: the codec-gain servo (RadioManagement_HandleRxIQSignalCodecGain), the sc.snap tune
 * request and its counter, all drawing, a per-channel tune_old, the meter on the 1024-point
 * spectrum, inside uhsdr_rx_* or uhsdr_i2s_*, the TX power / SWR meters, any FMA mode. */
enum { UHSDR_DIGITAL_MODE_NONE = 0, UHSDR_DIGITAL_MODE_RTTY = 1, UHSDR_DIGITAL_MODE_BPSK = 2 };
typedef struct uhsdr_meter_config
{
    int32_t fft_len, magnify, iq_freq_mode;
    int32_t dmod_mode, filter_path, sam_sideband, cw_lsb, digi_lsb, digital_mode, cw_sidetone_freq;
    int32_t dbm_constant, attack_alpha, decay_alpha, snap_enable;
    uint32_t tune_old;
    int32_t reserved[9];
} uhsdr_meter_config;
/* what UiSpectrum_CalculateDBm computes before its loops (:2003-2082), and the rest a frame needs */
typedef struct uhsdr_meter_plan
{
    int32_t fft_len, magnify, iq_freq_mode;
    int32_t bin_offset, posbin;
    int32_t lbin, ubin;                     /* (int)Lbin, (int)Ubin after the clamps */
    int32_t snap;                           /* 0 never, 1 every frame, 2 CW: the frames with cw_signal */
    uint32_t tune_old;
    float   bin_bw, width, offset, bw_lower, bw_upper;
    float   cons;                           /* dbm_constant - 225 - (3 at fft_iq_len 1024) */
    float   dbmhz_term;                     /* 10 * Math_log10f_fast((Ubin - Lbin) * bin_BW) */
    float   snap_offset;                    /* CW: -+ cw_sidetone_freq, BPSK: +- PSK_OFFSET, else 0 */
    float   attack_alpha, decay_alpha;      /* the config's times 0.01f */
    float   s_cal_dbm[33];                  /* S_Meter_Cal_dbm */
    int32_t reserved[5];
} uhsdr_meter_plan;
typedef struct uhsdr_meter_io
{
    float*    dbm_cur;                      /* sm.dbm_cur */
    float*    dbmhz_cur;                    /* sm.dbmhz_cur */
    float*    dbm;                          /* sm.dbm */
    float*    dbmhz;                        /* sm.dbmhz */
    int32_t*  s_count;                      /* sm.s_count, 1 .. 33 */
    uint32_t* snap_carrier_freq;            /* ads.snap_carrier_freq */
    const uint8_t* cw_signal;               /* input: ads.CW_signal at each frame; null: 0, a decoder that never saw a pulse */
} uhsdr_meter_io;
typedef struct uhsdr_meter_s* uhsdr_meter_handle;

void         uhsdr_meter_config_default(uhsdr_meter_config* cfg);
uhsdr_status uhsdr_meter_plan_build(const uhsdr_meter_config* cfg, uhsdr_meter_plan* plan);
uhsdr_status uhsdr_meter_create(int32_t num_channels, const uhsdr_meter_config* cfg, void* stream, uhsdr_meter_handle* out);
/* the same meter with its state in host memory, for the _host call (no device call) */
uhsdr_status uhsdr_meter_create_host(int32_t num_channels, const uhsdr_meter_config* cfg, uhsdr_meter_handle* out);
uhsdr_status uhsdr_meter_reset(uhsdr_meter_handle h);
uhsdr_status uhsdr_meter_set_stream(uhsdr_meter_handle h, void* stream);
uhsdr_status uhsdr_meter_process_mag(uhsdr_meter_handle h, const float* mag, int32_t frames, const uhsdr_meter_io* io);
uhsdr_status uhsdr_meter_process_mag_host(uhsdr_meter_handle h, const float* mag, int32_t frames, const uhsdr_meter_io* io);
uhsdr_status uhsdr_meter_state(uhsdr_meter_handle h, float* dbm_cur, float* dbmhz_cur, float* dbm, float* dbmhz, int32_t* s_count,
                               uint32_t* snap_carrier_freq);
uhsdr_status uhsdr_meter_synchronize(uhsdr_meter_handle h);
uhsdr_status uhsdr_meter_destroy(uhsdr_meter_handle h);
int32_t      uhsdr_sizeof_meter_config(void);
int32_t      uhsdr_sizeof_meter_plan(void);
/* The meter inside the spectrum: with a device meter attached, every uhsdr_spectrum_process runs the
   meter's frame on the magnitudes of each display frame it completes, where they lie staged in LDS,
   and writes io's rows ([C][F], F as for mag / avg; io is copied, null: the state only).  mag and avg
   may then both be null: such a call writes no spectrum at all.  A call that completes no frame
   writes nothing.  The meter's state moves exactly as under uhsdr_meter_process_mag on the same
   frames.  meter null detaches: calls then enqueue what they enqueued before.  UHSDR_ARGUMENT_ERROR
   unless fft_len, magnify and iq_freq_mode of the two agree, the meter is a device handle and both
   are on one stream; the caller keeps the meter alive and on that stream while it is attached: after a
   uhsdr_meter_set_stream to another one, uhsdr_spectrum_process is UHSDR_ARGUMENT_ERROR until the
   meter is detached or moved back. */
uhsdr_status uhsdr_spectrum_set_meter(uhsdr_spectrum_handle h, uhsdr_meter_handle meter, const uhsdr_meter_io* io);

/* ---- Display stage (ABI version 9): frames of sd.FFT_AVGData in, scope trace and waterfall line out ----
 * States 4 and 5 of UiSpectrum_RedrawSpectrum (drivers/ui/lcd/ui_spectrum.c:1467-1517) up to the LCD
 * calls, one instance per channel, once per completed display frame and in this order:
 *   UiSpectrum_ScaleFFT (:1258-1292): sig = display_offset + Math_log10f_fast(v) * db_scale per bin, the
 *     frame's minimum of sig before the clamp at 1, the centre frequency moved to the middle and the
 *     order flipped (dest[L-1-i] = src[i + L/2], dest[L-1-i] = src[i - L/2]);
 *   UiSpectrum_ScaleFFT2SpectrumWidth (:1300-1339) when width != fft_len: the fractional reduction in
 *     place, each pixel a sequential binary32 sum in the firmware's order;
 *   display_offset -= agc_rate * min / 5 (:1485), the display's sliding AGC: the only state, -80
 *     (INIT_SPEC_AGC_LEVEL) after create and reset;
 *   the scope trace (:881): height = (uint16_t)(row < limit ? row : limit), limit = scope_h - 1;
 *   the waterfall line (:1104, :1120-1128): row * wfall_contrast, >= 64 -> 63, to uint8_t.
 * The firmware's RedrawType and speed rate limiters are main-loop timing; here every frame gets one
 * of each.  Exact to the reference: the same bits in all four outputs.
 *   fft_len            256 or 512 (sd.spec_len); 1024 is UHSDR_ARGUMENT_ERROR, the firmware has no such panel
 *   width              slayout.scope.w, fft_len / 2 .. fft_len; 0: the firmware's, 256 for 256 and 480 for 512
 *   spectrum_db_scale  ts.spectrum_db_scale, the index into scope_scaling_factors; 9 (SCOPE_SCALE_NUM)
 *                      and above fall back to 3 (DB_DIV_ADJUST_DEFAULT) as :1023-1026; default 3
 *   spectrum_agc_rate  ts.spectrum_agc_rate, 1 .. 50, default 25
 *   waterfall_contrast ts.waterfall.contrast, 10 .. 225, default 120
 *   scope_h            slayout.scope.h, 1 .. 65535; 0: the panel's own after a first power-up with scope
 *                      and waterfall both shown, 21 at 256 and 64 at 512
 * process_avg: avg = f32 [C][frames][fft_len], frames of FFT_AVGData in natural bin order as
 * uhsdr_spectrum_process writes them, 16-byte aligned device memory (host memory for _host),
 * stream-ordered; edge = f32 [C][frames] or null (all 0), see below; io (null: the state only) holds
 * optional rows, null: not wanted.  state: offset and the last min per channel into host arrays of
 * num_channels after everything enqueued.
 * Reference oddities kept: the minimum is taken before the clamp and a NaN never wins it, so a frame of
 * NaNs leaves min at 100000; a NaN passes the clamp; a NaN height is the limit.  For most widths
 * below fft_len (480 of 512 among them, not 200 of 256; the plan's reads_edge says which) the
 * reduction's last pixel reads samples[fft_len], one float behind the scaled row, with a weight of
 * about 2.7e-5 at 512 -> 480: in the firmware that is float fft_len of arm_cfft_f32's output for the same
 * frame, the real part of bin fft_len / 2, which nothing overwrites between the transform and state
 * 4.  That float is `edge`; uhsdr_spectrum_set_display supplies it from the transform itself.
 * Defined here, not kept: C leaves the conversion of a NaN or of a value outside the target's range
 * to uint16_t / uint8_t undefined; here a value in (-2^31, 2^31) is truncated to int32 and its low
 * bits are taken, anything else gives 0, which is what the x86 recording shows.
 * Behind the byte line: uhsdr_wfall_* below (the waterfall's line ring with its frequency-shift
 * padding and scrolling, the palettes and RGB565 pixels, the markers).  Not built: the grid and
 * the bandwidth highlight, the light scope's line drawing, nr_gain_display, the 1024-point spectrum,
 * the redraw rate limiters, any FMA mode. */
typedef struct uhsdr_display_config
{
    int32_t fft_len, width;
    int32_t spectrum_db_scale, spectrum_agc_rate, waterfall_contrast, scope_h;
    int32_t reserved[10];
} uhsdr_display_config;
#define UHSDR_DISPLAY_MAX_WIDTH 512
/* what UiSpectrum_InitSpectrumDisplayData computes (:955-1089), and the walk of
   UiSpectrum_ScaleFFT2SpectrumWidth, which does not depend on the data, per output pixel */
typedef struct uhsdr_display_plan
{
    int32_t fft_len, width;
    int32_t resample;                       /* width != fft_len */
    int32_t reads_edge;                     /* the walk reads samples[fft_len] */
    int32_t limit;                          /* scope_h - 1 */
    float   db_scale;                       /* scope_scaling_factors[].value, times width / fft_len if resampled */
    float   agc_rate;                       /* spectrum_agc_rate / SPECTRUM_AGC_SCALING */
    float   wfall_contrast;                 /* (float)contrast / 100.0 */
    float   full_amount;                    /* (float)fft_len / (float)width */
    int32_t reserved[7];
    uint16_t first[UHSDR_DISPLAY_MAX_WIDTH];  /* idx_old when the pixel's inner loop starts */
    uint8_t  whole[UHSDR_DISPLAY_MAX_WIDTH];  /* samples that loop adds whole, 0 .. 2 */
    float    amount[UHSDR_DISPLAY_MAX_WIDTH]; /* `amount` when that loop ends, at the split sample */
} uhsdr_display_plan;
typedef struct uhsdr_display_io
{
    uint16_t* scope;                        /* [C][frames][width] heights */
    uint8_t*  wfall;                        /* [C][frames][width] palette indices 0 .. 63 */
    float*    offset;                       /* [C][frames] sd.display_offset after the frame's update */
    float*    min;                          /* [C][frames] min1 of the frame */
} uhsdr_display_io;
typedef struct uhsdr_display_s* uhsdr_display_handle;

void         uhsdr_display_config_default(uhsdr_display_config* cfg);
uhsdr_status uhsdr_display_plan_build(const uhsdr_display_config* cfg, uhsdr_display_plan* plan);
uhsdr_status uhsdr_display_create(int32_t num_channels, const uhsdr_display_config* cfg, void* stream, uhsdr_display_handle* out);
/* the same stage with its state in host memory, for the _host call (no device call) */
uhsdr_status uhsdr_display_create_host(int32_t num_channels, const uhsdr_display_config* cfg, uhsdr_display_handle* out);
uhsdr_status uhsdr_display_reset(uhsdr_display_handle h);
uhsdr_status uhsdr_display_set_stream(uhsdr_display_handle h, void* stream);
uhsdr_status uhsdr_display_process_avg(uhsdr_display_handle h, const float* avg, const float* edge, int32_t frames,
                                       const uhsdr_display_io* io);
uhsdr_status uhsdr_display_process_avg_host(uhsdr_display_handle h, const float* avg, const float* edge, int32_t frames,
                                            const uhsdr_display_io* io);
uhsdr_status uhsdr_display_state(uhsdr_display_handle h, float* offset, float* min);
uhsdr_status uhsdr_display_synchronize(uhsdr_display_handle h);
uhsdr_status uhsdr_display_destroy(uhsdr_display_handle h);
int32_t      uhsdr_sizeof_display_config(void);
int32_t      uhsdr_sizeof_display_plan(void);
/* The display stage inside the spectrum: with a device display attached, every uhsdr_spectrum_process
   runs the stage's frame on the average of each display frame it completes, where it lies staged in
   LDS, after the meter's frame when a meter is attached too, and writes io's rows ([C][F][width] and
   [C][F], F as for mag / avg; io is copied, null: the state only).  The kernel takes `edge` from its own
   transform; the caller cannot pass one.  mag and avg may both be null.  A call that completes no
   frame writes nothing.  The display's state moves exactly as under uhsdr_display_process_avg on the
   same frames with that edge.  display null detaches: calls then enqueue what they enqueued before.
   UHSDR_ARGUMENT_ERROR unless fft_len and the channel count of the two agree, the display is a device
   handle and both are on one stream; the caller keeps the display alive and on that stream while it
   is attached, as for uhsdr_spectrum_set_meter. */
uhsdr_status uhsdr_spectrum_set_display(uhsdr_spectrum_handle h, uhsdr_display_handle display, const uhsdr_display_io* io);

/* ---- Waterfall image (ABI version 9): byte lines of palette indices in, the panel's RGB565 rows out ----
 * The rest of UiSpectrum_DrawWaterfall (drivers/ui/lcd/ui_spectrum.c:1099-1256) behind the byte line,
 * with what it takes from UiSpectrum_InitSpectrumDisplayData (:990-1070) and
 * UiSpectrum_UpdateSpectrumPixelParameters (:244-350), one instance per channel:
 *   the ring: frame k's line goes to ring line wfall_line % wfall_size with sd.FFT_frequency beside it
 *     (:1118-1130); wfall_size is the height, halved if height * width exceeds the firmware's 20480
 *     bytes of ring and cut to 20480 / width if half does not fit either (:1046-1064); repeat =
 *     height / wfall_size (:1070);
 *   the counters (:1131-1146): doubleLineStart counts down from `repeat` and wfall_line advances only
 *     when it wraps, so a ring line is written by repeat + 1 consecutive frames and keeps the last;
 *     wfall_line_update counts modulo vert_step_size and only a frame that brings it to 0 draws;
 *   a drawing (:1150-1253) walks back through the ring from the line before wfall_line; per ring line
 *     offset_pixel = (int32)((float)(int32)(line's frequency - the frame's) / hz_per_pixel), replaced
 *     by width - 1 when |offset_pixel| >= width (either sign); the line is moved right by offset_pixel
 *     with black (0) where nothing comes, its bytes go through the palette, the marker columns are
 *     overwritten with entry 64; the first ring line is put repeat + 1 - doubleLineStart times, every
 *     other repeat + 1 times, height rows in all.
 * Exact to the reference: the same bits in every pixel.
 *   width              slayout.wfall.w, 128 .. 512 (what the display stage writes)
 *   height             slayout.wfall.h, 1 .. 255
 *   color_scheme       ts.waterfall.color_scheme, 0 .. 4: grey, hot-cold, rainbow, blue, inverse grey
 *   vert_step_size     ts.waterfall.vert_step_size, 1 .. 5
 *   marker_colour      RGB565, 0 .. 65535: sd.scope_centre_grid_colour_active, palette entry 64
 *   magnify            sd.magnify, 0 .. 5: hz_per_pixel = 48000 / (2^magnify * width)
 *   iq_freq_mode       UHSDR_IQ_CONV_*: where the receive carrier stands when magnify is 0
 *   dmod_mode, digital_mode (UHSDR_DIGITAL_MODE_*), cw_lsb, digi_lsb, cw_sidetone_freq (0 .. 65535),
 *   rtty_shift_idx (0 .. 5), psk_speed_idx (0 .. 2)    which markers there are (:292-335): CW one at
 *                      the sidetone, RTTY two at 915 Hz and 915 Hz + shift, BPSK two at 500 Hz -+ speed / 2,
 *                      anything else one at the carrier
 *   tx_minus_rx_hz     TX dial minus RX dial frequency, which moves every marker (:287)
 * process_lines: lines = u8 [C][frames][width], exactly the wfall row of uhsdr_display_io; center_hz =
 * u32 [C][frames], sd.FFT_frequency of each frame, or null (every frame at 0: nothing is shifted);
 * device memory (host memory for _host), stream-ordered.  io (null: ring and counters only):
 *   image  u16 [C][height][width]: the rows of the last drawing inside this call in the order the
 *          firmware hands them to the panel, row 0 the newest line; untouched if no frame of the call drew
 *   drawn  u8 [C][frames]: 1 where the frame drew
 * The counters never look at the data and are the handle's, one set for all channels, advanced on
 * the host at enqueue; state reports them.  Per channel: the ring and its frequencies, zero after
 * create and reset.
 * Defined here, not kept: doubleLineStart, a function static the firmware never clears, is 0 after
 * create and reset; a ring byte above 64 reads behind the palette in the firmware and is colour 0
 * here (64 is the marker colour in both); a marker position converts to uint16_t as the display
 * stage converts (truncated to int32, low bits; what x86 records); ts.ptt_req is always false.
 * UHSDR_ARGUMENT_ERROR: a value outside the ranges above; a configuration whose wfall_size exceeds
 * the 80 entries of sd.waterfall_frequencies (the firmware would write behind that array: width 128
 * with a height of 81 .. 255 does, widths from 256 on never do); image not 2-byte aligned;
 * lines and image overlapping.
 * Not built: the scope's drawing (grid, bandwidth highlight, light scope), an image per frame,
 * uhsdr_i2s_* with it, any fusion into the spectrum kernel. */
typedef struct uhsdr_wfall_config
{
    int32_t width, height;
    int32_t color_scheme, vert_step_size, marker_colour;
    int32_t magnify, iq_freq_mode, dmod_mode, digital_mode, cw_lsb, digi_lsb;
    int32_t cw_sidetone_freq, rtty_shift_idx, psk_speed_idx;
    int32_t tx_minus_rx_hz;
    int32_t reserved[9];
} uhsdr_wfall_config;
#define UHSDR_WFALL_COLOURS 65              /* NUMBER_WATERFALL_COLOURS + 1 */
#define UHSDR_WFALL_MAX_MARKER 3            /* SPECTRUM_MAX_MARKER */
#define UHSDR_WFALL_MAX_LINES 80            /* entries of sd.waterfall_frequencies */
#define UHSDR_WFALL_RING_BYTES 20480        /* sizeof sd.waterfall */
typedef struct uhsdr_wfall_plan
{
    int32_t width, height;
    int32_t wfall_size;                     /* ring lines */
    int32_t repeat;                         /* sd.repeatWaterfallLine */
    int32_t vert_step_size;
    int32_t marker_num;
    float   hz_per_pixel;
    float   rx_carrier_pos;
    float   marker_pos[UHSDR_WFALL_MAX_MARKER];      /* unused ones: width */
    uint16_t marker_pixel[UHSDR_WFALL_MAX_MARKER];   /* (uint16_t)marker_pos of the markers in use; unused ones: width */
    uint16_t colours[UHSDR_WFALL_COLOURS];           /* sd.waterfall_colours */
    int32_t reserved[8];
} uhsdr_wfall_plan;
typedef struct uhsdr_wfall_io
{
    uint16_t* image;                        /* [C][height][width] */
    uint8_t*  drawn;                        /* [C][frames] */
} uhsdr_wfall_io;
typedef struct uhsdr_wfall_s* uhsdr_wfall_handle;

void         uhsdr_wfall_config_default(uhsdr_wfall_config* cfg);
uhsdr_status uhsdr_wfall_plan_build(const uhsdr_wfall_config* cfg, uhsdr_wfall_plan* plan);
uhsdr_status uhsdr_wfall_create(int32_t num_channels, const uhsdr_wfall_config* cfg, void* stream, uhsdr_wfall_handle* out);
/* the same with ring and frequencies in host memory, for the _host call (no device call) */
uhsdr_status uhsdr_wfall_create_host(int32_t num_channels, const uhsdr_wfall_config* cfg, uhsdr_wfall_handle* out);
uhsdr_status uhsdr_wfall_reset(uhsdr_wfall_handle h);
uhsdr_status uhsdr_wfall_set_stream(uhsdr_wfall_handle h, void* stream);
uhsdr_status uhsdr_wfall_process_lines(uhsdr_wfall_handle h, const uint8_t* lines, const uint32_t* center_hz, int32_t frames,
                                       const uhsdr_wfall_io* io);
uhsdr_status uhsdr_wfall_process_lines_host(uhsdr_wfall_handle h, const uint8_t* lines, const uint32_t* center_hz, int32_t frames,
                                            const uhsdr_wfall_io* io);
/* sd.wfall_line, doubleLineStart and sd.wfall_line_update after everything enqueued; null: not wanted */
uhsdr_status uhsdr_wfall_state(uhsdr_wfall_handle h, uint32_t* wfall_line, uint32_t* double_line_start, uint32_t* wfall_line_update);
uhsdr_status uhsdr_wfall_synchronize(uhsdr_wfall_handle h);
uhsdr_status uhsdr_wfall_destroy(uhsdr_wfall_handle h);
int32_t      uhsdr_sizeof_wfall_config(void);
int32_t      uhsdr_sizeof_wfall_plan(void);

#ifdef __cplusplus
}
#endif
#endif /* UHSDR_H */
