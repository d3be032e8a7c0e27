// Spectral noise reduction: batched frames, one wave per channel (uhsdr_nr.h has the per-bin steps).
//
// nr_frames: a wave loads its channel's state (7 rows of 128 floats and four words) into registers,
// lane l holding bins l and l + 64 and samples l and l + 64 of each half frame, runs the call's
// frames one after the other and stores the state back.  A block is NR_WAVES independent waves; no
// block barrier is used, so the waves past the last channel simply leave.
//
// Per frame: the 256 windowed samples go through cfft_core<256> (uhsdr_cfft.h; the butterfly
// results of 32 lanes are scattered to bin order in LDS), each lane forms |X|^2 of its two bins and
// runs the start-up average or the noise estimate and the gain on them.  The two band powers are
// sequential binary32 sums in bin order, so every lane walks the band over LDS (broadcast reads)
// and all hold the same NN.  The three smoothing loops of the reference reduce to this: a bin b of
// [lo + NN/2, hi - NN/2) gets the mean of Hk[b - NN/2 .. b + NN/2] summed upwards, or, when
// b >= hi - NN, the mean of Hk[b], Hk[b - 1], .. Hk[b - NN + 1] summed downwards, because the
// upper-edge loop runs after the middle loop and overwrites it; what the edge loops write outside
// that range is never copied back to Hk.  Then both halves are weighted (the reference's mirror
// index 255 - b, not 256 - b), icfft256_core brings the frame back, and the first half is
// overlap-added to the second half of the frame before.
#include <hip/hip_runtime.h>
#include <math.h>
#include <new>

#include "uhsdr_arena.h"
#include "uhsdr_cfft.h"
#include "uhsdr_nr.h"
#include "uhsdr_nr_tables.h"

constexpr int NR_WAVES = 4;
constexpr int NR_STATE_FLOATS = NR_F_COUNT * NR_BINS;
// LDS of a wave: the padded FFT frame, the spectrum in bin order (then the time samples), Hk, |X|^2
constexpr int NR_LDS_SPEC = SpecGeom<NR_FFT>::FRAME;
constexpr int NR_LDS_HK = NR_LDS_SPEC + 2 * NR_FFT;
constexpr int NR_LDS_MAG = NR_LDS_HK + NR_BINS;
constexpr int NR_LDS_PITCH = NR_LDS_MAG + NR_BINS;

struct NrArena
{
    int32_t C;
    float* fs;                          // [C][NR_F_COUNT][NR_BINS]
    int32_t* is;                        // [C][NR_I_COUNT] (power_ratio as its bits)
    const float* window;                // SQRT_von_Hann_256
    const uhsdr_spectrum_plan* plan;    // 256 points: twiddles, bit reversal
    // the stream around the frames (uhsdr_nr_process)
    const float* dec_coeffs;            // NR_decimate_coeffs
    const float* int_coeffs;            // NR_interpolate_coeffs
    float* dec_hist;                    // [C][4]: the last 3 input samples
    float* int_hist;                    // [C][20]: the last 19 samples handed to the interpolator
    float* pend;                        // [C][128]: the frame being collected
    float* queue[2];                    // [C][256]: results not yet handed out, the current and the next call's
};

__global__ __launch_bounds__(NR_WAVES * 64) void nr_frames(NrArena a, NrParams p, const float* __restrict__ in, float* __restrict__ out,
                                                           int frames, int stride)
{
    __shared__ __attribute__((aligned(16))) float lds[NR_WAVES][NR_LDS_PITCH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * NR_WAVES + wave;
    if (c >= a.C) return;
    float2* X = (float2*)lds[wave];
    float2* S = (float2*)(lds[wave] + NR_LDS_SPEC);
    float* T = lds[wave] + NR_LDS_SPEC;
    float* hkL = lds[wave] + NR_LDS_HK;
    float* magL = lds[wave] + NR_LDS_MAG;
    const uhsdr_spectrum_plan* __restrict__ P = a.plan;
    const float* tw = P->twiddle;
    const float* twl = &P->tw_lane[0][0][0];

    float* st = a.fs + (size_t)c * NR_STATE_FLOATS;
    int32_t* sw = a.is + (size_t)c * NR_I_COUNT;
    float last_in[2], last_out[2], w[4];
    NrBin b[2];
#pragma unroll
    for (int j = 0; j < 2; j++)
    {
        const int bin = lane + 64 * j;
        last_in[j] = st[NR_F_LAST_IN * NR_BINS + bin];
        last_out[j] = st[NR_F_LAST_OUT * NR_BINS + bin];
        b[j].hk = st[NR_F_HK * NR_BINS + bin];
        b[j].hk_old = st[NR_F_HK_OLD * NR_BINS + bin];
        b[j].xt = st[NR_F_XT * NR_BINS + bin];
        b[j].pslp = st[NR_F_PSLP * NR_BINS + bin];
        b[j].nest = st[NR_F_NEST * NR_BINS + bin];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = a.window[lane + 64 * k];
    int first_time = sw[NR_I_FIRST_TIME], counter = sw[NR_I_INIT_COUNTER], nn = sw[NR_I_NN];
    float ratio = __int_as_float(sw[NR_I_POWER_RATIO]);
    // the butterfly results of this lane land in these bins (lanes 0..31)
    int dst[8];
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = lane < 32 ? (int)P->iperm[8 * lane + k] : 0;

    const float* src = in + (size_t)c * stride;
    float* o = out + (size_t)c * stride;
    for (int f = 0; f < frames; f++)
    {
        if (first_time == 1)
        {
#pragma unroll
            for (int j = 0; j < 2; j++)
            {
                last_in[j] = 0.0f;
                nr_bin_init(&b[j]);
            }
            first_time = 2;
        }
        const float x0 = src[f * NR_BINS + lane], x1 = src[f * NR_BINS + lane + 64];
        float2 z[4] = { make_float2(last_in[0] * w[0], 0.0f), make_float2(last_in[1] * w[1], 0.0f),
                        make_float2(x0 * w[2], 0.0f), make_float2(x1 * w[3], 0.0f) };
        last_in[0] = x0;
        last_in[1] = x1;
        float2 y[1][8];
        cfft_core<NR_FFT>(z, X, tw, twl, lane, y);
        if (lane < 32)
        {
#pragma unroll
            for (int k = 0; k < 8; k++) S[dst[k]] = y[0][k];
        }
        wave_sync();
        float mag[2];
#pragma unroll
        for (int j = 0; j < 2; j++)
        {
            const float2 s = S[lane + 64 * j];
            mag[j] = s.x * s.x + s.y * s.y;
        }
        if (first_time == 2)
        {
#pragma unroll
            for (int j = 0; j < 2; j++) nr_bin_startup(&b[j], mag[j]);
            if (++counter > 19)
            {
                counter = 0;
                first_time = 3;
            }
        }
        // VAD_low / VAD_high are 0 and 63 until the noise reduction runs (:1863-1864)
        int lo = 0, hi = 63;
        if (first_time == 3)
        {
            lo = p.lo;
            hi = p.hi;
#pragma unroll
            for (int j = 0; j < 2; j++)
            {
                const int bin = lane + 64 * j;
                float post, prio;
                nr_bin_estimate(&b[j], mag[j], &p, &post, &prio);
                if (bin >= lo && bin < hi) nr_bin_gain(&b[j], post, prio);
                hkL[bin] = b[j].hk;
                magL[bin] = mag[j];
            }
            wave_sync();
            float pre_power = 0.0f, post_power = 0.0f;
            for (int m = lo; m < hi; m++)
            {
                const float h = hkL[m], x = magL[m];
                pre_power += x;
                post_power += h * h * x;
            }
            nn = nr_smoothing_width(&ratio, pre_power, post_power, &p);
            const int half = nn / 2;
#pragma unroll
            for (int j = 0; j < 2; j++)
            {
                const int bin = lane + 64 * j;
                if (bin >= lo + half && bin < hi - half)
                {
                    float acc = 0.0f;
                    if (bin >= hi - nn)
                        for (int m = bin; m > bin - nn; m--) acc += hkL[m];
                    else
                        for (int m = bin - half; m <= bin + half; m++) acc += hkL[m];
                    b[j].hk = acc / (float)nn;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++)
        {
            const int bin = lane + 64 * j;
            if (bin >= lo && bin < hi)
            {
                const float2 s = S[bin], m = S[NR_FFT - 1 - bin];
                S[bin] = make_float2(s.x * b[j].hk, s.y * b[j].hk);
                S[NR_FFT - 1 - bin] = make_float2(m.x * b[j].hk, m.y * b[j].hk);
            }
        }
        wave_sync();
#pragma unroll
        for (int k = 0; k < 4; k++) z[k] = S[lane + 64 * k];
        icfft256_core(z, X, tw, twl, lane, y);
        if (lane < 32)
        {
#pragma unroll
            for (int k = 0; k < 8; k++) T[dst[k]] = y[0][k].x;
        }
        wave_sync();
#pragma unroll
        for (int j = 0; j < 2; j++)
        {
            const int t = lane + 64 * j;
            o[f * NR_BINS + t] = T[t] * w[j] + last_out[j];
            last_out[j] = T[NR_BINS + t] * w[2 + j];
        }
        wave_sync();                                 // T is read before the next frame's spectrum lands
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
    {
        const int bin = lane + 64 * j;
        st[NR_F_LAST_IN * NR_BINS + bin] = last_in[j];
        st[NR_F_LAST_OUT * NR_BINS + bin] = last_out[j];
        st[NR_F_HK * NR_BINS + bin] = b[j].hk;
        st[NR_F_HK_OLD * NR_BINS + bin] = b[j].hk_old;
        st[NR_F_XT * NR_BINS + bin] = b[j].xt;
        st[NR_F_PSLP * NR_BINS + bin] = b[j].pslp;
        st[NR_F_NEST * NR_BINS + bin] = b[j].nest;
    }
    if (lane == 0)
    {
        sw[NR_I_FIRST_TIME] = first_time;
        sw[NR_I_INIT_COUNTER] = counter;
        sw[NR_I_NN] = nn;
        sw[NR_I_POWER_RATIO] = __float_as_int(ratio);
    }
}

// One frame of one channel on the CPU, in the reference's loops (audio_nr.c:1920-2189) over the
// same per-bin steps.  st / sw: the channel's state rows and words.  The smoothing's Nest values
// go through a scratch array: after the start-up the reference only uses Nest[.][0] as one.
static void nr_frame_host(const uhsdr_spectrum_plan* plan, const float* window, const NrParams* p, float* st, int32_t* sw,
                          const float* in, float* out)
{
    float* last_in = st + NR_F_LAST_IN * NR_BINS;
    float* last_out = st + NR_F_LAST_OUT * NR_BINS;
    float* Hk = st + NR_F_HK * NR_BINS;
    float* Hk_old = st + NR_F_HK_OLD * NR_BINS;
    float* xt = st + NR_F_XT * NR_BINS;
    float* pslp = st + NR_F_PSLP * NR_BINS;
    float* Nest = st + NR_F_NEST * NR_BINS;
    float buf[2 * NR_FFT], X[NR_BINS], post[NR_BINS], prio[NR_BINS], sm[NR_BINS];
    int lo = 0, hi = 63;

    if (sw[NR_I_FIRST_TIME] == 1)
    {
        for (int i = 0; i < NR_BINS; i++)
        {
            NrBin b;
            nr_bin_init(&b);
            last_in[i] = 0.0f;
            Hk[i] = b.hk;
            Hk_old[i] = b.hk_old;
            Nest[i] = b.nest;
            pslp[i] = b.pslp;
        }
        sw[NR_I_FIRST_TIME] = 2;
    }
    for (int i = 0; i < NR_BINS; i++)
    {
        buf[2 * i] = last_in[i];
        buf[2 * i + 1] = 0.0f;
        buf[NR_FFT + 2 * i] = in[i];
        buf[NR_FFT + 2 * i + 1] = 0.0f;
    }
    for (int i = 0; i < NR_BINS; i++) last_in[i] = in[i];
    for (int i = 0; i < NR_FFT; i++) buf[2 * i] *= window[i];
    cfft256_host(plan, buf, 0);
    for (int i = 0; i < NR_BINS; i++) X[i] = buf[2 * i] * buf[2 * i] + buf[2 * i + 1] * buf[2 * i + 1];

    if (sw[NR_I_FIRST_TIME] == 2)
    {
        for (int i = 0; i < NR_BINS; i++)
        {
            NrBin b = { Hk[i], Hk_old[i], xt[i], pslp[i], Nest[i] };
            nr_bin_startup(&b, X[i]);
            Nest[i] = b.nest;
            xt[i] = b.xt;
        }
        if (++sw[NR_I_INIT_COUNTER] > 19)
        {
            sw[NR_I_INIT_COUNTER] = 0;
            sw[NR_I_FIRST_TIME] = 3;
        }
    }
    if (sw[NR_I_FIRST_TIME] == 3)
    {
        lo = p->lo;
        hi = p->hi;
        for (int i = 0; i < NR_BINS; i++)
        {
            NrBin b = { Hk[i], Hk_old[i], xt[i], pslp[i], Nest[i] };
            nr_bin_estimate(&b, X[i], p, &post[i], &prio[i]);
            xt[i] = b.xt;
            pslp[i] = b.pslp;
        }
        for (int i = lo; i < hi; i++)
        {
            NrBin b = { Hk[i], Hk_old[i], xt[i], pslp[i], Nest[i] };
            nr_bin_gain(&b, post[i], prio[i]);
            Hk[i] = b.hk;
            Hk_old[i] = b.hk_old;
        }
        float pre_power = 0.0f, post_power = 0.0f, ratio;
        for (int i = lo; i < hi; i++)
        {
            pre_power += X[i];
            post_power += Hk[i] * Hk[i] * X[i];
        }
        const int NN = nr_smoothing_width(&ratio, pre_power, post_power, p);
        sw[NR_I_NN] = NN;
        memcpy(&sw[NR_I_POWER_RATIO], &ratio, 4);
        for (int i = lo + NN / 2; i < hi - NN / 2; i++)
        {
            sm[i] = 0.0f;
            for (int m = i - NN / 2; m <= i + NN / 2; m++) sm[i] += Hk[m];
            sm[i] /= (float)NN;
        }
        for (int i = lo; i < lo + NN / 2; i++)                 /* lower edge */
        {
            sm[i] = 0.0f;
            for (int m = i; m < i + NN; m++) sm[i] += Hk[m];
            sm[i] /= (float)NN;
        }
        for (int i = hi - NN; i < hi; i++)                     /* upper edge, over the middle loop's values */
        {
            sm[i] = 0.0f;
            for (int m = i; m > i - NN; m--) sm[i] += Hk[m];
            sm[i] /= (float)NN;
        }
        for (int i = lo + NN / 2; i < hi - NN / 2; i++) Hk[i] = sm[i];
    }
    for (int i = lo; i < hi; i++)
    {
        buf[2 * i] = buf[2 * i] * Hk[i];
        buf[2 * i + 1] = buf[2 * i + 1] * Hk[i];
        buf[2 * NR_FFT - 2 * i - 2] = buf[2 * NR_FFT - 2 * i - 2] * Hk[i];
        buf[2 * NR_FFT - 2 * i - 1] = buf[2 * NR_FFT - 2 * i - 1] * Hk[i];
    }
    cfft256_host(plan, buf, 1);
    for (int i = 0; i < NR_FFT; i++) buf[2 * i] *= window[i];
    for (int i = 0; i < NR_BINS; i++) out[i] = buf[2 * i] + last_out[i];
    for (int i = 0; i < NR_BINS; i++) last_out[i] = buf[NR_FFT + 2 * i];
}

struct uhsdr_nr_s : ArenaMem               // one allocation: window, plan, coefficients, state
{
    NrArena a;
    NrParams p;
    uhsdr_nr_config cfg;
    uhsdr_spectrum_plan* host_plan;     // the host twin's tables (and the upload's source)
    size_t floats_end;
    // the stream: positions common to all channels, and the call's work rows
    NrParams sp;                        // the frames' parameters at the rate the stream runs them
    uhsdr_status stream_status;         // of sp: UHSDR_OK, or why uhsdr_nr_process refuses
    bool decimated;                     // filter width below 2701 Hz: frames at 6 ksps
    int64_t seen;                       // samples at the frames' rate since the reset
    int cur;                            // which queue row is current
    float* work;                        // W, Y, Z rows of one call
    size_t work_row;                    // floats per row of each
    uhsdr_nb_handle nb;                 // the noise blanker in front (cfg.nb_setting > 0), of the handle's kind and on its stream
};

static size_t nr_layout(uhsdr_nr_s* h, char* base)
{
    NrArena& a = h->a;
    const size_t C = (size_t)a.C;
    ArenaCarver m{base, 0};
    a.window = m.take<float>(NR_FFT);
    a.plan = m.take<uhsdr_spectrum_plan>(1);
    a.dec_coeffs = m.take<float>(NR_DEC_TAPS);
    a.int_coeffs = m.take<float>(NR_INT_TAPS);
    h->tables = m.off;
    a.fs = m.take<float>(NR_STATE_FLOATS * C);
    a.dec_hist = m.take<float>(4 * C);
    a.int_hist = m.take<float>(NR_INT_PHASE * C);
    a.pend = m.take<float>(NR_BINS * C);
    a.queue[0] = m.take<float>(NR_QUEUE * C);
    a.queue[1] = m.take<float>(NR_QUEUE * C);
    h->floats_end = m.off;              // the float state ends here: reset clears tables .. floats_end
    a.is = m.take<int32_t>(NR_I_COUNT * C);
    return m.off;
}

extern "C" void uhsdr_nr_config_default(uhsdr_nr_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->alpha = 0.94f;                  /* NR_Init */
    cfg->asnr = 30;
    cfg->width = 4;
    cfg->power_threshold_int = 40;       /* the menu's default; NR_Init's power_threshold 0.40 */
    cfg->width_hz = 2700;
    cfg->offset_hz = 1650;
    cfg->sample_rate = 6000;
}

extern "C" float uhsdr_nr_alpha_from_strength(int32_t nr_strength)
{
    return (float)(0.799 + (double)((float)nr_strength / 1000.0));    /* audio_driver.c:1195 */
}

// what spectral_noise_reduction_3 computes at its entry from ts and nr_params
static uhsdr_status nr_params(const uhsdr_nr_config* cfg, NrParams* p)
{
    if (!(cfg->alpha >= 0.0f && cfg->alpha <= 1.0f)) { uhsdr_set_error("nr: alpha %g outside 0..1", cfg->alpha); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->asnr < 2 || cfg->asnr > 30) { uhsdr_set_error("nr: asnr %d outside 2..30", cfg->asnr); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->width < 1 || cfg->width > 5) { uhsdr_set_error("nr: width %d outside 1..5", cfg->width); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->power_threshold_int < 10 || cfg->power_threshold_int > 100)
    { uhsdr_set_error("nr: power_threshold_int %d outside 10..100", cfg->power_threshold_int); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->sample_rate != 6000 && cfg->sample_rate != 12000) { uhsdr_set_error("nr: sample_rate %d: 6000 or 12000", cfg->sample_rate); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->width_hz < 0 || cfg->width_hz > 65535 || cfg->offset_hz < 0 || cfg->offset_hz > 65535)
    { uhsdr_set_error("nr: filter width %d / offset %d out of range", cfg->width_hz, cfg->offset_hz); return UHSDR_ARGUMENT_ERROR; }
    const float width = (float)cfg->width_hz, offset = (float)cfg->offset_hz;
    const float NR_sample_rate = cfg->sample_rate == 6000 ? 6000.0f : 12000.0f;
    const float lf_freq = (offset - width / 2) / (NR_sample_rate / (float)NR_FFT);
    const float uf_freq = (offset + width / 2) / (NR_sample_rate / (float)NR_FFT);
    uint8_t VAD_low = (uint8_t)(int)lf_freq, VAD_high = (uint8_t)(int)uf_freq;     /* a negative lf_freq wraps */
    if (VAD_low == VAD_high) VAD_high++;
    if (VAD_low < 1) VAD_low = 1;
    else if (VAD_low > NR_FFT / 2 - 2) VAD_low = NR_FFT / 2 - 2;
    if (VAD_high < 1) VAD_high = 1;
    else if (VAD_high > NR_FFT / 2) VAD_high = NR_FFT / 2;
    if (!nr_band_in_bounds(VAD_low, VAD_high, cfg->width))
    {
        uhsdr_set_error("nr: band of bins [%d, %d) with smoothing width %d: the reference's smoothing would index outside its arrays",
                        VAD_low, VAD_high, cfg->width);
        return UHSDR_ARGUMENT_ERROR;
    }
    const float xih1 = exp10f((float)((float)(int16_t)cfg->asnr / 10.0));
    p->xih1r = (float)(1.0 / (1.0 + (double)xih1) - 1.0);
    const float pspri = 0.5f;
    p->pfac = (float)((1.0 / (double)pspri - 1.0) * (1.0 + (double)xih1));
    p->power_threshold = (float)((double)(float)cfg->power_threshold_int / 100.0);
    p->alpha = cfg->alpha;
    p->width = cfg->width;
    p->lo = VAD_low;
    p->hi = VAD_high;
    return UHSDR_OK;
}

// a fresh noise reduction: every static zero, first_time 1
static void nr_fresh_words(int32_t* is, int32_t C)
{
    memset(is, 0, sizeof(int32_t) * NR_I_COUNT * (size_t)C);
    for (int32_t c = 0; c < C; c++) is[(size_t)c * NR_I_COUNT + NR_I_FIRST_TIME] = 1;
}

extern "C" uhsdr_status uhsdr_nr_reset(uhsdr_nr_handle h)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const size_t C = (size_t)h->a.C;
    const size_t floats = h->floats_end - h->tables;      // every float of the state, the stream's included
    h->seen = 0;
    h->cur = 0;
    if (h->nb)
    {
        const uhsdr_status st = uhsdr_nb_reset(h->nb);
        if (st != UHSDR_OK) return st;
    }
    if (h->host)
    {
        memset(h->a.fs, 0, floats);
        nr_fresh_words(h->a.is, h->a.C);
        return UHSDR_OK;
    }
    int32_t* words = (int32_t*)malloc(sizeof(int32_t) * NR_I_COUNT * C);
    if (!words) { uhsdr_set_error("nr: host allocation failed"); return UHSDR_DEVICE_ERROR; }
    nr_fresh_words(words, h->a.C);
    hipError_t e = hipMemsetAsync(h->a.fs, 0, floats, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h->a.is, words, sizeof(int32_t) * NR_I_COUNT * C, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);        // words is pageable and freed here
    free(words);
    if (e != hipSuccess) { uhsdr_set_error("nr: reset: %s", hipGetErrorString(e)); return UHSDR_DEVICE_ERROR; }
    return UHSDR_OK;
}

static uhsdr_status nr_create(int32_t num_channels, const uhsdr_nr_config* cfg, bool host, void* stream, uhsdr_nr_handle* out)
{
    if (!out || !cfg || num_channels < 1) { uhsdr_set_error("nr: bad argument"); return UHSDR_ARGUMENT_ERROR; }
    NrParams p;
    uhsdr_status st = nr_params(cfg, &p);
    if (st != UHSDR_OK) return st;
    if (cfg->nb_setting < 0 || cfg->nb_setting > 15) { uhsdr_set_error("nr: nb_setting %d outside 0..15", cfg->nb_setting); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->nr_bypass != 0 && cfg->nr_bypass != 1) { uhsdr_set_error("nr: nr_bypass %d: 0 or 1", cfg->nr_bypass); return UHSDR_ARGUMENT_ERROR; }
    if (cfg->nr_bypass && !cfg->nb_setting)
    { uhsdr_set_error("nr: nr_bypass without the noise blanker (nb_setting 0): the firmware does not enter the stream then"); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_nr_s* h = new (std::nothrow) uhsdr_nr_s();
    if (!h) { uhsdr_set_error("nr: host allocation of the handle failed"); return UHSDR_DEVICE_ERROR; }
    h->a.C = num_channels;
    h->p = p;
    // the stream decides the frames' rate itself (audio_driver.c:2355)
    uhsdr_nr_config sc_cfg = *cfg;
    h->decimated = cfg->width_hz < 2701;
    sc_cfg.sample_rate = h->decimated ? 6000 : 12000;
    h->stream_status = nr_params(&sc_cfg, &h->sp);
    h->cfg = *cfg;
    h->host = host;
    h->stream = (hipStream_t)stream;
    h->bytes = nr_layout(h, nullptr);
    h->host_plan = (uhsdr_spectrum_plan*)malloc(sizeof(uhsdr_spectrum_plan));
    uhsdr_spectrum_config sc;
    uhsdr_spectrum_config_default(&sc);
    sc.fft_len = NR_FFT;
    st = UHSDR_DEVICE_ERROR;
    if (!h->host_plan) uhsdr_set_error("nr: host allocation of %zu bytes failed", sizeof(uhsdr_spectrum_plan));
    else if (uhsdr_spectrum_plan_build(&sc, h->host_plan) == UHSDR_OK) st = h->alloc("nr");     // (plan_build sets its own error text)
    if (st == UHSDR_OK)
    {
        // the four tables go up one by one, so what lies between them in device memory is what hipMalloc left
        nr_layout(h, (char*)h->mem);
        const struct { const void *dst, *src; size_t n; } tab[4] = {
            { h->a.window, uhsdr_nr_sqrt_hann_256, sizeof(float) * NR_FFT },
            { h->a.plan, h->host_plan, sizeof(uhsdr_spectrum_plan) },
            { h->a.dec_coeffs, uhsdr_nr_decimate_coeffs, sizeof(float) * NR_DEC_TAPS },
            { h->a.int_coeffs, uhsdr_nr_interpolate_coeffs, sizeof(float) * NR_INT_TAPS } };
        hipError_t e = hipSuccess;
        for (int t = 0; t < 4 && e == hipSuccess; t++)
        {
            if (host) memcpy((void*)tab[t].dst, tab[t].src, tab[t].n);
            else e = hipMemcpy((void*)tab[t].dst, tab[t].src, tab[t].n, hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) { uhsdr_set_error("nr: table upload failed: %s", hipGetErrorString(e)); st = UHSDR_DEVICE_ERROR; }
    }
    if (st == UHSDR_OK && cfg->nb_setting)
    {
        uhsdr_nb_config nc;
        uhsdr_nb_config_default(&nc);
        nc.nb_setting = cfg->nb_setting;
        st = host ? uhsdr_nb_create_host(num_channels, &nc, &h->nb) : uhsdr_nb_create(num_channels, &nc, stream, &h->nb);
    }
    if (st == UHSDR_OK) st = uhsdr_nr_reset(h);
    if (st != UHSDR_OK) { uhsdr_nr_destroy(h); return st; }
    *out = h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_create(int32_t num_channels, const uhsdr_nr_config* cfg, void* stream, uhsdr_nr_handle* out)
{
    return nr_create(num_channels, cfg, false, stream, out);
}

extern "C" uhsdr_status uhsdr_nr_create_host(int32_t num_channels, const uhsdr_nr_config* cfg, uhsdr_nr_handle* out)
{
    return nr_create(num_channels, cfg, true, nullptr, out);
}

extern "C" uhsdr_status uhsdr_nr_destroy(uhsdr_nr_handle h)
{
    if (!h) return UHSDR_ARGUMENT_ERROR;
    h->release();
    if (h->nb) uhsdr_nb_destroy(h->nb);
    if (h->host) free(h->work);
    else if (h->work) (void)hipFree(h->work);
    free(h->host_plan);
    delete h;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_set_stream(uhsdr_nr_handle h, void* stream)
{
    const uhsdr_status st = arena_set_stream(h, "nr", stream, false);
    return st == UHSDR_OK && h->nb ? uhsdr_nb_set_stream(h->nb, stream) : st;
}

// The call's work rows W, Y, Z of `row` floats each per channel; they only grow
static uhsdr_status nr_work_rows(uhsdr_nr_handle h, size_t row)
{
    if (row <= h->work_row) return UHSDR_OK;
    const size_t bytes = sizeof(float) * 3 * row * (size_t)h->a.C;
    if (h->host)
    {
        free(h->work);
        h->work = (float*)malloc(bytes);
    }
    else
    {
        HIPCHK(hipStreamSynchronize(h->stream));       // earlier calls still read the rows
        if (h->work) (void)hipFree(h->work);
        h->work = nullptr;
        if (hipMalloc((void**)&h->work, bytes) != hipSuccess) h->work = nullptr;
    }
    if (!h->work) { h->work_row = 0; uhsdr_set_error("nr: allocation of %zu bytes failed", bytes); return UHSDR_DEVICE_ERROR; }
    h->work_row = row;
    return UHSDR_OK;
}

// frames W -> Y without the noise reduction (nr_bypass): the copy AudioNr_RunNoiseReduction ends with
static uhsdr_status nr_copy_frames(uhsdr_nr_handle h, const float* src, size_t src_row, float* dst, size_t dst_row, int frames)
{
    const size_t width = sizeof(float) * NR_BINS * (size_t)frames;
    if (h->host)
        for (int32_t c = 0; c < h->a.C; c++) memcpy(dst + (size_t)c * dst_row, src + (size_t)c * src_row, width);
    else
        HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * dst_row, src, sizeof(float) * src_row, width, (size_t)h->a.C, hipMemcpyDeviceToDevice, h->stream));
    return UHSDR_OK;
}

static uhsdr_status nr_check_run(uhsdr_nr_handle h, const float* in, float* out, int32_t frames, int32_t stride)
{
    if (!h || !in || !out) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (frames < 0 || stride < 0 || (int64_t)frames * NR_BINS > stride)
    { uhsdr_set_error("nr: %d frames of %d samples do not fit a row of %d", frames, NR_BINS, stride); return UHSDR_LENGTH_ERROR; }
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_process_frames(uhsdr_nr_handle h, const float* in, float* out, int32_t frames, int32_t stride)
{
    const uhsdr_status st = nr_check_run(h, in, out, frames, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, false, "nr", "uhsdr_nr_process_frames_host")) return UHSDR_ARGUMENT_ERROR;
    if (frames == 0) return UHSDR_OK;
    if (h->nb)
    {
        // the blanker's result goes to the output rows (nr_bypass), or to work rows of the caller's
        // stride, which the noise reduction reads
        if (h->cfg.nr_bypass) return uhsdr_nb_process_frames(h->nb, in, out, frames, stride);
        uhsdr_status sn = nr_work_rows(h, (size_t)stride);
        if (sn == UHSDR_OK) sn = uhsdr_nb_process_frames(h->nb, in, h->work, frames, stride);
        if (sn != UHSDR_OK) return sn;
        in = h->work;
    }
    const int grid = (h->a.C + NR_WAVES - 1) / NR_WAVES;
    hipLaunchKernelGGL(nr_frames, dim3(grid), dim3(NR_WAVES * 64), 0, h->stream, h->a, h->p, in, out, frames, stride);
    HIPCHK(hipGetLastError());
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_process_frames_host(uhsdr_nr_handle h, const float* in, float* out, int32_t frames, int32_t stride)
{
    const uhsdr_status st = nr_check_run(h, in, out, frames, stride);
    if (st != UHSDR_OK) return st;
    if (arena_wrong_kind(h, true, "nr", "uhsdr_nr_process_frames")) return UHSDR_ARGUMENT_ERROR;
    if (h->nb && frames)
    {
        if (h->cfg.nr_bypass) return uhsdr_nb_process_frames_host(h->nb, in, out, frames, stride);
        uhsdr_status sn = nr_work_rows(h, (size_t)stride);
        if (sn == UHSDR_OK) sn = uhsdr_nb_process_frames_host(h->nb, in, h->work, frames, stride);
        if (sn != UHSDR_OK) return sn;
        in = h->work;
    }
    for (int32_t c = 0; c < h->a.C; c++)
        for (int32_t f = 0; f < frames; f++)
            nr_frame_host(h->a.plan, h->a.window, &h->p, h->a.fs + (size_t)c * NR_STATE_FLOATS, h->a.is + (size_t)c * NR_I_COUNT,
                          in + (size_t)c * stride + (size_t)f * NR_BINS, out + (size_t)c * stride + (size_t)f * NR_BINS);
    return UHSDR_OK;
}

// ---- the 12 ksps stream (uhsdr_nr.h has the element functions) ----
// Positions of one call, the same for every channel.
struct NrCall
{
    int decimated, fill, m, n, frames;  // m samples at the frames' rate, n at 12 ksps
    int64_t T0, E0, P0, E1, P1;         // seen / emitted / produced before the call, and after it
    int work_row, stride;
};

// W: the frame being collected and the call's samples at the frames' rate, [C][work_row]
__global__ __launch_bounds__(256) void nr_stream_pre(NrArena a, NrCall k, const float* __restrict__ in, float* __restrict__ W)
{
    const int len = k.fill + k.m;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.C * len) return;
    const int c = (int)(e / len), i = (int)(e % len);
    W[(size_t)c * k.work_row + i] = nr_stream_work(in + (size_t)c * k.stride, a.pend + (size_t)c * NR_BINS, a.dec_hist + (size_t)c * 4,
                                                   a.dec_coeffs, k.decimated, k.fill, i);
}

// Z: what the output FIFO hands out for the call's samples, [C][work_row]
__global__ __launch_bounds__(256) void nr_stream_fifo(NrArena a, NrCall k, const float* __restrict__ queue, const float* __restrict__ Y,
                                                      float* __restrict__ Z)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.C * k.m) return;
    const int c = (int)(e / k.m), i = (int)(e % k.m);
    Z[(size_t)c * k.work_row + i] = nr_stream_emit(queue + (size_t)c * NR_QUEUE, Y + (size_t)c * k.work_row, k.T0, k.E0, k.P0, i);
}

// out: the interpolator and the scale behind the FIFO, or a copy
__global__ __launch_bounds__(256) void nr_stream_post(NrArena a, NrCall k, const float* __restrict__ Z, float* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.C * k.n) return;
    const int c = (int)(e / k.n), o = (int)(e % k.n);
    const float* z = Z + (size_t)c * k.work_row;
    out[(size_t)c * k.stride + o] = k.decimated ? nr_stream_interpolate(z, a.int_hist + (size_t)c * NR_INT_PHASE, o, a.int_coeffs) : z[o];
}

// The state the next call starts from: thread i of a channel moves sample i of the frame being
// collected and result i of the queue (into the other queue row: it reads this one), thread 0 the
// two filter histories (read whole before they are written).
__device__ __host__ static inline void nr_stream_carry(const NrArena& a, const NrCall& k, const float* in, const float* W, const float* Y,
                                                       const float* Z, const float* queue, float* next, int c, int i)
{
    const float* w = W + (size_t)c * k.work_row;
    if (i < (k.fill + k.m) % NR_BINS) a.pend[(size_t)c * NR_BINS + i] = w[k.frames * NR_BINS + i];
    if (i < k.P1 - k.E1)
        next[(size_t)c * NR_QUEUE + i] = nr_stream_result(queue + (size_t)c * NR_QUEUE, Y + (size_t)c * k.work_row, k.E1 + i, k.E0, k.P0);
    if (i == 0)
    {
        const float* x = in + (size_t)c * k.stride;
        float* dh = a.dec_hist + (size_t)c * 4;
        for (int t = 0; t < NR_DEC_TAPS - 1; t++) dh[t] = x[k.n - (NR_DEC_TAPS - 1) + t];      // n >= 8
        const float* z = Z + (size_t)c * k.work_row;
        float* ih = a.int_hist + (size_t)c * NR_INT_PHASE;
        float keep[NR_INT_PHASE - 1];
        for (int t = 0; t < NR_INT_PHASE - 1; t++)
        {
            const int s = k.m - (NR_INT_PHASE - 1) + t;
            keep[t] = s >= 0 ? z[s] : ih[NR_INT_PHASE - 1 + s];
        }
        for (int t = 0; t < NR_INT_PHASE - 1; t++) ih[t] = keep[t];
    }
}

__global__ __launch_bounds__(NR_QUEUE) void nr_stream_next(NrArena a, NrCall k, const float* __restrict__ in, const float* __restrict__ W,
                                                           const float* __restrict__ Y, const float* __restrict__ Z,
                                                           const float* __restrict__ queue, float* __restrict__ next)
{
    nr_stream_carry(a, k, in, W, Y, Z, queue, next, blockIdx.x, threadIdx.x);
}

static uhsdr_status nr_stream_call(uhsdr_nr_handle h, const float* in, float* out, int32_t n, int32_t stride, bool host, NrCall* k)
{
    if (!h || !in || !out) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    if (n < 0 || stride < 0 || n > stride || n % 8 != 0)
    { uhsdr_set_error("nr: %d samples: a multiple of 8 that fits a row of %d", n, stride); return UHSDR_LENGTH_ERROR; }
    if (arena_wrong_kind(h, host, "nr", host ? "uhsdr_nr_process" : "uhsdr_nr_process_host")) return UHSDR_ARGUMENT_ERROR;
    if (h->stream_status != UHSDR_OK && !h->cfg.nr_bypass)
    { uhsdr_set_error("nr: the band at the stream's frame rate (%d) is refused", h->decimated ? 6000 : 12000); return h->stream_status; }
    k->decimated = h->decimated;
    k->n = n;
    k->m = h->decimated ? n / 2 : n;
    k->T0 = h->seen;
    k->fill = (int)(k->T0 % NR_BINS);
    k->frames = (k->fill + k->m) / NR_BINS;
    k->P0 = k->T0 - k->fill;
    k->E0 = k->T0 > NR_LATENCY ? k->T0 - NR_LATENCY : 0;
    const int64_t T1 = k->T0 + k->m;
    k->P1 = T1 - T1 % NR_BINS;
    k->E1 = T1 > NR_LATENCY ? T1 - NR_LATENCY : 0;
    k->stride = stride;
    // the work rows W, Y, Z: fill + m <= 127 + m floats each
    const uhsdr_status sw = nr_work_rows(h, (size_t)NR_BINS + (size_t)k->m);
    if (sw != UHSDR_OK) return sw;
    k->work_row = (int)h->work_row;
    return UHSDR_OK;
}

static void nr_stream_done(uhsdr_nr_handle h, const NrCall& k)
{
    h->seen += k.m;
    h->cur ^= 1;
}

extern "C" uhsdr_status uhsdr_nr_process(uhsdr_nr_handle h, const float* in, float* out, int32_t n, int32_t stride)
{
    NrCall k;
    const uhsdr_status st = nr_stream_call(h, in, out, n, stride, false, &k);
    if (st != UHSDR_OK || n == 0) return st;
    const size_t C = (size_t)h->a.C, plane = C * h->work_row;
    float *W = h->work, *Y = h->work + plane, *Z = h->work + 2 * plane;
    auto blocks = [](size_t elems) { return dim3((unsigned)((elems + 255) / 256)); };
    hipLaunchKernelGGL(nr_stream_pre, blocks(C * (k.fill + k.m)), dim3(256), 0, h->stream, h->a, k, in, W);
    if (k.frames && h->nb)
    {
        // the blanker works on the collected frames in place, as the firmware does, in a launch of its own
        uhsdr_status sn = uhsdr_nb_process_frames(h->nb, W, W, k.frames, k.work_row);
        if (sn == UHSDR_OK && h->cfg.nr_bypass) sn = nr_copy_frames(h, W, h->work_row, Y, h->work_row, k.frames);
        if (sn != UHSDR_OK) return sn;
    }
    if (k.frames && !h->cfg.nr_bypass)
        hipLaunchKernelGGL(nr_frames, dim3((h->a.C + NR_WAVES - 1) / NR_WAVES), dim3(NR_WAVES * 64), 0, h->stream, h->a, h->sp, (const float*)W, Y,
                           k.frames, k.work_row);
    hipLaunchKernelGGL(nr_stream_fifo, blocks(C * k.m), dim3(256), 0, h->stream, h->a, k, (const float*)h->a.queue[h->cur], (const float*)Y, Z);
    hipLaunchKernelGGL(nr_stream_post, blocks(C * k.n), dim3(256), 0, h->stream, h->a, k, (const float*)Z, out);
    hipLaunchKernelGGL(nr_stream_next, dim3(h->a.C), dim3(NR_QUEUE), 0, h->stream, h->a, k, in, (const float*)W, (const float*)Y, (const float*)Z,
                       (const float*)h->a.queue[h->cur], h->a.queue[h->cur ^ 1]);
    HIPCHK(hipGetLastError());
    nr_stream_done(h, k);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_process_host(uhsdr_nr_handle h, const float* in, float* out, int32_t n, int32_t stride)
{
    NrCall k;
    const uhsdr_status st = nr_stream_call(h, in, out, n, stride, true, &k);
    if (st != UHSDR_OK || n == 0) return st;
    const size_t plane = (size_t)h->a.C * h->work_row;
    float *W = h->work, *Y = h->work + plane, *Z = h->work + 2 * plane;
    const NrArena& a = h->a;
    const float* queue = a.queue[h->cur];
    for (int32_t c = 0; c < a.C; c++)
    {
        float* w = W + (size_t)c * k.work_row;
        for (int i = 0; i < k.fill + k.m; i++)
            w[i] = nr_stream_work(in + (size_t)c * stride, a.pend + (size_t)c * NR_BINS, a.dec_hist + (size_t)c * 4, a.dec_coeffs, k.decimated, k.fill, i);
    }
    if (k.frames && h->nb)
    {
        uhsdr_status sn = uhsdr_nb_process_frames_host(h->nb, W, W, k.frames, k.work_row);
        if (sn == UHSDR_OK && h->cfg.nr_bypass) sn = nr_copy_frames(h, W, h->work_row, Y, h->work_row, k.frames);
        if (sn != UHSDR_OK) return sn;
    }
    for (int32_t c = 0; c < a.C; c++)
    {
        float *w = W + (size_t)c * k.work_row, *y = Y + (size_t)c * k.work_row, *z = Z + (size_t)c * k.work_row;
        for (int f = 0; f < (h->cfg.nr_bypass ? 0 : k.frames); f++)
            nr_frame_host(a.plan, a.window, &h->sp, a.fs + (size_t)c * NR_STATE_FLOATS, a.is + (size_t)c * NR_I_COUNT, w + f * NR_BINS, y + f * NR_BINS);
        for (int i = 0; i < k.m; i++) z[i] = nr_stream_emit(queue + (size_t)c * NR_QUEUE, y, k.T0, k.E0, k.P0, i);
        for (int o = 0; o < k.n; o++)
            out[(size_t)c * stride + o] = k.decimated ? nr_stream_interpolate(z, a.int_hist + (size_t)c * NR_INT_PHASE, o, a.int_coeffs) : z[o];
        for (int i = 0; i < NR_QUEUE; i++) nr_stream_carry(a, k, in, W, Y, Z, queue, a.queue[h->cur ^ 1], c, i);
    }
    nr_stream_done(h, k);
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_synchronize(uhsdr_nr_handle h)
{
    return h ? h->synchronize() : UHSDR_ARGUMENT_ERROR;
}

extern "C" uhsdr_status uhsdr_nr_state(uhsdr_nr_handle h, int32_t* first_time, int32_t* nn, float* power_ratio)
{
    if (!h) { uhsdr_set_error("null handle"); return UHSDR_ARGUMENT_ERROR; }
    const size_t C = (size_t)h->a.C;
    int32_t* words = h->a.is;
    if (!h->host)
    {
        words = (int32_t*)malloc(sizeof(int32_t) * NR_I_COUNT * C);
        if (!words) { uhsdr_set_error("nr: host allocation failed"); return UHSDR_DEVICE_ERROR; }
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipMemcpy(words, h->a.is, sizeof(int32_t) * NR_I_COUNT * C, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(words); uhsdr_set_error("nr: state: %s", hipGetErrorString(e)); return UHSDR_DEVICE_ERROR; }
    }
    for (size_t c = 0; c < C; c++)
    {
        if (first_time) first_time[c] = words[c * NR_I_COUNT + NR_I_FIRST_TIME];
        if (nn) nn[c] = words[c * NR_I_COUNT + NR_I_NN];
        if (power_ratio) memcpy(&power_ratio[c], &words[c * NR_I_COUNT + NR_I_POWER_RATIO], 4);
    }
    if (!h->host) free(words);
    return UHSDR_OK;
}

extern "C" uhsdr_nb_handle uhsdr_nr_blanker(uhsdr_nr_handle h) { return h ? h->nb : nullptr; }

extern "C" uhsdr_status uhsdr_nr_band(const uhsdr_nr_config* cfg, int32_t* vad_low, int32_t* vad_high)
{
    if (!cfg) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    NrParams p;
    const uhsdr_status st = nr_params(cfg, &p);
    if (st != UHSDR_OK) return st;
    if (vad_low) *vad_low = p.lo;
    if (vad_high) *vad_high = p.hi;
    return UHSDR_OK;
}

extern "C" uhsdr_status uhsdr_nr_cfft256_host(float* x, int32_t inverse)
{
    if (!x) { uhsdr_set_error("null argument"); return UHSDR_ARGUMENT_ERROR; }
    uhsdr_spectrum_plan* plan = (uhsdr_spectrum_plan*)malloc(sizeof(uhsdr_spectrum_plan));
    uhsdr_spectrum_config sc;
    uhsdr_spectrum_config_default(&sc);
    sc.fft_len = NR_FFT;
    if (!plan) uhsdr_set_error("nr: host allocation of %zu bytes failed", sizeof(uhsdr_spectrum_plan));
    if (!plan || uhsdr_spectrum_plan_build(&sc, plan) != UHSDR_OK) { free(plan); return UHSDR_DEVICE_ERROR; }
    cfft256_host(plan, x, inverse != 0);
    free(plan);
    return UHSDR_OK;
}
