// Host-side (CPU, double precision) design maths of the SDR++ hot path, restated for callers that do not link SDR++'s
// headers.  These functions produce the CONSTANTS the kernels consume (taps, windows, NCO increments, twiddle tables);
// they never touch sample data.  Each cites the reference header it follows (paths relative to /root/reference).
#include "../../include/sdrpp_gpu.h"
#include "host_design.h"

#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace {
constexpr double kPi = 3.14159265358979323846;  // DB_M_PI, core/src/dsp/math/constants.h:3

// core/src/dsp/window/cosine.h:7-15 — generalised cosine-sum window, alternating signs
double cosineWindow(double n, double N, const double* a, int terms) {
    double acc = 0.0, sign = 1.0;
    for (int i = 0; i < terms; i++) {
        acc += sign * a[i] * std::cos((double)i * 2.0 * kPi * n / N);
        sign = -sign;
    }
    return acc;
}
double nuttall(double n, double N) {  // window/nuttall.h:5-8
    static const double a[] = { 0.355768, 0.487396, 0.144232, 0.012604 };
    return cosineWindow(n, N, a, 4);
}
double blackman(double n, double N) {  // window/blackman.h:5-8
    static const double a[] = { 0.42, 0.5, 0.08 };
    return cosineWindow(n, N, a, 3);
}
double sinc(double x) { return (x == 0.0) ? 1.0 : std::sin(x) / x; }           // math/sinc.h:5-7
double hzToRads(double f, double sr) { return 2.0 * kPi * (f / sr); }            // math/hz_to_rads.h:6-8
int estimateTapCount(double tw, double sr) { return (int)(3.8 * sr / tw); }      // taps/estimate_tap_count.h:5

// taps/windowed_sinc.h:9-29 specialised to the two windows the hot path uses
int windowedSinc(int count, double omega, bool alternate, float* taps, int max, double norm = 1.0) {
    const double half = (double)count / 2.0;
    const double corr = norm * omega / kPi;
    for (int i = 0; i < count && i < max; i++) {
        const double t = (double)i - half + 0.5;
        double w = nuttall(t - half, (double)count);
        if (alternate) {  // taps/high_pass.h:11-13: nuttall * (-1)^round(n)
            w = w * ((((int)std::round(t - half)) % 2) ? -1.0f : 1.0f);
        }
        taps[i] = (float)(sinc(t * omega) * w * corr);
    }
    return count;
}
}  // namespace

extern "C" {

int sdrpp_design_low_pass(double cutoff, double trans_width, double sample_rate, int odd, float* taps, int max) {
    int count = estimateTapCount(trans_width, sample_rate);
    if (odd && !(count % 2)) { count++; }
    return windowedSinc(count, hzToRads(cutoff, sample_rate), false, taps, max);
}

int sdrpp_design_high_pass(double cutoff, double trans_width, double sample_rate, int odd, float* taps, int max) {
    int count = estimateTapCount(trans_width, sample_rate);
    if (odd && !(count % 2)) { count++; }
    return windowedSinc(count, hzToRads((sample_rate / 2.0) - cutoff, sample_rate), true, taps, max);
}

// taps/band_pass.h:11-25 with T = complex_t through taps/windowed_sinc.h:9-29: the window function returns phasor(-offsetOmega * (float)n) * nuttall(n, N)
// (complex_t * double: both parts times (float)nuttall), the tap is {(float)sinc, 0} * that (complex_t * complex_t, every product in place) * corr (complex_t * double)
int sdrpp_design_band_pass_complex(double band_start, double band_stop, double trans_width, double sample_rate, int odd, float* taps, int max) {
    if (!(band_stop > band_start)) { return SDRPP_ERR_INVALID; }
    const float offsetOmega = hzToRads((band_start + band_stop) / 2.0, sample_rate);
    int count = estimateTapCount(trans_width, sample_rate);
    if (odd && !(count % 2)) { count++; }
    const double omega = hzToRads((band_stop - band_start) / 2.0, sample_rate);
    const double half = (double)count / 2.0;
    const double corr = 1.0 * omega / kPi;
    for (int i = 0; i < count && 2 * i + 1 < max; i++) {
        const double t = (double)i - half + 0.5;
        const double n = t - half;
        const float x = -offsetOmega * (float)n;
        const float w = (float)nuttall(n, (double)count);
        const float wr = cosf(x) * w, wi = sinf(x) * w;
        const float cr = (float)sinc(t * omega), ci = 0.0f;
        const float pr = (cr * wr) - (ci * wi), pi = (ci * wr) + (cr * wi);
        taps[2 * i] = pr * (float)corr;
        taps[2 * i + 1] = pi * (float)corr;
    }
    return count;
}

// clock_recovery/mm.h:173-178 (generateInterpTaps) through multirate/polyphase_bank.h:15-48: tap i of the prototype is tap i / phases of phase
// (phases - 1) - (i % phases)
int sdrpp_design_mm_interp(int phases, int ntaps, float* bank) {
    if (phases < 1 || phases > 1024 || ntaps < 1 || ntaps > 16 || !bank) { return SDRPP_ERR_INVALID; }
    const int count = phases * ntaps;
    std::vector<float> lp((size_t)count);
    const double bw = 0.5 / (double)phases;
    windowedSinc(count, hzToRads(bw, 1.0), false, lp.data(), count, (double)phases);
    for (int i = 0; i < count; i++) { bank[(size_t)((phases - 1) - (i % phases)) * (size_t)ntaps + (size_t)(i / phases)] = lp[(size_t)i]; }
    return count;
}

// pocsag/dsp.h:20-37: demod.init(NULL, -4500.0, samplerate); recov.init(NULL, samplerate / baudrate, 1e-4, 1.0, 0.05) — MM::init hands
// pcl.init(muGain, omegaGain, 0, 0, 1, omega, omega * (1 - lim), omega * (1 + lim)) doubles that become the loop's floats (mm.h:32)
int sdrpp_design_pager(double if_rate, double baudrate, sdrpp_sym_desc* d) {
    if (!d || !(if_rate > 0.0) || !(baudrate > 0.0) || !std::isfinite(if_rate) || !std::isfinite(baudrate)) { return SDRPP_ERR_INVALID; }
    const double omega = if_rate / baudrate, lim = 0.05;
    d->inv_deviation = (float)(1.0 / hzToRads(-4500.0, if_rate));  // quadrature.h:18-25
    d->shape_ntaps = 10;
    d->omega = (float)omega;
    d->mu_gain = (float)1.0;
    d->omega_gain = (float)1e-4;
    d->min_omega = (float)(omega * (1.0 - lim));
    d->max_omega = (float)(omega * (1.0 + lim));
    d->interp_phases = 128;
    d->interp_ntaps = 8;
    return SDRPP_OK;
}

void sdrpp_design_pll(double bandwidth_d, float* alpha, float* beta);
// radio/src/rds_demod.h:19-41: every member as init leaves it, the doubles of the init calls become the members' floats where the classes store floats
// (fast_agc.h:13-19, pll.h:15-23 through phase_control_loop.h:16-29, mm.h:24-32)
int sdrpp_design_rds_demod(double rate, sdrpp_rdsd_desc* d, float* taps, int max_taps, float* bank, int max_bank) {
    if (!d || !taps || !bank || !(rate > 0.0) || !std::isfinite(rate) || max_bank < 128 * 8) { return SDRPP_ERR_INVALID; }
    const int K = sdrpp_design_band_pass_complex(0.0, 2375.0, 100.0, rate, 0, taps, 0);
    if (K < 1 || K > max_taps) { return SDRPP_ERR_INVALID; }
    sdrpp_design_band_pass_complex(0.0, 2375.0, 100.0, rate, 0, taps, 2 * K);
    if (sdrpp_design_mm_interp(128, 8, bank) != 128 * 8) { return SDRPP_ERR_INVALID; }
    const float FL_PI = 3.1415926535f;  // FL_M_PI, math/constants.h:4
    d->source = 0;
    d->agc_set_point = (float)1.0;
    d->agc_max_gain = (float)1e6;
    d->agc_rate = (float)0.1;
    d->agc_init_gain = (float)1.0;
    sdrpp_design_pll((double)0.005f, &d->loop1.alpha, &d->loop1.beta);  // costas.init(NULL, 0.005f)
    d->loop1.init_phase = 0.0f;
    d->loop1.init_freq = 0.0f;
    d->loop1.min_freq = (float)(double)-FL_PI;
    d->loop1.max_freq = (float)(double)FL_PI;
    const double baudfreq = hzToRads(2375.0 / 2.0, rate);
    sdrpp_design_pll(0.01, &d->loop2.alpha, &d->loop2.beta);  // costas2.init(NULL, 0.01, 0.0, baudfreq, baudfreq - baudfreq * 0.1, baudfreq + baudfreq * 0.1)
    d->loop2.init_phase = (float)0.0;
    d->loop2.init_freq = (float)baudfreq;
    d->loop2.min_freq = (float)(baudfreq - (baudfreq * 0.1));
    d->loop2.max_freq = (float)(baudfreq + (baudfreq * 0.1));
    d->n_taps = K;
    d->taps = taps;
    const double omega = rate / (2375.0 / 2.0), lim = 0.01;  // recov.init(NULL, 5000.0 / (2375.0 / 2.0), 1e-6, 0.01, 0.01)
    d->omega = (float)omega;
    d->mu_gain = (float)0.01;
    d->omega_gain = (float)1e-6;
    d->min_omega = (float)(omega * (1.0 - lim));
    d->max_omega = (float)(omega * (1.0 + lim));
    d->interp_phases = 128;
    d->interp_ntaps = 8;
    d->interp_bank = bank;
    return K;
}

// taps/root_raised_cosine.h:8-34: Ts = samplerate / symbolrate; the tap in the middle, the two at +-Ts / (4 beta), every other one
int sdrpp_design_root_raised_cosine(int count, double beta, double symbolrate, double samplerate, float* taps, int max) {
    if (count < 1 || count > max || !taps || !(beta > 0.0) || !(symbolrate > 0.0) || !(samplerate > 0.0) || !std::isfinite(beta) || !std::isfinite(symbolrate) || !std::isfinite(samplerate)) {
        return SDRPP_ERR_INVALID;
    }
    const double Ts = samplerate / symbolrate;
    const double half = (double)count / 2.0;
    const double limit = Ts / (4.0 * beta);
    const double kSqrt2 = 1.41421356237309504880;  // DB_M_SQRT2, math/constants.h
    for (int i = 0; i < count; i++) {
        const double t = (double)i - half + 0.5;
        double v;
        if (t == 0.0) { v = (1.0 + beta * (4.0 / kPi - 1.0)) / Ts; }
        else if (t == limit || t == -limit) { v = ((1.0 + 2.0 / kPi) * std::sin(kPi / (4.0 * beta)) + (1.0 - 2.0 / kPi) * std::cos(kPi / (4.0 * beta))) * beta / (Ts * kSqrt2); }
        else { v = ((std::sin((1.0 - beta) * kPi * t / Ts) + std::cos((1.0 + beta) * kPi * t / Ts) * 4.0 * beta * t / Ts) / ((1.0 - (4.0 * beta * t / Ts) * (4.0 * beta * t / Ts)) * kPi * t / Ts)) / Ts; }
        taps[i] = (float)v;
    }
    return count;
}

// m17_decoder/src/m17dsp.h: M17Decoder::init calls demod.init(input, 4800.0f, sampleRate, 2400.0f, 31, 0.5f, 1e-6f, 0.01f, 0.01f) — GFSK::init (demod/gfsk.h:24-35)
// hands Quadrature(deviation, samplerate), rootRaisedCosine(31, 0.5, 4800, samplerate) and MM(samplerate / 4800, omegaGain, muGain, omegaRelLimit), every float
// literal widened to a double on the way.  The framing is stated from the M17 specification: sync words, decorrelator sequence, quadratic interleaver.
int sdrpp_design_m17(double if_rate, sdrpp_sym_desc* sym, float* rrc_taps, int max_taps, sdrpp_frame_desc* frame, uint8_t* scramble, uint16_t* interleave) {
    if (!sym || !rrc_taps || !frame || !scramble || !interleave || !(if_rate > 0.0) || !std::isfinite(if_rate)) { return SDRPP_ERR_INVALID; }
    const double baud = (double)4800.0f, dev = (double)2400.0f, beta = (double)0.5f, omega_gain = (double)1e-6f, mu_gain = (double)0.01f, lim = (double)0.01f;
    const int K = sdrpp_design_root_raised_cosine(31, beta, baud, if_rate, rrc_taps, max_taps);
    if (K != 31) { return SDRPP_ERR_INVALID; }
    const double omega = if_rate / baud;
    sym->inv_deviation = (float)(1.0 / hzToRads(dev, if_rate));  // quadrature.h:18-25
    sym->shape_ntaps = K;
    sym->shape_taps = rrc_taps;
    sym->omega = (float)omega;
    sym->mu_gain = (float)mu_gain;
    sym->omega_gain = (float)omega_gain;
    sym->min_omega = (float)(omega * (1.0 - lim));
    sym->max_omega = (float)(omega * (1.0 + lim));
    sym->interp_phases = 128;
    sym->interp_ntaps = 8;
    // the decorrelator sequence of the M17 specification, 46 bytes, read MSB first
    static const uint8_t kSeq[46] = { 0xD6, 0xB5, 0xE2, 0x30, 0x82, 0xFF, 0x84, 0x62, 0xBA, 0x4E, 0x96, 0x90, 0xD8, 0x98, 0xDD, 0x5D, 0x0C, 0xC8, 0x52, 0x43, 0x91, 0x1D, 0xF8,
                                      0x6E, 0x68, 0x2F, 0x35, 0xDA, 0x14, 0xEA, 0xCD, 0x76, 0x19, 0x8D, 0xD5, 0x80, 0xD1, 0x33, 0x87, 0x13, 0x57, 0x18, 0x2D, 0x29, 0x78, 0xC3 };
    for (int k = 0; k < 368; k++) {
        scramble[k] = (uint8_t)((kSeq[k >> 3] >> (7 - (k & 7))) & 1);
        interleave[k] = (uint16_t)((45ll * k + 92ll * k * k) % 368);  // the specification's quadratic permutation polynomial
    }
    frame->high_cut = (1.0f + (1.0f / 3.0f)) / 2.0f;  // half way between the inner and the outer level
    frame->n_sync = 3;
    frame->sync[0] = 0x55F7;  // link setup
    frame->sync[1] = 0xFF5D;  // stream
    frame->sync[2] = 0x75FF;  // packet
    frame->sync[3] = 0;
    frame->frame_bits = 368;
    frame->scramble = scramble;
    frame->interleave = interleave;
    return SDRPP_OK;
}

// meteor_demodulator/src/meteor_demod.h:24-43: every member as init leaves it (fast_agc.h:13-19, meteor_costas.h:13-16 through pll.h:15-23, mm.h:24-32).
// init takes omegaRelLimit and does not hand it to recov.init: MM's limit is its default, 0.01
int sdrpp_design_meteor(double symbolrate, double samplerate, int rrc_taps, double rrc_beta, double agc_rate, double costas_bw, int broken, int oqpsk, double omega_gain,
                        double mu_gain, sdrpp_qpsk_desc* d, float* taps, int max_taps, float* bank, int max_bank) {
    if (!d || !taps || !bank || max_bank < 128 * 8 || !std::isfinite(agc_rate) || !std::isfinite(costas_bw) || !std::isfinite(omega_gain) || !std::isfinite(mu_gain)) { return SDRPP_ERR_INVALID; }
    const int K = sdrpp_design_root_raised_cosine(rrc_taps, rrc_beta, symbolrate, samplerate, taps, max_taps);
    if (K < 1) { return SDRPP_ERR_INVALID; }
    if (sdrpp_design_mm_interp(128, 8, bank) != 128 * 8) { return SDRPP_ERR_INVALID; }
    const float FL_PI = 3.1415926535f;  // FL_M_PI, math/constants.h:4
    d->n_taps = K;
    d->taps = taps;
    d->agc_set_point = (float)1.0;  // agc.init(NULL, 1.0, 10e6, agcRate)
    d->agc_max_gain = (float)10e6;
    d->agc_rate = (float)agc_rate;
    d->agc_init_gain = (float)1.0;
    sdrpp_design_pll(costas_bw, &d->loop.alpha, &d->loop.beta);  // costas.init(NULL, costasBandwidth, brokenModulation)
    d->loop.init_phase = (float)0.0;
    d->loop.init_freq = (float)0.0;
    d->loop.min_freq = (float)(double)-FL_PI;
    d->loop.max_freq = (float)(double)FL_PI;
    d->broken = broken != 0;
    d->oqpsk = oqpsk != 0;
    const double omega = samplerate / symbolrate, lim = 0.01;  // recov.init(NULL, _samplerate / _symbolrate, omegaGain, muGain, omegaRelLimit = 0.01)
    d->omega = (float)omega;
    d->mu_gain = (float)mu_gain;
    d->omega_gain = (float)omega_gain;
    d->min_omega = (float)(omega * (1.0 - lim));
    d->max_omega = (float)(omega * (1.0 + lim));
    d->interp_phases = 128;
    d->interp_ntaps = 8;
    d->interp_bank = bank;
    d->soft_scale = 84.0f;  // main.cpp:198-199
    return K;
}

void sdrpp_design_pll(double bandwidth_d, float* alpha, float* beta) {
    const float bandwidth = bandwidth_d;  // criticallyDamped(T bandwidth, ...) with T = float
    const float dampningFactor = sqrt(2.0) / 2.0;
    const float denominator = (1.0 + 2.0 * dampningFactor * bandwidth + bandwidth * bandwidth);
    *alpha = (4 * dampningFactor * bandwidth) / denominator;
    *beta = (4 * bandwidth * bandwidth) / denominator;
}

int sdrpp_design_fft_window(int kind, int nz, float* window) {
    if (kind < 0 || kind > 2 || nz <= 0 || !window) { return SDRPP_ERR_INVALID; }
    for (int i = 0; i < nz; i++) {
        const float flip = (i % 2) ? -1.0f : 1.0f;  // fftshift folded into the window, iq_frontend.cpp:284-290
        if (kind == 0) { window[i] = 1.0f * flip; }
        else if (kind == 1) { window[i] = blackman(i, nz) * flip; }
        else { window[i] = nuttall(i, nz) * flip; }
    }
    return SDRPP_OK;
}

void sdrpp_design_reshape_params(double sample_rate, int fft_size, double fft_rate, int* skip, int* nz) {
    const int interval = (int)std::round(sample_rate / fft_rate);  // iq_frontend.h:60
    *nz = interval < fft_size ? interval : fft_size;
    *skip = interval - *nz;
}

void sdrpp_design_phase_delta(double offset_hz, double sample_rate, float* re, float* im) {
    const double w = hzToRads(offset_hz, sample_rate);
    *re = (float)std::cos(w);
    *im = (float)std::sin(w);
}

// The 256 values a U8 source can produce, each in that source's own arithmetic (the types are the point: see include/sdrpp_gpu.h)
int sdrpp_design_u8_table(int source, float gain, float* table256) {
    if (!table256 || source < 0 || source > 2) { return SDRPP_ERR_INVALID; }
    const float scale = 1.0f / (gain * 128.0f);  // spyserver_client.cpp:139
    for (int i = 0; i < 256; i++) {
        const unsigned char b = (unsigned char)i;
        if (source == 0) { table256[i] = ((float)b - 127.4) / 128.0f; }          // rtl_sdr_source/src/main.cpp:535: double subtraction and division, rounded by the store
        else if (source == 1) { table256[i] = ((double)b - 128.0) / 128.0; }      // rtl_tcp_client.cpp:86
        else { table256[i] = ((float)b - 128.0f) * scale; }                       // spyserver_client.cpp:141
    }
    return SDRPP_OK;
}

float sdrpp_design_deemphasis_alpha(double tau, double sample_rate) {
    const float dt = 1.0f / sample_rate;  // deephasis.h:91-92: float dt = 1.0f / _samplerate; alpha = dt / (_tau + dt);
    return (float)(dt / (tau + dt));
}

int sdrpp_design_resampler(double in_sr, double out_sr, int max_ratio, int* mode, int* predec_ratio, int* interp, int* decim,
                           float* taps, int max) {
    // rational_resampler.h:120-165.  Note the reference clamps the POWER against the maximum RATIO (line 122); kept.
    int power = (int)std::floor(std::log2(in_sr / out_sr));
    if (power > max_ratio) { power = max_ratio; }
    int ratio = (power >= 0 && power < 31) ? (1 << power) : max_ratio;
    if (ratio > max_ratio) { ratio = max_ratio; }
    const bool useDecim = (in_sr > out_sr && power > 0);
    double intSr = in_sr;
    *predec_ratio = 1;
    if (useDecim) {
        intSr = in_sr / (double)ratio;
        *predec_ratio = ratio;
    }
    const int iSr = (int)std::round(intSr), oSr = (int)std::round(out_sr);
    const int g = std::gcd(iSr, oSr);
    *interp = oSr / g;
    *decim = iSr / g;
    if (*interp == *decim) {
        *mode = useDecim ? 1 : 3;
        return 0;
    }
    const double tapSr = intSr * (double)(*interp);
    const double tapBw = (in_sr < out_sr ? in_sr : out_sr) / 2.0;
    const double tapTw = tapBw * 0.1;
    const int n = sdrpp_design_low_pass(tapBw, tapTw, tapSr, 0, taps, max);
    for (int i = 0; i < n && i < max; i++) { taps[i] *= (float)(*interp); }  // line 159
    *mode = useDecim ? 0 : 2;
    return n;
}

void sdrpp_design_waterfall_view(double view_offset, double view_bandwidth, double whole_bandwidth, int raw_fft_size,
                                 int* draw_data_start, int* draw_data_size) {
    const double offsetRatio = view_offset / (whole_bandwidth / 2.0);                        // waterfall.cpp:892
    const int size = (view_bandwidth / whole_bandwidth) * raw_fft_size;                       // :893
    const int start = (((double)raw_fft_size / 2.0) * (offsetRatio + 1)) - (size / 2);        // :894
    *draw_data_start = start;
    *draw_data_size = size;
}

}  // extern "C"

namespace sdrpp_host {

// FFT twiddle tw(e, L) = exp(-2*pi*i*e/L) as float2.  Only the first octant is evaluated with libm (double, rounded
// once); the rest of the circle follows from exact sign/swap symmetries, so tw(e + L/4) == -j * tw(e) bit for bit —
// the kernels rely on that to derive half of their twiddles by a register swap.
void twiddle(int e, int L, float* re, float* im) {
    int circle = L, idx = ((e % L) + L) % L;
    if (circle < 8) { idx *= 8 / circle; circle = 8; }
    const int quarter = circle / 4;
    const int quadrant = idx / quarter, rem = idx % quarter;
    float c, s;
    if (rem <= circle / 8) {
        const double a = 2.0 * kPi * ((double)rem / (double)circle);
        c = (float)std::cos(a);
        s = (float)std::sin(a);
    }
    else {
        const double a = 2.0 * kPi * ((double)(quarter - rem) / (double)circle);
        c = (float)std::sin(a);
        s = (float)std::cos(a);
    }
    float cf, sf;
    if (quadrant == 0) { cf = c; sf = s; }
    else if (quadrant == 1) { cf = -s; sf = c; }
    else if (quadrant == 2) { cf = -c; sf = -s; }
    else { cf = s; sf = -c; }
    *re = cf;
    *im = -sf;
}

// doZoom's float32 running index (waterfall.cpp:74-89) evaluated once per view change: for each output pixel the first
// bin and the number of bins it covers.  The kernel then only does the max-reduction.
void zoomTable(int offset, int width, int inSize, int outSize, std::vector<int32_t>& start, std::vector<int32_t>& count) {
    if (offset < 0) { offset = 0; }
    if (width > 524288) { width = 524288; }
    start.assign((size_t)outSize, 0);
    count.assign((size_t)outSize, 0);
    const float factor = (float)width / (float)outSize;
    const float sFactor = std::ceil(factor);
    float id = (float)offset;
    for (int i = 0; i < outSize; i++) {
        const int sId = (int)id;
        const float uFactor = (sId + sFactor > inSize) ? sFactor - ((sId + sFactor) - inSize) : sFactor;
        int n = 0;
        for (int j = 0; j < uFactor; j++) { n++; }  // same float comparison as the reference loop
        start[(size_t)i] = sId;
        count[(size_t)i] = n;
        id += factor;
    }
}

// Effective NCO increment of the reference rotator in turns per sample: the recursion phase *= phaseDelta advances by
// arg(phaseDelta) each sample, where phaseDelta is the float pair the reference stores (frequency_xlator.h:17).
double turnsPerSample(float re, float im) { return std::atan2((double)im, (double)re) / (2.0 * kPi); }

// FMIF (noise_reduction/fm_if.h:45-77, :113) as one matrix: the window (nuttall(n, N - 1), stored as float like the reference's fftWin), the forward
// DFT and the twiddle the un-normalised backward DFT of a single bin gives at index N / 2,
//     A[k][n] = w[n] * e^{-j 2 pi k (n - N/2) / N},      N = bins, integer N / 2
// designed in double and rounded to float.  tab: [2][32][32] floats, re then im, A[k][n] at [n][k], zero for k >= N or n >= N.
void fmifMatrix(int bins, float* tab) {
    const int N = bins, half = N / 2;
    for (int i = 0; i < 2 * 32 * 32; i++) { tab[i] = 0.0f; }
    for (int n = 0; n < N; n++) {
        const double w = (double)(float)nuttall((double)n, (double)(N - 1));
        for (int k = 0; k < N; k++) {
            const int m = (((k * (n - half)) % N) + N) % N;  // the angle reduced exactly
            const double a = -2.0 * kPi * (double)m / (double)N;
            tab[n * 32 + k] = (float)(w * std::cos(a));
            tab[1024 + n * 32 + k] = (float)(w * std::sin(a));
        }
    }
}

}  // namespace sdrpp_host
