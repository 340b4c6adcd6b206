/*
 * sdrpp_gpu.h — C-ABI of the MI355X (gfx950) implementation of SDR++'s streaming-DSP hot path.
 *
 * One `sdrpp_ctx` = one wideband IQ stream on one GPU = what one `IQFrontEnd` owns in the reference
 * (core/src/signal_path/iq_frontend.h:12-109): the FFT -> log-power -> waterfall-line branch and N per-VFO channelisers
 * (dsp::channel::RxVFO, core/src/dsp/channel/rx_vfo.h) followed by the radio module's demodulators
 * (decoder_modules/radio/src/demodulators/{wfm,nfm,am,usb,lsb,dsb}.h).  All arithmetic runs in hand-written HIP
 * kernels; there is NO CPU fallback — every entry point returns SDRPP_ERR_NO_DEVICE when no gfx950 device exists.
 *
 * Conventions: plain C, opaque context, `int` return (0 = OK, negative = error, see sdrpp_strerror), no exceptions,
 * no C++ or torch types.  Complex IQ is interleaved float32 {re, im} (dsp::complex_t, core/src/dsp/types.h:6-92);
 * audio is interleaved float32 {l, r} (dsp::stereo_t, types.h:94-127).  A context is thread-compatible: one caller
 * thread at a time (the reference serialises reconfiguration with block::ctrlMtx + tempStop/tempStart,
 * core/src/dsp/block.h:46-62; the host block wrappers in sdrplusplus_amd/host keep that rule).
 *
 * The taps / window / NCO constants are passed IN by the caller, designed with the reference's own double-precision
 * host maths (dsp/taps, dsp/window, dsp/multirate/decim/plans.h) so that they stay bit-identical to what an
 * SDR++ build computes; sdrpp_design_* below restate that maths for callers that do not link SDR++'s headers.
 */
#ifndef SDRPP_GPU_H
#define SDRPP_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRPP_OK 0
#define SDRPP_ERR_NO_DEVICE (-1)   /* no HIP device / not gfx950 / HIP runtime error at create */
#define SDRPP_ERR_INVALID (-2)     /* bad argument or call sequence */
#define SDRPP_ERR_NOMEM (-3)       /* hipMalloc failed */
#define SDRPP_ERR_HIP (-4)         /* HIP runtime error (message in sdrpp_last_error) */
#define SDRPP_ERR_UNSUPPORTED (-5) /* parameter outside what the kernels implement */
#define SDRPP_ERR_NOT_FOUND (-6)   /* unknown VFO id (IQFrontEnd::removeVFO logs the same condition, iq_frontend.cpp:164-167) */

typedef struct sdrpp_ctx sdrpp_ctx;

/* ---- lifecycle ----------------------------------------------------------------------------------------------------- */
/* Replaces IQFrontEnd::init's allocation half (iq_frontend.cpp:17-71).  `max_push` = largest sample count one
 * sdrpp_push* call will carry (the reference's streams carry <= 1 000 000, core/src/dsp/stream.h:9; device-resident
 * callers may use larger batches).
 * The SDRPP_GPU_* environment variables the library reads when a context is created (grid rules of the ticks, SDRPP_GPU_FRONT_WAVES, ...)
 * are test and measurement switches: results are bit-identical with or without them, only the shape of the launches changes.  A host
 * does not set them; unset is the tuned configuration. */
int sdrpp_device_count(void);   /* usable devices (0: none — nothing here runs without one) */
int sdrpp_create(int device, int64_t max_push, sdrpp_ctx** ctx);
int sdrpp_destroy(sdrpp_ctx* ctx);
const char* sdrpp_strerror(int code);
const char* sdrpp_last_error(const sdrpp_ctx* ctx);
/* Run all work of this context on the caller's HIP stream (hipStream_t cast to void*), e.g. torch's current stream;
 * NULL restores the context-owned stream. */
int sdrpp_set_stream(sdrpp_ctx* ctx, void* hip_stream);
int sdrpp_sync(sdrpp_ctx* ctx);
/* ABI self-description for foreign-function bindings: returns the ABI version and, if non-NULL, sizeof(sdrpp_vfo_desc). */
#define SDRPP_ABI_VERSION 2   /* 2: sdrpp_vfo_desc.nco_mode, sdrpp_pipeline_stats */
/* (sdrpp_push_raw / sdrpp_push_frame / sdrpp_design_u8_table / sdrpp_iq_format are additions: no existing call or structure changed, the version stays 2) */
int sdrpp_abi_version(int* sizeof_vfo_desc);
/* Human-readable device name / arch into buf (for logs and bench records). */
int sdrpp_device_info(sdrpp_ctx* ctx, char* buf, int buflen);

/* ---- host-side design maths (pure CPU, double precision; restates the reference's header maths) ---------------------- */
/* dsp/taps/low_pass.h:7-11, high_pass.h:7-15 (Nuttall-windowed sinc, tap count int(3.8*sr/tw)).  Return the tap count;
 * write min(count, max) taps.  Call with max = 0 to size the buffer. */
int sdrpp_design_low_pass(double cutoff, double trans_width, double sample_rate, int odd_tap_count, float* taps, int max);
int sdrpp_design_high_pass(double cutoff, double trans_width, double sample_rate, int odd_tap_count, float* taps, int max);
/* iq_frontend.cpp:280-291: kind 0 RECTANGULAR, 1 BLACKMAN, 2 NUTTALL; includes the (-1)^i fftshift factor. */
/* taps::bandPass<complex_t> (dsp/taps/band_pass.h:11-25): `count` complex taps, interleaved (re, im), into taps[0 .. 2 * count) while 2 * count <= max; returns count */
int sdrpp_design_band_pass_complex(double band_start, double band_stop, double trans_width, double sample_rate, int odd_tap_count, float* taps, int max);
/* loop::PhaseControlLoop<float>::criticallyDamped (dsp/loop/phase_control_loop.h:31-36) as loop::PLL::init calls it, evaluated in float like the reference */
void sdrpp_design_pll(double bandwidth, float* alpha, float* beta);
int sdrpp_design_fft_window(int kind, int nz, float* window);
/* iq_frontend.h:59-63 */
void sdrpp_design_reshape_params(double sample_rate, int fft_size, double fft_rate, int* skip, int* nz);
/* frequency_xlator.h:17,28: phaseDelta = (float)cos(w), (float)sin(w), w = 2*pi*(offset_hz/sample_rate). */
void sdrpp_design_phase_delta(double offset_hz, double sample_rate, float* re, float* im);
/* rational_resampler.h:120-165: picks the power-of-two pre-decimation, the polyphase L/M and designs the polyphase taps
 * (already multiplied by L).  mode: 0 BOTH, 1 DECIM_ONLY, 2 RESAMP_ONLY, 3 NONE.  `max_ratio` = 1 << plans_len
 * (power_decimator.h:29-31; 8192 for the reference's tables).  Returns tap count (0 if no polyphase stage). */
int sdrpp_design_resampler(double in_sr, double out_sr, int max_ratio, int* mode, int* predec_ratio, int* interp, int* decim,
                           float* taps, int max);
/* filter/deephasis.h:90-93: alpha = dt / (tau + dt), dt = 1.0f / samplerate (float arithmetic as in the reference). */
float sdrpp_design_deemphasis_alpha(double tau, double sample_rate);
/* gui/widgets/waterfall.cpp:891-894 (view -> bin window) */
void sdrpp_design_waterfall_view(double view_offset, double view_bandwidth, double whole_bandwidth, int raw_fft_size,
                                 int* draw_data_start, int* draw_data_size);

/* ---- what in the reference depends on how its stream is cut into blocks ---------------------------------------------------------------
 * Two operations of the path are block-size dependent in the reference: loop::AGC's look-ahead on clipping scans to the end of the
 * CURRENT block (agc.h:91-104; AM and SSB demodulators), and VOLK's rotator renormalises its phase at the end of every call
 * (frequency_xlator.h:43-50).  ref_block > 0: every push is treated as consecutive reference blocks of `ref_block` input samples (the
 * last one may be shorter), whatever the push size — e.g. sample_rate / 200 for a file source (file_source/src/main.cpp:157) — and the
 * block ends are carried through the decimators / resampler down to the demodulator's rate.  0 (default): one push = one block. */
int sdrpp_set_reference_block(sdrpp_ctx* ctx, int ref_block);
/* NCO of the frequency translations (RxVFO's xlator, SSB's second xlator).
 *   SDRPP_NCO_CLOSED_FORM (default): phase = arg(phaseDelta) * n evaluated in float64, folded into the first filter's taps; exact
 *     frequency, no drift.  FM / AM outputs agree with the reference to ~1e-7 for any run length; the raw IF and an SSB product detector
 *     additionally see the reference rotator's own rounding drift (1e-10 .. 2e-9 rad per sample, linear in time), which this mode does not have.
 *     VALIDITY WINDOW against the reference for SSB / DSB audio and the raw IF — MEASURED by tests/test_bench_geometry_gpu.py::
 *     test_closed_form_nco_validity_window_vs_pinned_oracle (BASELINE cfg 4, 61.44 MS/s, 42 USB channels, pipelined, against the oracle pinned to
 *     the reference's own rotator; windows of 10^5 INPUT samples since the VFO was added / reset, errors relative to the RMS of the reference
 *     stream): audio inside BASELINE.json's 1e-5 over the first 2e5 input samples for every channel; once the channel filter has filled
 *     (10^6 samples) the difference grows by 2.8e-8 .. 1.05e-5 per 10^5 samples (median channel 1.5e-6), the raw IF by 1.0e-7 .. 3.1e-5
 *     (median 4.5e-6): the worst channel leaves 1e-5 in the third window, the median channel after ~1.2e6 input samples (20 ms of the stream);
 *     against the reference with its rotator replaced by an exact NCO it stays at
 *     3e-7 for any length.  A host that needs SSB / raw-IF parity with the reference's OWN phase sequence beyond that window selects
 *     SDRPP_NCO_REFERENCE_ROTATOR for those channels (sdrpp_vfo_desc.nco_mode = 2: per VFO, the FM / AM channels of the bank stay on the fast path).
 *   SDRPP_NCO_REFERENCE_ROTATOR: the reference's float recursion itself (VOLK generic rotator2: phase *= phaseDelta in float, renormalised
 *     every 512 samples and at the end of every block), one lane per VFO at the full input rate, then the plan's stages as plain FIRs.
 *     Reproduces the reference's phase sequence — IF and SSB parity ~1e-7 for any run length — at a few times real time instead of
 *     thousands: a parity mode.  Set sdrpp_set_reference_block as well: the renormalisation points are the reference's block ends.
 *     Why there is no third, "re-seeded" mode (closed form inside a reference block, phase re-seeded from the recursion's value at every block
 *     end): the block-end phases ARE the recursion — N dependent float multiply-adds per block and VFO whatever is done with the samples, and a
 *     dependent packed multiply + add is 21 cycles on this SIMD (tools/probe/chain_latency_probe.hip), i.e. <= 115 MS/s for ANY scheme that
 *     follows the reference's phase sequence; the reference-rotator kernel runs at 26 cycles per sample (cfg 4: 67-69 MS/s with every SSB channel
 *     exact), so the re-seeded form could gain at most 1.2x while giving up exactness inside the block (its error would saw-tooth to ~1.7e-5 per
 *     307 200-sample block unless the drift were interpolated as well).  Not built; the numbers are in DESIGN.md 5.
 * Can only be changed while the context has no VFO. */
#define SDRPP_NCO_CLOSED_FORM 0
#define SDRPP_NCO_REFERENCE_ROTATOR 1
int sdrpp_set_nco_mode(sdrpp_ctx* ctx, int mode);
/* How the per-VFO filters behind the front end are launched for FM VFOs (WFM / NFM: last decimator -> resampler -> channel filter ->
 * discriminator + audio low-pass; the chain of rx_vfo.h:20-66 + demod/broadcast_fm.h, demod/fm.h).
 *   on (default): as ONE launch where that pays — the four stages run as a pipeline inside a workgroup, the streams between them stay in
 *     LDS (csrc/pipe_kernels.h); the library decides push by push (large pushes and launch-bound small ones).
 *   off: one launch per stage, intermediate streams in HBM.
 * Results are bit-identical either way (same tap tables, same summation order); a switch for measurements and for the test that says so
 * (on >= 2, a test hook: always pipelined, `on` segments per VFO). */
int sdrpp_set_backend_pipeline(sdrpp_ctx* ctx, int on);

/* ---- FFT -> log-power -> waterfall line (replaces Reshaper + Handler + IQFrontEnd::handler, iq_frontend.cpp:248-309,
 *      and WaterFall::pushFFT's doZoom + palette index, waterfall.cpp:65-90, 889-906) --------------------------------------- */
/* Numerics: the reference links libfftw3f / libvolk, neither of which is part of its tree (unpinned distro packages), so "bit-exact" for
 * this branch is defined against a fully specified float32 FFT + log2 that the test oracle and these kernels
 * share operation for operation; against a float64 DFT it is accurate to < 4e-7 relative (tests/test_oracle_kat.py), i.e. palette
 * indices agree with ANY correct FFT to +-1 of 10^6 levels.
 * fft_size: power of two 1024..1048576.  Frame k covers stream samples [k*(nz+skip), k*(nz+skip)+nz) since the last
 * configure/reset (reshaper.h:101-128); fftIn[nz:fft_size] is zero (iq_frontend.cpp:301).  `window` has nz floats.
 * Reconfiguring drops the partial frame, like updateFFTPath's tempStop/tempStart. */
int sdrpp_fft_configure(sdrpp_ctx* ctx, int fft_size, int nz, int skip, const float* window);
int sdrpp_fft_disable(sdrpp_ctx* ctx);
/* doZoom(draw_data_start, draw_data_size, fft_size, data_width) then palette index
 * (int)((clamp(v, wf_min, wf_max) - wf_min) / (wf_max - wf_min) * 999999).  data_width = 0 disables the zoomed outputs. */
int sdrpp_fft_set_view(sdrpp_ctx* ctx, int draw_data_start, int draw_data_size, int data_width, float wf_min, float wf_max);
/* Lines produced by the most recent push (each overwrites the previous push's). */
int sdrpp_fft_lines(sdrpp_ctx* ctx);
/* Copy line `first`..`first+n-1` of the last push to host memory: raw dB lines (fft_size floats each, DC-centred — what
 * acquireFFTBuffer/releaseFFTBuffer hand to the waterfall), zoomed lines (data_width floats) and palette indices.
 * Any destination may be NULL.  Returns the number of lines copied. */
int sdrpp_fft_read(sdrpp_ctx* ctx, int first, int n, float* raw_host, float* zoomed_host, int32_t* index_host);
/* Same, but into DEVICE memory of the caller (asynchronous D2D copies on the context's stream) — e.g. torch tensors that
 * are then handed to an RCCL gather of waterfall lines. */
int sdrpp_fft_copy_device(sdrpp_ctx* ctx, int first, int n, float* raw_dev, float* zoomed_dev, int32_t* index_dev);
/* Device pointers to the same buffers (valid until the next push). */
int sdrpp_fft_device_buffers(sdrpp_ctx* ctx, const float** raw, const float** zoomed, const int32_t** index, int* n_lines);

/* ---- VFO bank (replaces Splitter fan-out + N x RxVFO + radio demodulators) --------------------------------------------------- */
#define SDRPP_MAX_DECIM_STAGES 4

enum sdrpp_demod_mode {
    SDRPP_DEMOD_RAW = -1, /* no demodulator: output = RxVFO::out (complex IF)                                        */
    SDRPP_DEMOD_WFM = 0,  /* dsp::demod::BroadcastFM mono branch (broadcast_fm.h:146,205-211)                        */
    SDRPP_DEMOD_NFM = 1,  /* dsp::demod::FM<stereo_t> (fm.h:79-96)                                                   */
    SDRPP_DEMOD_AM = 2,   /* dsp::demod::AM<stereo_t> (am.h:101-133)                                                 */
    SDRPP_DEMOD_USB = 3,  /* dsp::demod::SSB<stereo_t> (ssb.h:77-92)                                                 */
    SDRPP_DEMOD_LSB = 4,
    SDRPP_DEMOD_DSB = 5,
    SDRPP_DEMOD_CW = 6    /* dsp::demod::CW<stereo_t> (cw.h:17-29, 57-68): statement for statement SSB(USB, bandwidth = 2 * tone) — one translation by
                           * `tone`, ComplexToReal, loop::AGC, MonoToStereo (ssb.h:23-35, 77-92, 106-108).  The tone's increment travels in
                           * ssb_phase_delta_re/im: sdrpp_design_phase_delta(tone, if_rate).  The radio module runs it at 3 kS/s (demodulators/cw.h:82). */
};

typedef struct sdrpp_vfo_desc {
    /* FrequencyXlator (frequency_xlator.h:14-30): phaseDelta for -offset at the input rate */
    float phase_delta_re, phase_delta_im;
    /* PowerDecimator (power_decimator.h:93-111): stages of the chosen plan, in order; n_stages = 0 for ratio 1 */
    int n_stages;
    int stage_decim[SDRPP_MAX_DECIM_STAGES];
    int stage_ntaps[SDRPP_MAX_DECIM_STAGES];
    const float* stage_taps[SDRPP_MAX_DECIM_STAGES];
    /* PolyphaseResampler (polyphase_resampler.h:69-99): interp == decim -> stage absent; taps already scaled by interp */
    int interp, decim;
    int resamp_ntaps;
    const float* resamp_taps;
    /* RxVFO channel filter (rx_vfo.h:95-98, 117-121); chan_ntaps = 0 when bandwidth == out rate (filterNeeded false) */
    int chan_ntaps;
    const float* chan_taps;
    /* demodulator */
    int demod;                /* enum sdrpp_demod_mode */
    float inv_deviation;      /* Quadrature::_invDeviation = 1/hzToRads(deviation, if_rate) (quadrature.h:19-26)         */
    int audio_ntaps;          /* WFM alFir / NFM fir / AM lpf real taps; 0 = filter bypassed (fm.h:88, broadcast_fm.h:205) */
    const float* audio_taps;
    /* loop::AGC (agc.h:15-27), used by AM (audio or carrier AGC), SSB and CW */
    float agc_set_point, agc_attack, agc_decay, agc_max_gain, agc_max_output_amp, agc_init_gain;
    int am_carrier_agc;       /* AM: 1 = AGCMode::CARRIER, 0 = AGCMode::AUDIO (am.h:14-17)                               */
    float dc_block_rate;      /* AM: DCBlocker rate (am.h:32 -> dc_blocker.h:54-60)                                       */
    float ssb_phase_delta_re, ssb_phase_delta_im; /* SSB second xlator (ssb.h:24,106-117); CW: the tone's (cw.h:20,28)     */
    /* NCO of THIS VFO: 0 = the context's mode (sdrpp_set_nco_mode), 1 = closed form, 2 = the reference's float rotator recursion.
     * FM and AM do not see the difference (no output depends on the absolute phase); a product detector (SSB) and the raw IF follow
     * the reference's own rounding drift only with the recursion, which costs a sequential pass over the full-rate stream — so a bank
     * can keep its FM / AM channels on the fast path and pay for exactness where it shows. */
    int nco_mode;
} sdrpp_vfo_desc;

/* IQFrontEnd::addVFO / removeVFO (iq_frontend.cpp:140-183).  Arrays in `desc` are copied.  *id receives a handle. */
int sdrpp_vfo_add(sdrpp_ctx* ctx, const sdrpp_vfo_desc* desc, int* id);
int sdrpp_vfo_remove(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_count(sdrpp_ctx* ctx);
/* RxVFO::setInSamplerate / setOutSamplerate (rx_vfo.h:35-58) — and with them IQFrontEnd::setSampleRate / setDecimation (iq_frontend.cpp:76-123) and
 * the radio module's demodulator switch (vfo_manager.cpp:52, radio_module.h:419-563): the VFO is described anew (`desc`: new plan, new taps), the
 * old handle dies, *new_id takes its place — and what the reference's objects carry across such a change is carried here:
 *   keep & 1: the RxVFO's own state — the translation's phase (FrequencyXlator::setOffset swaps phaseDelta only) and the channel filter's delay line
 *             (FIR::setTaps moves it under the new tap count, fir.h:31-52; a filter bypassed under the new settings keeps it for when it wakes up).
 *             The decimator stages and the polyphase resampler start from cleared state, as the reference re-creates / resets them
 *             (power_decimator.h:91-108, polyphase_resampler.h:38-67).
 *   keep & 2: the demodulator behind it lives on (setInSamplerate: the radio's demodulator block is not touched): discriminator and audio low-pass
 *             history, AGC / DC-blocker state, SSB's second translation (CW -> CW: the tone translation's phase).  Only where the new description has
 *             the same demodulator; a demodulator SWITCH creates a new demodulator object in the reference too: leave the bit off.  The AGC's amplitude
 *             estimate lives on while its attack / decay follow the NEW description (AGC::setAttack / setDecay, agc.h:31-43, swap the coefficients only).
 *   keep & 4: the IF chain (sdrpp_vfo_set_if, sdrpp_vfo_set_fmnr) moves to the new handle with its parameters, the blanker's amplitude estimate and FMIF's delay line: the radio module's
 *             IF-chain blocks are not the demodulator's and outlive a demodulator switch (radio_module.h:84-96).  Without the bit the new handle has no chain.
 * An AF chain (sdrpp_vfo_set_af) is not carried over: attach it to the new handle (it starts cleared, as afChain's blocks do after a restart). */
int sdrpp_vfo_replace(sdrpp_ctx* ctx, int old_id, const sdrpp_vfo_desc* desc, int keep, int* new_id);
/* RxVFO::setOffset (rx_vfo.h:72-77): only phaseDelta changes, phase stays continuous; the samples already inside the first
 * decimator's delay line keep their old rotation (the first outputs after the change are handed over sample-exactly). */
int sdrpp_vfo_set_phase_delta(sdrpp_ctx* ctx, int id, float re, float im);
/* SSB::setBandwidth / setMode (ssb.h:44-62, 106-117): the second translation's increment follows bandwidth / 2; phase continuous.
 * CW::setTone (dsp/demod/cw.h:31-36) is the same call with sdrpp_design_phase_delta(tone, if_rate): FrequencyXlator::setOffset, phase continuous. */
int sdrpp_vfo_set_ssb_phase_delta(sdrpp_ctx* ctx, int id, float re, float im);
/* RxVFO::setBandwidth (rx_vfo.h:60-70): swap the channel-filter taps, history kept (fir.h:31-52). n = 0 bypasses.  The delay line is sized from the
 * tap count (CW's 50 Hz channel at 3 kS/s has 4 560 taps); more than 65 536 taps are refused (SDRPP_ERR_UNSUPPORTED), here and in sdrpp_vfo_add. */
int sdrpp_vfo_set_channel_taps(sdrpp_ctx* ctx, int id, const float* taps, int n);
/* RxVFO::reset + demod reset: clears histories, NCO phase and loop states. */
int sdrpp_vfo_reset(sdrpp_ctx* ctx, int id);
/* Output of the most recent push: number of samples (stereo frames, or complex IF samples in RAW mode). */
int sdrpp_vfo_out_count(sdrpp_ctx* ctx, int id);
/* Copy up to max samples (2 floats each) to host memory; returns the count copied (what RxVFO::run/demod swap()). */
int sdrpp_vfo_read(sdrpp_ctx* ctx, int id, float* dst_host, int max);
/* The same for many VFOs with ONE device-to-host copy (a host block that delivers every VFO stream after each block would otherwise
 * pay one small copy + synchronisation per VFO).  which[i]: 0 = what sdrpp_vfo_read returns, 1 = the complex IF, 2 = the AF chain
 * output, 3 = the IF chain's output (sdrpp_vfo_set_if) (NULL: all 0).  The blocks are packed back to back into dst_host (2 floats per sample); offsets[i] / counts[i] (in samples)
 * locate VFO ids[i]'s block.  Returns the total number of samples, SDRPP_ERR_INVALID if max_samples is too small.  dst_host = NULL is
 * a size query: offsets / counts are filled and the total returned, nothing is copied. */
int sdrpp_vfo_read_many(sdrpp_ctx* ctx, int n, const int* ids, const int* which, float* dst_host, int64_t max_samples, int64_t* offsets, int* counts);
/* Device pointers: demodulated audio (or IF in RAW mode) and the complex IF stream (RxVFO::out) of the last push. */
int sdrpp_vfo_device_buffers(sdrpp_ctx* ctx, int id, const float** out, int* n_out, const float** if_out, int* n_if);

/* ---- radio AF chain behind a demodulating VFO (decoder_modules/radio/src/radio_module.h:98-110, 540-547) ------
 * RationalResampler<stereo_t> (demodulator AF rate -> audio rate: power-of-two pre-decimation plan + L/M polyphase,
 * rational_resampler.h:80-165) -> FIR<stereo_t,float> high-pass (radio_module.h:103,597; optional) -> Deemphasis<stereo_t>
 * (filter/deephasis.h:58-77; optional).  Attached to an existing VFO; its output replaces nothing: the demodulator output
 * (sdrpp_vfo_read) stays available, the AF output has its own accessors. */
typedef struct sdrpp_af_desc {
    int n_stages;                                     /* PowerDecimator stages of the pre-decimation plan (0: ratio 1)        */
    int stage_decim[SDRPP_MAX_DECIM_STAGES];
    int stage_ntaps[SDRPP_MAX_DECIM_STAGES];
    const float* stage_taps[SDRPP_MAX_DECIM_STAGES];
    int interp, decim;                                /* polyphase L/M; interp == decim -> stage absent                         */
    int resamp_ntaps;
    const float* resamp_taps;                         /* already scaled by interp (sdrpp_design_resampler)                      */
    int hpf_ntaps;                                    /* 0 = high-pass block disabled; at most 65 536 taps (SDRPP_ERR_UNSUPPORTED) */
    const float* hpf_taps;
    float deemph_alpha;                               /* 0 = de-emphasis block disabled (sdrpp_design_deemphasis_alpha)         */
} sdrpp_af_desc;
/* afChain.enableBlock / setAudioSampleRate (radio_module.h:540-547, 585-600).  af == NULL detaches.  Arrays are copied; the chain
 * starts from cleared state.  Only for VFOs with a demodulator (demod != RAW).  The high-pass is not bound by the channel filter's 4 096 taps
 * (highPass(300, 100, rate) has 7 296 at 192 kHz): its delay line is sized from hpf_ntaps; more than 65 536 taps are refused with
 * SDRPP_ERR_UNSUPPORTED and the tap count in the message. */
int sdrpp_vfo_set_af(sdrpp_ctx* ctx, int id, const sdrpp_af_desc* af);
/* AF output of the most recent push: stereo frames at the audio rate (what afChain.out swap()s to the sink stream). */
int sdrpp_vfo_af_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_af_read(sdrpp_ctx* ctx, int id, float* dst_host, int max);
int sdrpp_vfo_af_device_buffer(sdrpp_ctx* ctx, int id, const float** out, int* n_out);
int sdrpp_abi_sizeof_af_desc(void);

/* ---- radio IF chain between a VFO's IF stream and its demodulator (decoder_modules/radio/src/radio_module.h:84-96) ------------------
 * NoiseBlanker (dsp/noise_reduction/noise_blanker.h:38-57) -> PowerSquelch (dsp/noise_reduction/power_squelch.h:33-50), in that order,
 * on the complex IF; the demodulator (and the AF chain behind it) then reads the chain's output.  RxVFO::out itself (`if_out`, which = 1)
 * stays the stream IN FRONT of the chain, as vfo->output is in the reference; the chain's own output of the last push has its accessors
 * below and is which = 3.  A RAW VFO with a chain delivers the chain's output as its `out`.
 *   blanker: per sample, state amp (1 when the blanker starts, sdrpp_vfo_reset sets it back): inAmp = |x|; if inAmp != 0 { amp = amp * (1 -
 *            nb_rate) + inAmp * nb_rate; excess = inAmp / amp; if excess > nb_level: x /= excess }.  The radio module uses nb_rate = 500 / IF rate.
 *   squelch: per REFERENCE BLOCK (sdrpp_set_reference_block; 0: one push = one block) of the blanker's output: the block passes if
 *            10 * log10(mean |x|) >= squelch_level, else it is zeroed.  No state.
 * Calling it on a VFO that has a chain changes the parameters and keeps amp (setRate / setLevel keep it); a blanker switched from off to
 * on starts at amp = 1.  desc == NULL detaches.  With both blocks disabled, or without a chain, nothing is planned for it: every path is
 * what it is without this call.  VFOs with an active chain do not take part in the one-launch FM back end (sdrpp_set_backend_pipeline).
 * FMIF, the third block of the reference's chain, has a call of its own (sdrpp_vfo_set_fmnr below); sdrpp_vfo_set_if leaves it alone.
 * Not covered: the AF-side CTCSS squelch. */
typedef struct sdrpp_if_desc {
    int nb_enabled;
    float nb_rate, nb_level;
    int squelch_enabled;
    float squelch_level;                              /* dB                                                                      */
} sdrpp_if_desc;
int sdrpp_vfo_set_if(sdrpp_ctx* ctx, int id, const sdrpp_if_desc* desc);
int sdrpp_vfo_ifc_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_ifc_read(sdrpp_ctx* ctx, int id, float* dst_host, int max);
int sdrpp_vfo_ifc_device_buffer(sdrpp_ctx* ctx, int id, const float** out, int* n_out);
int sdrpp_abi_sizeof_if_desc(void);
/* FMIF, the radio's "IF Noise Reduction" (dsp/noise_reduction/fm_if.h:45-77), the LAST block of the chain: blanker -> squelch -> FMIF ->
 * demodulator.  For every IF sample i, with N = bins and the window w[n] = (float)nuttall(n, N - 1):
 *     X_i[k] = sum_n w[n] * x[i - (N-1) + n] * e^{-j 2 pi k n / N},   idx = first k of maximal sqrtf(re^2 + im^2),
 *     out[i] = X_i[idx] * e^{+j 2 pi idx (N / 2) / N}    (integer N / 2: what the un-normalised backward DFT of that single bin holds at index N / 2)
 * The radio module's presets are 9, 15, 31 and 32 bins (radio_module.h:31-36); any bins in 2 .. 32 is taken (more: SDRPP_ERR_UNSUPPORTED).
 * It reads the blanker / squelch output while one of them runs, else RxVFO::out, and writes the chain's output (which = 3, sdrpp_vfo_ifc_*, a
 * RAW VFO's `out`; the demodulator reads it).  A chain that consists of FMIF alone is an active chain.
 * State: the delay line of N - 1 samples, zero at the start.  Changing `bins` clears it (setBins); enabled = 0 only unplugs the block — the bin
 * count is recorded, nothing runs, and switching it on again with the same bins continues from the delay line as it was left; sdrpp_vfo_reset
 * clears it; sdrpp_vfo_replace with keep & 4 moves bins, the switch and the delay line to the new handle with the rest of the chain.
 * Numerics: the reference links whatever libfftw3f is installed, so (as for the waterfall branch) "the reference" is its control flow around an
 * EXACT DFT.  Here window, DFT and output twiddle are one matrix designed in double and rounded to float, applied on the FP32 matrix cores: an
 * output is within 1e-5 * sum_n w[n] * |x[i - (N-1) + n]| of that definition (each part a sum of 2 N products of float-rounded factors:
 * (2 N + 2) * 2^-24 * sqrt(2) = 5.6e-6 at N = 32; measured on an MI355X over the streams of tests/test_fmif.py: at most 4.2e-7).  Among bins of EQUAL float magnitude the lowest wins, as in the reference; where the two
 * largest magnitudes differ by less than the rounding of either (a few samples per thousand on FM signals, and the first windows after a
 * cleared delay line, where every bin is equal) the neighbouring bin may win, and the output then is that bin's value.
 * The results do not depend on how the stream is cut into pushes, launch groups or pipelined blocks. */
int sdrpp_vfo_set_fmnr(sdrpp_ctx* ctx, int id, int enabled, int bins);

/* ---- sink-side sample packing: float -> int16 / int8 on the device, before the copy to the host -----------------
 * `which`: 0 = what sdrpp_vfo_read returns (demodulator output, or the IF in RAW mode), 1 = the complex IF (RxVFO::out), 2 = the AF
 * chain output.  pcm_type follows dsp/compression/pcm_type.h: 0 = I8, 1 = I16, 2 = F32.
 * sdrpp_vfo_read_pcm: VOLK's volk_32f_s32f_convert_16i / _8i with the caller's scale (the recorder writes int16 WAV with 32767,
 *   utils/wav.cpp:166); returns frames.  sdrpp_vfo_read_compressed: one SDR++-server frame exactly as
 *   SampleStreamCompressor::process builds it (sample_stream_compressor.h:30-62): [u16 0][u16 pcm_type][f32 scaler][data], scaler =
 *   the largest VALUE of the block, data scaled by 128 / scaler or 32768 / scaler; returns bytes (0 for an empty block). */
int sdrpp_vfo_read_pcm(sdrpp_ctx* ctx, int id, int which, int pcm_type, float scale, void* dst_host, int max_frames);
/* The same conversion for the pre-processed wideband IQ of the most recent push (sdrpp_preproc_read's samples): what the recorder's baseband
 * mode writes from its bindIQStream consumer (recorder/src/main.cpp:209, 528-530 -> wav::Writer::write, utils/wav.cpp:158-167); returns
 * complex samples (2 values each). */
int sdrpp_preproc_read_pcm(sdrpp_ctx* ctx, int pcm_type, float scale, void* dst_host, int max_samples);
int sdrpp_vfo_read_compressed(sdrpp_ctx* ctx, int id, int which, int pcm_type, unsigned char* dst_host, int max_bytes);

/* ---- recorder sink behind a demodulating VFO (misc_modules/recorder) ---------------------------------------------------
 * What the recorder module does to a radio's audio stream, block by block, on the device:
 *   dsp::audio::Volume (audio/volume.h:14,22,37)            v = x * g per value, g = powf(volume, 2) computed once on the host as a float
 *   dsp::bench::PeakLevelMeter<stereo_t> (peak_level_meter.h:52-57)   peak |v.l|, |v.r| of the block (the host keeps the running maximum and resets it)
 *   dsp::convert::StereoToMono (stereo_to_mono.h:13-15), optional      m = (v.l + v.r) / 2.0f
 *   wav::Writer::write (utils/wav.cpp:158-180) in the file's sample type, wav::SampleType numbering (utils/wav.h:25-30):
 *     1 INT16    VOLK generic volk_32f_s32f_convert_16i(.., 32767.0f): s * 32767.0f, clamped to [-32768, 32767], rintf, cast
 *     0 UINT8    (uint8_t)((s * 127.0f) + 128.0f): the product, then the sum, then truncation toward zero.  The reference's cast is UNDEFINED where that
 *                float lies outside [0, 256): OUR DEFINITION there is saturation — 255 from 255.0 up, 0 from 0.0 down
 *     3 FLOAT32  the floats as they are
 *     2 INT32    NOT IMPLEMENTED (SDRPP_ERR_UNSUPPORTED), on purpose: VOLK's generic volk_32f_s32f_convert_32i clamps at 2147483647.0f, which as a float
 *                is 2^31, so the cast of a clipped sample overflows int32 and the reference's own value is undefined; there is nothing to be exact against
 *   "ignore silence" (recorder/src/main.cpp:28, 533-561): a block whose absolute maximum over the values that would be written is below SILENCE_LVL
 *     (the float compared with the double 10e-6) is not written at all.  `silent` only REPORTS that decision: the block's bytes are delivered all the
 *     same, `frames` stays the block's frame count, and the host skips the block.
 * Every product and sum is rounded on its own (nothing contracts into a fused multiply-add), so every byte and every figure of the record is a bit-exact
 * function of the float frames the same block delivers (sdrpp_vfo_read / sdrpp_vfo_af_read, result flag 1).
 * SOURCE: the end of the VFO's chain, i.e. what result flag 1 delivers for it — the AF chain's output where one is attached, else the demodulator's
 * output; sdrpp_vfo_set_af attaching or detaching moves what the sink reads.  Only for VFOs with a demodulator (RAW: SDRPP_ERR_UNSUPPORTED).
 * A BLOCK is one push; outside pipelined mode with deferred processing on it is the whole pass (the silence decision and the peaks then cover all the
 * staged pushes together; a decision per staged push is not offered).  An empty block (0 frames) gives frames = 0, peaks and abs_max 0, silent = 0.
 * The sink has NO streaming state: calling sdrpp_vfo_set_rec again only changes the parameters, from the next block on (blocks already pushed in
 * pipelined mode keep the parameters they were pushed with); desc == NULL detaches.  sdrpp_vfo_replace does not carry the sink over — like the AF
 * chain the host re-attaches it: the reference's recorder binds to the sink stream, not to the VFO. */
#define SDRPP_REC_UINT8 0     /* wav::SAMP_TYPE_UINT8                                                                                   */
#define SDRPP_REC_INT16 1     /* wav::SAMP_TYPE_INT16                                                                                   */
#define SDRPP_REC_INT32 2     /* wav::SAMP_TYPE_INT32: refused                                                                          */
#define SDRPP_REC_FLOAT32 3   /* wav::SAMP_TYPE_FLOAT32                                                                                 */
typedef struct sdrpp_rec_desc {
    float volume;         /* the slider value; the gain applied is powf(volume, 2)                                                 */
    int mono;             /* 1: StereoToMono behind the volume                                                                      */
    int sample_type;      /* SDRPP_REC_UINT8 / _INT16 / _FLOAT32; SDRPP_REC_INT32: SDRPP_ERR_UNSUPPORTED; anything else: SDRPP_ERR_INVALID */
    int ignore_silence;
} sdrpp_rec_desc;
typedef struct sdrpp_rec_info {
    int frames, channels, sample_type;   /* of the block as it was converted: frames * channels samples of sample_type                */
    int silent;           /* 1: ignore_silence is on and (double)abs_max < 10e-6 — the reference writes nothing for this block     */
    float peak_l, peak_r; /* PeakLevelMeter of THIS block: max fabsf of the volume's output per channel (in front of the mono fold)  */
    float abs_max;        /* max fabsf over the values that would be written (both channels, or the mono stream), before conversion */
} sdrpp_rec_info;
int sdrpp_vfo_set_rec(sdrpp_ctx* ctx, int id, const sdrpp_rec_desc* desc);
/* The most recent push (pass) through the sink: up to max_frames frames of packed samples to dst_host (may be NULL with max_frames = 0), the record
 * of the WHOLE block to *info (may be NULL); returns the frames copied.  SDRPP_ERR_INVALID for a VFO without a sink. */
int sdrpp_vfo_rec_read(sdrpp_ctx* ctx, int id, void* dst_host, int max_frames, sdrpp_rec_info* info);
int sdrpp_abi_sizeof_rec_desc(void);

/* ---- RDS branch of the WFM demodulator (dsp/demod/broadcast_fm.h:144-215 with _rdsOut on; decoder_modules/radio/src/demodulators/wfm.h:79) --------------
 * The 5 kS/s complex baseband the radio's RDSDemod consumes, as dsp::demod::BroadcastFM makes it from the IF stream, feed-forward throughout:
 *     d[i]   = Quadrature(x[i])                          the discriminator, the same values the audio low-pass reads (quadrature.h:39-46)
 *     c[i]   = (d[i] + 0j) * phase;  phase *= delta      FrequencyXlator(-57000, IF rate) (channel/frequency_xlator.h:43-50)
 *     rdsout = RationalResampler<complex_t>(IF rate -> 5000)(c)     (rational_resampler.h:120-165: at 250 kS/s the stored ratio-32 plan
 *              {8 x 44 taps, 2 x 12, 2 x 69}, then the 5000 / 7813 polyphase stage, 593 750 taps, 119 per phase)
 * Every filter is designed on the host (sdrpp_design_phase_delta, the stored decimation plan, sdrpp_design_resampler); the arrays are copied.
 * What becomes of the baseband — RDSDemod's AGC, Costas loops and clock recovery — runs on the device as well, as a block of its own behind this one
 * (sdrpp_vfo_set_rds_demod, source 0); only the group decoder, which reads bits, stays on the host.  Giving the branch another description, or detaching
 * it, detaches a demodulator behind it.
 * Only for SDRPP_DEMOD_WFM VFOs (anything else: SDRPP_ERR_UNSUPPORTED); bad stage or polyphase descriptions give the errors sdrpp_vfo_set_af gives;
 * the first stage must decimate (n_stages >= 1) and its window must fit the kernel's tile (SDRPP_ERR_UNSUPPORTED otherwise: every plan of the
 * reference up to ratio 32 with at most 128 taps does).
 * SOURCE: what the demodulator reads — the IF chain's output where a chain is active, else RxVFO::out.  The discriminator values are recomputed from
 * that stream and its history by the device routine the audio path uses; the branch never changes a bit of the VFO's audio, IF, AF, recorder or
 * meter outputs.  DEVIATION from the reference: BroadcastFM::setRDSOut also clears the discriminator and the audio filter (one click in the
 * audio); here switching the branch leaves the audio path alone.
 * STATE, as the reference keeps it in `xlator` and `rdsResamp`: the rotator's phase, the delay lines, the decimators' offsets and the polyphase
 * phase.  Attaching starts from a fresh BroadcastFM: phase (1, 0), cleared delay lines, offsets and phase 0.  enabled = 0 unplugs the branch and
 * freezes all of it — nothing is planned, nothing delivered, nothing advances; enabled = 1 with the SAME description continues from there.  A call
 * with another description starts cleared.  desc == NULL detaches.  sdrpp_vfo_reset leaves the branch's own state alone, as BroadcastFM::reset and
 * RxVFO::reset do (the IF history it clears is the discriminator's "previous phase 0").  sdrpp_vfo_replace with keep & 2 and a WFM description
 * moves the branch, parameters and state, to the new handle (it belongs to the demodulator object; where the new description runs the other NCO mode
 * the parameters move and the branch starts cleared); otherwise the new handle has none.
 * NCO: closed form, the phase arg(phase_delta) * n evaluated in float64 and anchored per push like SSB's second translation; a launch group is
 * anchored push by push, so grouped results equal ungrouped ones bit for bit.  Against the reference's float recursion (renormalised every 512
 * samples) the closed form differs by the recursion's own drift: 4.7e-6, 5.3e-6 and 9.5e-6 of the output RMS over the first 12 500, 50 000 and
 * 200 000 IF samples (1.5e-5 over the last tenth of the longest; computed on the CPU between the two yardsticks of tests/test_rds.py, profiles/rds_rate.md)
 * — the closed form stands for the reference within the project's 1e-5 for about the first 0.8 s of a stream, and for an exact NCO throughout.
 * Where the VFO runs the reference rotator (nco_mode = 2, or the context's mode when the branch is attached) the branch runs the reference's float
 * recursion at the IF rate — renormalised every 512 samples and at the reference-block ends (sdrpp_set_reference_block) carried down to the IF rate —
 * writes the rotated stream, and its first decimator follows as a plain FIR: results then do not depend on the cut as long as the blocks are the same.
 * The polyphase bank (2.4 MB at 5000 / 7813) exists ONCE per context for identical descriptions, however many VFOs carry the branch.
 * Outside pipelined mode the accessors below name the most recent push, as the AF chain's do: SDRPP_ERR_INVALID for a VFO without a branch
 * (count 0 while it is switched off).  Pipelined: sdrpp_pipeline_set_rds_results / sdrpp_result_rds. */
typedef struct sdrpp_rds_desc {
    float phase_delta_re, phase_delta_im;             /* sdrpp_design_phase_delta(-57000, if_rate)                              */
    int n_stages;                                     /* PowerDecimator stages of the pre-decimation plan (>= 1)                */
    int stage_decim[SDRPP_MAX_DECIM_STAGES];
    int stage_ntaps[SDRPP_MAX_DECIM_STAGES];
    const float* stage_taps[SDRPP_MAX_DECIM_STAGES];
    int interp, decim;                                /* polyphase L/M; interp == decim -> stage absent                         */
    int resamp_ntaps;
    const float* resamp_taps;                         /* already scaled by interp (sdrpp_design_resampler(if_rate, 5000, ...))  */
} sdrpp_rds_desc;
int sdrpp_vfo_set_rds(sdrpp_ctx* ctx, int id, const sdrpp_rds_desc* desc, int enabled);
/* The branch's output of the most recent push: complex samples at 5 kS/s (what BroadcastFM::rdsOut swap()s). */
int sdrpp_vfo_rds_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_rds_read(sdrpp_ctx* ctx, int id, float* dst_host, int max);
int sdrpp_vfo_rds_device_buffer(sdrpp_ctx* ctx, int id, const float** out, int* n_out);
int sdrpp_abi_sizeof_rds_desc(void);
/* Test and statistics hook: polyphase banks of RDS branches the context holds in device memory (identical descriptions share one). */
int sdrpp_rds_bank_count(sdrpp_ctx* ctx);

/* ---- Stereo branch of the WFM demodulator (dsp/demod/broadcast_fm.h:147-191 with _stereo on; decoder_modules/radio/src/demodulators/wfm.h `_stereo`) --------
 * What dsp::demod::BroadcastFM computes per IF sample i with its stereo decoder on:
 *     m[i]  = Quadrature(x[i])                                  the discriminator the mono path has
 *     p[i]  = FIR<complex_t, complex_t>(m[i] + 0j)              pilot_taps: taps::bandPass<complex_t>(18750, 19250, 3000, if_rate, true), 317 taps at 250 kS/s
 *     v[i]  = phasor(phase)                                     loop::PLL (pll.h:64-70): the phase BEFORE the update
 *     e     = normalizePhase(atan2f(p.im, p.re) - phase);  freq += beta * e, clamped to [min_freq, max_freq];  phase += freq + alpha * e, wrapped to +-pi
 *     q     = (m[i - delay] + 0j) * conj(v) * conj(v);  lmr = 2 q.re;  l = m[i - delay] + lmr,  r = m[i - delay] - lmr
 *     out   = (alFir(l), arFir(r))                              the VFO description's audio taps; audio_ntaps == 0: no filter (`_lowPass` off)
 * in float throughout, the loop in the reference's operations and order.  The result does not depend on how the stream is cut into pushes: the same
 * samples give the same bits in one push, in pushes of one sample, pipelined or in launch groups.  The (l, r) frames are the VFO's output: the AF chain,
 * the recorder sink, sdrpp_vfo_read and the pipelined results read them as they read the mono frames.
 * Only for SDRPP_DEMOD_WFM VFOs (anything else: SDRPP_ERR_UNSUPPORTED).  SDRPP_ERR_INVALID: no taps, an even tap count, a delay below 1 — and a loop
 * description outside these limits, which bound the phase step so that the loop's wrap into +-pi ends after at most two rounds: alpha, beta, init_freq,
 * min_freq and max_freq finite; min_freq < max_freq; |min_freq|, |max_freq|, |init_freq| <= pi; |alpha| * pi + max(|min_freq|, |max_freq|) <= 4 pi (the
 * reference's description: 0.48 + 0.25 pi).  SDRPP_ERR_UNSUPPORTED: more than 576 pilot taps, or a VFO whose audio low-pass has more than 289 (the kernels' tiles).
 * SWITCHING is BroadcastFM::setStereo, which calls reset(): a call that changes `enabled` — or attaches an enabled branch, replaces the description of an
 * enabled one, or detaches an enabled one (desc == NULL) — makes the demodulator start over from the next sample: discriminator's previous phase 0, pilot
 * filter, both delays and both audio filters cleared, the loop at phase 0 and init_freq; the mono path likewise (its discriminator and audio filter
 * cleared).  RxVFO's own state, the IF chain's and the RDS branch's are not touched.  A call with the same description and the same `enabled` changes
 * nothing.  sdrpp_vfo_reset clears the branch with the rest of the demodulator.  sdrpp_vfo_replace with keep & 2 and a WFM description moves the branch,
 * parameters and state, to the new handle (a handle with another stream capacity or audio filter length gets the description attached afresh: with an
 * enabled branch its demodulator starts from the reset() state).
 * The arrays are copied during the call. */
typedef struct sdrpp_stereo_desc {
    const float* pilot_taps;      /* pilot_ntaps complex taps, interleaved (re, im): sdrpp_design_band_pass_complex(18750, 19250, 3000, if_rate, 1, ...) */
    int pilot_ntaps;              /* odd                                                                                                              */
    int delay;                    /* (pilot_ntaps - 1) / 2 + 1 (broadcast_fm.h:47-48)                                                                 */
    float alpha, beta;            /* sdrpp_design_pll(25000 / if_rate, ...)  (broadcast_fm.h:46)                                                       */
    float init_freq;              /* (float)hzToRads(19000, if_rate), radians per sample                                                               */
    float min_freq, max_freq;     /* (float)hzToRads(18750 / 19250, if_rate)                                                                           */
    int enabled;
} sdrpp_stereo_desc;
int sdrpp_vfo_set_stereo(sdrpp_ctx* ctx, int id, const sdrpp_stereo_desc* desc);
int sdrpp_abi_sizeof_stereo_desc(void);

/* ---- Symbol branch of a RAW VFO: FSK discriminator -> shaping FIR -> Mueller-Mueller clock recovery -> soft symbols and bits ----------------------------
 * What the pager decoder's POCSAGDSP (decoder_modules/pager_decoder/src/pocsag/dsp.h) computes from its VFO's output:
 *     d[i]  = Quadrature(x[i]) = normalizePhase(phase(x[i]) - phase(x[i-1])) * inv_deviation          (demod/quadrature.h:39-46)
 *     f[i]  = FIR<float, float>(d)[i] = sum_k d[i - (K-1) + k] * shape_taps[k]                        (filter/fir.h; sums k-ascending, product and sum rounded apart)
 *     MM<float> (clock_recovery/mm.h:100-156), per symbol while offset < count:
 *         p     = clamp((int)floorf(phase * interp_phases), 0, interp_phases - 1)
 *         out   = sum_k f[offset - (T-1) + k] * interp_bank[p][k]         T = interp_ntaps; volk_32f_x2_dot_prod_32f in the generic order: k ascending
 *         error = clamp(step(lastOut) * out - lastOut * step(out), -1, 1);  lastOut = out               step(x) = x > 0 ? 1 : -1
 *         freq  = clamp(freq + omega_gain * error, min_omega, max_omega);  phase += freq + mu_gain * error      (PhaseControlLoop<float, false>::advance)
 *         delta = floorf(phase);  offset += delta;  phase -= delta
 *     after the loop offset -= count;  soft = out per symbol, bit = soft > 0.0f                         (digital/binary_slicer.h)
 * in float throughout, every operation of the recursion in the reference's order.  Built as a general block: the parameters come from the description
 * (sdrpp_design_pager fills the pager's), the input is the real stream f.
 * WHERE IT ATTACHES: only SDRPP_DEMOD_RAW VFOs — the pager's VFO has no demodulator; anything else: SDRPP_ERR_UNSUPPORTED.  SOURCE: what a demodulator
 * would read — the IF chain's output where a chain is active, else RxVFO::out.  The discriminator is the device routine the FM path and the RDS branch
 * call (|error| <= 3e-7 rad against atan2f: soft values are not the reference's bit for bit).  The branch never changes a bit of any other
 * output of the VFO.
 * SDRPP_ERR_INVALID: a parameter that is not finite; shape_ntaps outside 1 .. 64, interp_ntaps outside 1 .. 16, interp_phases outside 1 .. 1024, a missing
 * array; min_omega >= max_omega; and a loop whose step leaves these bounds: every step delta = floorf(phase + freq + mu_gain * error) with phase in [0, 1),
 * |error| <= 1 lies in [floorf(min_omega - |mu_gain|), max_omega + |mu_gain| + 1), and the branch demands
 *     min_omega - |mu_gain| >= 1       every symbol advances at least one sample: the walk ends, and a push of n samples yields at most
 *                                      ceil(n / floorf(min_omega - |mu_gain|)) + 1 symbols (the capacity of the outputs below; never less than the
 *                                      reference-typical ceil(n / min_omega) + 1)
 *     max_omega + |mu_gain| <= 4096    offsets stay far inside the range in which `offset += delta` (an int plus a float, mm.h:147) is exact for every
 *                                      push the context takes (max_push < 2^24 - 4097 samples at the branch's rate, else SDRPP_ERR_UNSUPPORTED)
 * (the reference's pager at 24 kS/s: mu_gain 1, omega 10 .. 46.9 +- 5 %).  The rule is stricter than "min_omega >= 1": with mu_gain = 1 a step of
 * floorf(min_omega - 1) = 0 would neither advance nor bound the output, so descriptions with 1 <= min_omega < 1 + |mu_gain| are refused although the
 * reference would run them.  The loop stages nothing: for a symbol at `offset` a lane reads the T samples ENDING there (mm.h:113 with bufStart = buffer +
 * T - 1) and the T taps of one interpolator phase straight from device memory, so no bound on the step follows from any chunk or overlap.
 * STATE, as the reference keeps it: the discriminator's previous phase, the FIR's delay line, MM's offset, pcl.phase, pcl.freq, lastOut and the T - 1
 * delay samples.  Attaching starts from a fresh POCSAGDSP: previous phase 0, phase 0, freq = omega, offset 0, lastOut 0, cleared lines.  enabled = 0
 * freezes all of it — nothing is planned, nothing delivered, nothing advances, whatever the VFO's stream does meanwhile; enabled = 1 with the SAME
 * description continues from there (the outputs equal an uninterrupted run over the pushes the branch was switched on for).  A call with another
 * description starts cleared.  desc == NULL detaches.  sdrpp_vfo_reset treats the branch as it treats the RDS branch: the discriminator's previous phase
 * becomes 0 with the IF history it clears, everything else the branch holds stays (the decoder is a block of its own behind the VFO; to start it over,
 * attach the description anew after a detach).  sdrpp_vfo_replace with keep & 2 and a RAW
 * description moves the branch, parameters and state, to the new handle (a handle with another stream capacity gets the description attached afresh,
 * cleared); otherwise the new handle has none.
 * The interpolator bank exists ONCE per context for identical banks, however many VFOs carry the branch (sdrpp_sym_bank_count).
 * OUTPUT of a push: the symbols whose start `offset` lies inside that push — the reference's `while (offset < count)` followed by `offset -= count` — so
 * the concatenated output does not depend on how the stream is cut: one push, pushes of a single sample, pipelined or in launch groups (where every push
 * keeps its own count and slice) give the same bits and the same soft values bit for bit.  Outside pipelined mode the accessors name the most recent push
 * (SDRPP_ERR_INVALID for a VFO without a branch, count 0 while it is switched off); each of them waits for the device and copies the counts to the host, because
 * the count is the loop's own result — a convenience for a few channels: a receiver with many reads them out of the pipelined results, which cost no wait.
 * Pipelined: sdrpp_pipeline_set_sym_results / sdrpp_result_sym.  The arrays are copied during the call. */
typedef struct sdrpp_sym_desc {
    float inv_deviation;              /* (float)(1.0 / hzToRads(deviation, if_rate)); negative for the pager (deviation -4500)  */
    int shape_ntaps;                  /* FIR<float, float> in front of the loop, 1 .. 64                                         */
    const float* shape_taps;
    float omega;                      /* samples per symbol: pcl.freq after init                                                 */
    float mu_gain, omega_gain;        /* pcl alpha, beta                                                                         */
    float min_omega, max_omega;       /* (float)(omega * (1 - lim)), (float)(omega * (1 + lim))                                  */
    int interp_phases, interp_ntaps;  /* 128, 8; the bank holds interp_phases * interp_ntaps floats                              */
    const float* interp_bank;         /* phase-major, as buildPolyphaseBank lays it out: sdrpp_design_mm_interp                  */
} sdrpp_sym_desc;
int sdrpp_vfo_set_symbols(sdrpp_ctx* ctx, int id, const sdrpp_sym_desc* desc, int enabled);
/* The branch's output of the most recent push: soft symbols and their bits (soft > 0.0f). */
int sdrpp_vfo_sym_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_sym_read(sdrpp_ctx* ctx, int id, float* soft_host, uint8_t* bits_host, int max);   /* either array may be NULL; returns the symbols copied */
int sdrpp_vfo_sym_device_buffers(sdrpp_ctx* ctx, int id, const float** soft, const uint8_t** bits, int* n);
int sdrpp_abi_sizeof_sym_desc(void);
/* Test and statistics hook: interpolator banks the context holds in device memory (identical banks share one). */
int sdrpp_sym_bank_count(sdrpp_ctx* ctx);
/* MM::generateInterpTaps (mm.h:173-178): windowedSinc(phases * ntaps, hzToRads(0.5 / phases, 1.0), nuttall, phases) through buildPolyphaseBank
 * (polyphase_bank.h:15-48), phase-major into bank[phases * ntaps]; bit for bit the reference's.  Returns phases * ntaps, or SDRPP_ERR_INVALID. */
int sdrpp_design_mm_interp(int phases, int ntaps, float* bank);
/* The scalars of POCSAGDSP::init(in, if_rate, baudrate) (pocsag/dsp.h:20-37) into *desc: inv_deviation for Quadrature(-4500, if_rate), omega = if_rate /
 * baudrate with MM's gains 1e-4 (omega) and 1.0 (mu) and relative limit 0.05, 128 x 8 interpolator, shape_ntaps = 10.  The two arrays stay the caller's:
 * ten taps of 0.1f and sdrpp_design_mm_interp(128, 8).  SDRPP_ERR_INVALID for rates that are not positive and finite. */
int sdrpp_design_pager(double if_rate, double baudrate, sdrpp_sym_desc* desc);

/* ---- Framer behind a symbol branch: 4FSK slicer -> sync search at every bit offset -> descrambled, de-interleaved frames ---------------------------------
 * What the M17 decoder's M17Slice4FSK and M17FrameDemux (decoder_modules/m17_decoder/src/m17dsp.h:96-276) compute from the clock recovery's soft symbols,
 * as a general block: the thresholds, the sync words, the frame length and the two tables come from the description (sdrpp_design_m17 fills M17's).
 *     slicer, per soft symbol `val`, two bits in this order:   val < 0.0f,   fabsf(val) > high_cut          (both strict: a NaN gives 0, 0)
 *     demux over delay[0 .. 16 + count): the 16 newest bits of the previous push, then this push's bits; for i from 0 while i < count:
 *         searching: delay[i .. i + 16) equals sync word t (at EVERY bit offset, odd ones included; the lowest t wins): frame type t begins, the step counter
 *                    becomes 0, the walk goes on AT THE SAME i; no match: i++
 *         in a frame: steps 0 .. 15 only advance (the sync word's own bits pass); step 16 + k, k in 0 .. frame_bits - 1, writes delay[i] ^ scramble[k] to
 *                    position interleave[k] of the frame and advances.  Nothing is searched inside a frame.  With step 16 + frame_bits - 1 the frame is
 *                    complete, leaves in THIS push, and the search resumes at the next i — a sync word directly behind a frame is found at once.
 * WHERE IT ATTACHES: only to a VFO that carries a symbol branch (sdrpp_vfo_set_symbols), else SDRPP_ERR_INVALID; it reads the branch's soft values of the same
 * push, in every push the branch runs in.  Detaching the branch, removing the VFO, or attaching ANOTHER branch description (which replaces the branch) detaches the framer.  It never changes a bit of any other output.
 * SDRPP_ERR_INVALID, each with its reason in sdrpp_last_error: high_cut not finite; n_sync outside 1 .. 4; frame_bits no multiple of 8 or outside 8 .. 1024;
 * a missing table; a scramble entry that is not 0 or 1; an interleave table that is not a permutation of 0 .. frame_bits - 1.
 * STATE, as the reference keeps it: the 16 delay bits, whether a frame is being built, its type, its step counter and the part-built frame.  Attaching starts
 * cleared: delay 0 (the reference's array is not initialised there), searching.  While the branch or the framer is switched off the state freezes; enabled = 1
 * with the SAME description continues from there.  Another description, a fresh attach or sdrpp_vfo_framer_reset start cleared.  desc == NULL detaches.
 * sdrpp_vfo_reset leaves the framer alone, as it leaves the loop.  sdrpp_vfo_replace with keep & 2 moves the framer with the branch, by the branch's rule (a
 * handle with another stream capacity gets both descriptions attached afresh, cleared).
 * The two tables exist ONCE per context for identical tables, however many VFOs carry a framer (sdrpp_frame_table_count).
 * OUTPUT of a push: the frames whose LAST bit was consumed in that push, so the concatenated output does not depend on how the stream is cut.  A frame RECORD
 * is  [type][0][frame_bits / 8 bytes: the frame, position 0 in the MSB of the first byte]  with the stride rounded up to a multiple of 4 (M17: 48 bytes; the
 * padding is 0); a push has room for (16 + 2 * symbol capacity) / (16 + frame_bits) + 1 records, which the walk cannot exceed.  Outside pipelined mode the
 * accessors name the most recent push (count 0 while the branch or the framer is switched off) and wait for the device, like the branch's.
 * Pipelined: sdrpp_pipeline_set_frame_results / sdrpp_result_frames.  The arrays are copied during the call. */
typedef struct sdrpp_frame_desc {
    float high_cut;             /* second slicer threshold; M17: (1 + 1/3) / 2 in float        */
    int n_sync;                 /* 1 .. 4 sync words of 16 bits, MSB first; index = frame type */
    uint16_t sync[4];
    int frame_bits;             /* bits behind the sync word: a multiple of 8, 8 .. 1024; M17: 368 */
    const uint8_t* scramble;    /* [frame_bits] 0 / 1                                          */
    const uint16_t* interleave; /* [frame_bits] destination of bit k: a permutation, else SDRPP_ERR_INVALID */
} sdrpp_frame_desc;
int sdrpp_vfo_set_framer(sdrpp_ctx* ctx, int id, const sdrpp_frame_desc* desc, int enabled);
int sdrpp_vfo_framer_reset(sdrpp_ctx* ctx, int id);
/* The framer's output of the most recent push: the number of frames, their records (sdrpp_frame_record_stride bytes apart). */
int sdrpp_vfo_frame_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_frame_read(sdrpp_ctx* ctx, int id, uint8_t* records, int max_frames);   /* returns the frames copied */
int sdrpp_vfo_frame_device_buffer(sdrpp_ctx* ctx, int id, const uint8_t** records, int* n);
int sdrpp_abi_sizeof_frame_desc(void);
/* Bytes from one record to the next for frames of `frame_bits` bits: 2 + frame_bits / 8 rounded up to a multiple of 4; SDRPP_ERR_INVALID for a length the framer refuses. */
int sdrpp_frame_record_stride(int frame_bits);
/* Test and statistics hook: table pairs (scramble, interleave) the context holds in device memory (identical pairs share one). */
int sdrpp_frame_table_count(sdrpp_ctx* ctx);
/* M17Decoder::init (m17dsp.h) for a VFO at if_rate: GFSK::init(.., 4800, if_rate, 2400, 31, 0.5, 1e-6, 0.01, 0.01) into *sym — inv_deviation for
 * Quadrature(2400, if_rate), omega = if_rate / 4800 with MM's gains 1e-6 (omega) and 0.01 (mu) and relative limit 0.01, 128 x 8 interpolator (the bank stays
 * the caller's: sdrpp_design_mm_interp), shape_ntaps = 31 with sdrpp_design_root_raised_cosine(31, 0.5, 4800, if_rate) into rrc_taps[] — and M17's framing into
 * *frame, scramble[368] and interleave[368], stated from the M17 specification: high_cut (1 + 1/3) / 2, sync words 0x55F7 (link setup), 0xFF5D (stream), 0x75FF
 * (packet), 368 bits, the 46-byte decorrelator sequence MSB first, interleave[k] = (45 k + 92 k^2) mod 368.  The pointers of the two descriptions are set to
 * the caller's arrays (interp_bank is left alone).  SDRPP_ERR_INVALID for a rate that is not positive and finite, a missing argument or max_taps < 31. */
int sdrpp_design_m17(double if_rate, sdrpp_sym_desc* sym, float* rrc_taps, int max_taps, sdrpp_frame_desc* frame, uint8_t* scramble, uint16_t* interleave);

/* ---- RDS demodulator: AGC -> Costas loop -> complex band-pass -> Costas loop -> MM clock recovery -> slicer -> differential decoder ---------------------
 * What the radio module's RDSDemod (decoder_modules/radio/src/rds_demod.h:64-74) computes from BroadcastFM::rdsOut, per 5 kS/s sample x[i] and per symbol:
 *     a[i]  = x[i] * gain;  gain += (set_point - |a[i]|) * rate, clamped to max_gain from above only                     (loop/fast_agc.h)
 *     c[i]  = a[i] * phasor(-phase1);  e = clamp(c.re * c.im, -1, 1)                                                      (loop/costas.h, ORDER 2)
 *             freq1 = clamp(freq1 + beta * e, min_freq, max_freq);  phase1 += freq1 + alpha * e, wrapped into +-FL_M_PI  (loop/phase_control_loop.h:58-85)
 *     f[i]  = sum_k c[i - (K-1) + k] * taps[k]          FIR<complex_t, complex_t>: volk_32fc_x2_dot_prod_32fc in the generic order, every product and sum rounded apart
 *     r[i]  = (f[i] * phasor(-phase2)).re, the second loop advanced likewise
 *     MM<float> over r exactly as the symbol branch runs it (above); soft = its output, b = soft > 0, bit = (b - last + 2) % 2, last = b
 * in float throughout, every operation of the three recursions in the reference's order.  A general block: every parameter comes from the description
 * (sdrpp_design_rds_demod fills the radio's).  The group decoder (rds::Decoder) stays host code and reads the bits.
 * SOURCE 0: the output of the VFO's RDS branch — needs sdrpp_vfo_set_rds on that (WFM) VFO first, SDRPP_ERR_INVALID otherwise; it runs in the blocks the
 * branch runs in, and detaching the RDS branch detaches the demodulator.  SOURCE 1: the stream a demodulator would read, on SDRPP_DEMOD_RAW VFOs only
 * (SDRPP_ERR_UNSUPPORTED otherwise): a BPSK demodulator for any channel.  It never changes a bit of any other output.
 * SDRPP_ERR_INVALID, each with its reason in sdrpp_last_error: a value that is not finite; n_taps outside 1 .. 256, interp_ntaps outside 1 .. 16,
 * interp_phases outside 1 .. 1024, a missing array; a source other than 0 or 1; min >= max for a loop's frequency limits or for omega's; MM's step bounds
 * as the symbol branch has them (min_omega - |mu_gain| >= 1, max_omega + |mu_gain| <= 4096); and a Costas loop with
 *     max(|min_freq|, |max_freq|) + |alpha| > 2 pi      or      |init_phase| > pi
 * — the reference wraps the phase with `while (phase > max) phase -= 2 pi`; under this bound (|error| <= 1) one conditional subtraction and one conditional
 * addition are that loop exactly, and that is what the device runs: no trip count on the device depends on a sample's value.  Samples that are not numbers
 * give unspecified values; the block ends and stays inside its arrays.
 * STATE: gain, both loops' phase and frequency, the filter's K - 1 newest inputs, MM's four words and T - 1 samples, the decoder's last bit.  A fresh attach
 * and a call with another description start as RDSDemod::init leaves them; enabled = 0 freezes everything (nothing planned, nothing delivered) and enabled = 1
 * with the SAME description continues; desc == NULL detaches.  sdrpp_vfo_rds_demod_reset is RDSDemod::reset(): gain, loops, filter line, MM (offset, phase,
 * omega, lastOut — its T - 1 delay samples stay, as MM::reset leaves them) and the decoder's last bit.  sdrpp_vfo_reset leaves the demodulator alone, as it
 * leaves the RDS branch's own streams.  sdrpp_vfo_replace with keep & 2 and the same demodulator kind moves it, parameters and state, to the new handle (a
 * source-0 demodulator moves with its RDS branch; a handle with another stream capacity gets the description attached afresh, cleared).
 * Tap table and interpolator bank exist ONCE per context for identical descriptions (sdrpp_rdsd_bank_count).
 * OUTPUT of a push: the symbols whose start lies inside it, as for the symbol branch: the concatenated output does not depend on how the stream is cut.
 * The accessors name the most recent push (SDRPP_ERR_INVALID without a demodulator, count 0 while it is switched off) and wait for the device.
 * Pipelined: sdrpp_pipeline_set_rds_bits_results / sdrpp_result_rds_bits.
 * The arrays are copied during the call. */
typedef struct sdrpp_rdsd_loop {
    float alpha, beta;                /* PhaseControlLoop::criticallyDamped(bandwidth): sdrpp_design_pll                          */
    float init_phase, init_freq;      /* radians, radians per sample                                                             */
    float min_freq, max_freq;
} sdrpp_rdsd_loop;
typedef struct sdrpp_rdsd_desc {
    int source;                       /* 0: the VFO's RDS branch, 1: the stream a demodulator would read (RAW VFOs)               */
    float agc_set_point, agc_max_gain, agc_rate, agc_init_gain;
    sdrpp_rdsd_loop loop1, loop2;     /* in front of and behind the band-pass                                                     */
    int n_taps;                       /* complex taps, 1 .. 256                                                                   */
    const float* taps;                /* interleaved (re, im): sdrpp_design_band_pass_complex(0, 2375, 100, rate, 0, ...)          */
    float omega;                      /* MM, as in sdrpp_sym_desc                                                                 */
    float mu_gain, omega_gain;
    float min_omega, max_omega;
    int interp_phases, interp_ntaps;
    const float* interp_bank;
} sdrpp_rdsd_desc;
int sdrpp_vfo_set_rds_demod(sdrpp_ctx* ctx, int id, const sdrpp_rdsd_desc* desc, int enabled);
int sdrpp_vfo_rds_demod_reset(sdrpp_ctx* ctx, int id);
/* The demodulator's output of the most recent push: soft symbols (MM's output) and decoded bits. */
int sdrpp_vfo_rds_demod_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_rds_demod_read(sdrpp_ctx* ctx, int id, float* soft_host, uint8_t* bits_host, int max);   /* either array may be NULL; returns the symbols copied */
int sdrpp_vfo_rds_demod_device_buffers(sdrpp_ctx* ctx, int id, const float** soft, const uint8_t** bits, int* n);
int sdrpp_abi_sizeof_rdsd_desc(void);
/* Test and statistics hook: tap table / interpolator bank pairs of RDS demodulators the context holds in device memory (identical descriptions share one). */
int sdrpp_rdsd_bank_count(sdrpp_ctx* ctx);
/* Every field of *desc as RDSDemod::init (rds_demod.h:19-41) leaves its members, for a stream of `rate` samples per second (the radio's: 5000), source 0:
 * FastAGC(1.0, 1e6, 0.1, 1.0); Costas<2>(0.005f); bandPass<complex_t>(0, 2375, 100, rate) through sdrpp_design_band_pass_complex into taps[]; Costas<2>(0.01)
 * at hzToRads(1187.5, rate) +- 10 %; MM(rate / 1187.5, 1e-6, 0.01, 0.01) with sdrpp_design_mm_interp(128, 8) into bank[].  The two arrays stay the caller's
 * (max_taps complex taps, max_bank floats) and desc points at them.  Returns the number of complex taps (190 at 5000), or SDRPP_ERR_INVALID: a rate that
 * is not positive and finite, an array that is missing or too small (1024 floats of bank). */
int sdrpp_design_rds_demod(double rate, sdrpp_rdsd_desc* desc, float* taps, int max_taps, float* bank, int max_bank);

/* ---- Meteor QPSK demodulator: root-raised-cosine FIR -> AGC -> QPSK Costas loop -> optional OQPSK delay -> complex MM clock recovery -> int8 pairs ---------
 * What the meteor_demodulator module's dsp::demod::Meteor (decoder_modules/meteor_demodulator/src/meteor_demod.h:150-167) computes from a 150 kS/s channel,
 * per sample x[i] and per symbol:
 *     f[i]  = sum_k x[i - (K-1) + k] * taps[k]          FIR<complex_t, float>: volk_32fc_32f_dot_prod_32fc in the generic order, re and im each accumulated
 *                                                        sequentially, every product and sum rounded apart
 *     a[i]  = f[i] * gain;  gain += (set_point - |a[i]|) * rate, clamped to max_gain from above only                       (loop/fast_agc.h)
 *     c[i]  = a[i] * phasor(-phase);  e = clamp(step(c.re) * c.im - step(c.im) * c.re, -1, 1), or with broken != 0 the four-phase rule of
 *             meteor_costas.h:35-51 (atan2f, normalizePhase, the lowest |dp| in the reference's order, times the amplitude); the loop advanced as
 *             sdrpp_rdsd_desc's loops are (loop/phase_control_loop.h:58-85)
 *     oqpsk != 0:  c[i].im is exchanged with the carried lastI: the imaginary part is delayed by one sample             (meteor_demod.h:155-162)
 *     MM<complex_t> over c (clock_recovery/mm.h:100-156): the interpolator applied to re and im, the delays _p_2T <- _p_1T <- _p_0T and _c_2T <- _c_1T <- _c_0T
 *             with _c_0T = step(out) per component, error = ((p0 - p2) * conj(c1) - (c0 - c2) * conj(p1)).re clamped to +-1, pcl.advance, offset += floorf(phase)
 *     per symbol two outputs: the complex soft symbol, and two int8 values (int8)clamp((int)(v * soft_scale), -127, 127) as the module's sink writes them
 *             (main.cpp:193-201, soft_scale 84): the conversion truncates towards zero, values beyond +-127 / soft_scale saturate, a NaN gives 0
 * in float throughout, every operation in the reference's order.  A general block: every parameter comes from the description (sdrpp_design_meteor fills the
 * module's).  The frame decoder stays host code and reads the int8 pairs: 144 KB/s per channel instead of 1.2 MB/s of IF samples.
 * Works on SDRPP_DEMOD_RAW VFOs only, on the stream a demodulator would read (SDRPP_ERR_UNSUPPORTED otherwise).  It never changes a bit of any other output.
 * SDRPP_ERR_INVALID, each with its reason in sdrpp_last_error: a value that is not finite (taps included); n_taps outside 1 .. 256, interp_ntaps outside
 * 1 .. 16, interp_phases outside 1 .. 1024, a missing array; min >= max for the loop's frequency limits or for omega's; MM's step bounds as the symbol branch
 * has them (min_omega - |mu_gain| >= 1, max_omega + |mu_gain| <= 4096); and a loop with max(|min_freq|, |max_freq|) + |alpha| > 2 pi or |init_phase| > pi
 * (the bounded-loop rule of sdrpp_rdsd_desc: no trip count on the device depends on a sample's value).  Samples that are not numbers give unspecified values;
 * the block ends and stays inside its arrays.
 * STATE: the filter's K - 1 newest inputs, gain, loop phase and frequency, lastI, MM's phase, frequency, offset, six delay words and T - 1 samples.  A fresh
 * attach and a call with another description start as Meteor::init leaves them; `broken` and `oqpsk` are modes and no part of the description's identity: the
 * same description with other modes only sets them.  enabled = 0 freezes everything (nothing planned, nothing delivered) and enabled = 1 with the SAME
 * description continues; desc == NULL detaches.  sdrpp_vfo_qpsk_set_mode is setBrokenModulation / setOQPSK: the state is kept, the modes hold from the next
 * push.  sdrpp_vfo_qpsk_reset is Meteor::reset(): the filter line, the gain, the loop, MM's offset / phase / omega and six delay words — lastI and MM's T - 1
 * delay samples stay, as the reference leaves them.  sdrpp_vfo_reset leaves the demodulator alone.  sdrpp_vfo_replace with keep & 2 between two RAW VFOs
 * moves it, parameters and state, to the new handle (a handle with another stream capacity gets the description attached afresh, cleared).
 * Tap table and interpolator bank exist ONCE per context for identical descriptions (sdrpp_qpsk_bank_count).
 * OUTPUT of a push: the symbols whose start lies inside it: the concatenated output does not depend on how the stream is cut.  The accessors name the most
 * recent push (SDRPP_ERR_INVALID without a demodulator, count 0 while it is switched off) and wait for the device.  soft_iq: interleaved (re, im), 2 floats per
 * symbol; packed: 2 int8 per symbol.  Pipelined: sdrpp_pipeline_set_qpsk_results / sdrpp_result_qpsk.
 * The arrays are copied during the call. */
typedef struct sdrpp_qpsk_desc {
    int n_taps;                       /* real taps of the shaping filter, 1 .. 256                                                */
    const float* taps;                /* sdrpp_design_root_raised_cosine                                                          */
    float agc_set_point, agc_max_gain, agc_rate, agc_init_gain;
    sdrpp_rdsd_loop loop;             /* the QPSK Costas loop                                                                     */
    int broken, oqpsk;                /* MeteorCostas::_broken, Meteor::_oqpsk                                                    */
    float omega;                      /* MM, as in sdrpp_sym_desc                                                                 */
    float mu_gain, omega_gain;
    float min_omega, max_omega;
    int interp_phases, interp_ntaps;
    const float* interp_bank;
    float soft_scale;                 /* int8 = clamp((int)(v * soft_scale), -127, 127): 84 for the module                        */
} sdrpp_qpsk_desc;
int sdrpp_vfo_set_qpsk(sdrpp_ctx* ctx, int id, const sdrpp_qpsk_desc* desc, int enabled);
int sdrpp_vfo_qpsk_set_mode(sdrpp_ctx* ctx, int id, int broken, int oqpsk);
int sdrpp_vfo_qpsk_reset(sdrpp_ctx* ctx, int id);
/* The demodulator's output of the most recent push. */
int sdrpp_vfo_qpsk_count(sdrpp_ctx* ctx, int id);
int sdrpp_vfo_qpsk_read(sdrpp_ctx* ctx, int id, float* soft_iq, int8_t* packed, int max);   /* either array may be NULL; returns the symbols copied */
int sdrpp_vfo_qpsk_device_buffers(sdrpp_ctx* ctx, int id, const float** soft_iq, const int8_t** packed, int* n);
int sdrpp_abi_sizeof_qpsk_desc(void);
/* Test and statistics hook: tap table / interpolator bank pairs of QPSK demodulators the context holds in device memory (identical descriptions share one). */
int sdrpp_qpsk_bank_count(sdrpp_ctx* ctx);
/* taps/root_raised_cosine.h in double, its three branches (t == 0, t == +-Ts / (4 beta), otherwise) included, Ts = samplerate / symbolrate; every tap rounded
 * to float once.  Returns count, or SDRPP_ERR_INVALID: count < 1 or > max, a missing array, values that are not positive and finite. */
int sdrpp_design_root_raised_cosine(int count, double beta, double symbolrate, double samplerate, float* taps, int max);
/* Every field of *desc as Meteor::init (meteor_demod.h:24-43) leaves its members: rootRaisedCosine(rrc_taps, rrc_beta, symbolrate, samplerate) into taps[];
 * FastAGC(1.0, 10e6, agc_rate) with its initial gain 1.0; MeteorCostas(costas_bw) at phase 0, frequency 0, limits +-FL_M_PI; MM(samplerate / symbolrate,
 * omega_gain, mu_gain, 0.01 — init does not pass omegaRelLimit on) with sdrpp_design_mm_interp(128, 8) into bank[]; soft_scale 84.  The two arrays stay the
 * caller's (max_taps taps, max_bank floats) and desc points at them.  Returns the number of taps, or SDRPP_ERR_INVALID: rates or gains that are not finite, an
 * array that is missing or too small (1024 floats of bank). */
int sdrpp_design_meteor(double symbolrate, double samplerate, int rrc_taps, double rrc_beta, double agc_rate, double costas_bw, int broken, int oqpsk, double omega_gain,
                        double mu_gain, sdrpp_qpsk_desc* desc, float* taps, int max_taps, float* bank, int max_bank);

/* ---- WaterFall display state around the raw-line history (core/src/gui/widgets/waterfall.cpp) ---------------
 * The last `height` raw dB lines stay resident in HBM in the reference's ring order (getFFTBuffer :875-886), so a zoom / pan /
 * level change re-renders the whole waterfall on the device (updateWaterfallFb :600-631) instead of re-reading host memory, and
 * the FFT trace's smoothing and peak hold (pushFFT :913-939) run per new line next to the zoom that already does.
 * Needs sdrpp_fft_configure first (and sdrpp_fft_set_view for the trace); re-configuring the FFT size invalidates it. */
int sdrpp_wf_configure(sdrpp_ctx* ctx, int height);                              /* waterfallHeight lines kept; 0 removes          */
int sdrpp_wf_set_smoothing(sdrpp_ctx* ctx, int enabled, float speed);            /* setFFTSmoothing + setFFTSmoothingSpeed :1166-1194 */
int sdrpp_wf_set_hold(sdrpp_ctx* ctx, int enabled, float speed);                 /* setFFTHold + setFFTHoldSpeed :1153-1164          */
/* latestFFT (after smoothing) and latestFFTHold of the current view: data_width floats each (NULL to skip); returns data_width */
int sdrpp_wf_latest(sdrpp_ctx* ctx, float* latest, float* hold);
/* calculateVFOSignalInfo (:558-598) on the newest stored line: strength = max dB inside the VFO, snr = strength - mean of the two
 * half-bandwidth side bands.  Returns 1, or 0 while no line is stored. */
int sdrpp_wf_signal_info(sdrpp_ctx* ctx, double center_offset, double bandwidth, double whole_bandwidth, float* strength, float* snr);
/* ---- signal meters: calculateVFOSignalInfo for a TABLE of bands on EVERY raw line a push completes, inside the push's own launches ----
 * sdrpp_wf_signal_info answers for one band on the newest stored line and has to drain a pipelined run to do so; a receiver that meters 32 to 128
 * channels on every block sets a table instead.  Meter m is the band (descs[m].center_offset, descs[m].bandwidth) of a spectrum `whole_bandwidth`
 * wide; for every line f of a push: out[f][m][0] = strength, out[f][m][1] = snr — the same arithmetic in the same summation order as
 * sdrpp_wf_signal_info, so a line's values are bit-identical to what that call returns while the line is the newest of the history ring (which the
 * meters do not need: they read the block's own lines).  Empty side bands (all four offsets in one bin, or a band at the lower edge whose side
 * bands are clamped away on both sides) give snr = NaN, as the reference's 0.0 / 0.0 does.
 * OUT-OF-BAND RULE (as for sdrpp_wf_signal_info): the four bin offsets are clamped to [0, fft_size]; for a band that reaches past
 * +whole_bandwidth / 2 the reference reads one bin beyond the line (fftLine[rawFFTSize]), the device clamps that read to the last bin.
 * Needs sdrpp_fft_configure (SDRPP_ERR_INVALID without).  n = 0 removes the table; n > SDRPP_MAX_METERS: SDRPP_ERR_UNSUPPORTED.  The table is kept
 * as frequencies: sdrpp_fft_configure with another size keeps it and recomputes the offsets.  Setting a table is a configuration change (it
 * flushes deferred pushes and sends a held launch group on its way) but does not drain a pipelined run: blocks already pushed keep the table they
 * were pushed with — it travels with their job tables — and the new one applies from the next push. */
#define SDRPP_MAX_METERS 1024
typedef struct sdrpp_meter_desc { double center_offset, bandwidth; } sdrpp_meter_desc;
int sdrpp_wf_set_meters(sdrpp_ctx* ctx, int n, const sdrpp_meter_desc* descs, double whole_bandwidth);
/* Outside pipelined mode: the meters of the most recent push (pass), [n_lines][n_meters][2] floats, oldest line first.  *n_lines = 0 when the push
 * completed no line or came before the table.  dst may be NULL to ask for the counts alone; more than max_lines lines: SDRPP_ERR_INVALID.  In
 * pipelined mode the values come with the results (sdrpp_result_meters) and this call is SDRPP_ERR_INVALID. */
int sdrpp_wf_meters_read(sdrpp_ctx* ctx, float* dst_host, int max_lines, int* n_lines, int* n_meters);
int sdrpp_abi_sizeof_meter_desc(void);
/* updateWaterfallFb: palette indices [height][data_width], newest line first, rows beyond the stored lines = -1 (opaque black). */
int sdrpp_wf_raster(sdrpp_ctx* ctx, int draw_data_start, int draw_data_size, int data_width, float wf_min, float wf_max, int32_t* dst_host, int* n_lines);

/* ---- IQFrontEnd pre-processing chain (core/src/signal_path/iq_frontend.cpp:32-39, setDecimation /
 *      setDCBlocking / setInvertIQ :105-130): PowerDecimator<complex_t> (stages of the plan for the ratio, power_decimator.h:93-111)
 *      -> DCBlocker<complex_t> (dc_rate = genDCBlockRate(effectiveSr) = 50 / effectiveSr, iq_frontend.h:55-57; 0 = block disabled)
 *      -> Conjugate.  Runs on the device in front of the FFT branch and the VFO bank: every later stage sees the pre-processed
 *      stream at the effective sample rate (FFT framing, VFO descriptors are the caller's, designed at that rate).  max_push of
 *      sdrpp_create counts RAW samples.  n_stages = 0, dc_rate = 0, conjugate = 0 removes the chain.  State starts cleared. */
/* Numerics of the chain.  Default: the decimator stages run on the matrix cores (k-ordered fused multiply-adds) and the DC blocker as a
 * parallel scan — the pre-processed stream then agrees with the reference to ~1e-7 (decimation only) resp. ~5e-5 (DC blocker on: the
 * reference's sequential float32 integrator carries a rounding drift of its own that a parallel sum does not reproduce), and waterfall
 * lines computed from it are NOT bit-exact any more (up to 5e-3 dB with decimation, 0.05 dB with DC blocking).  With
 * sdrpp_preproc_set_reference_order(ctx, 1) the chain evaluates the reference's own arithmetic — VOLK's generic tap-ordered
 * multiply-then-add dot product (decimating_fir.h:51-61) and the sequential DC-blocker recursion (dc_blocker.h:54-60), one wavefront,
 * ~40 cycles per sample — and the pre-processed stream, and every waterfall line behind it, is bit-identical to the compiled reference
 * (tests/test_parity_fft.py::test_preproc_chain_reference_order).  A parity mode: a few times real time at 10 MS/s, not thousands.
 * The switch survives sdrpp_preproc_configure; streaming state (history, offsets, the DC estimate) is shared by both modes. */
int sdrpp_preproc_set_reference_order(sdrpp_ctx* ctx, int on);
int sdrpp_preproc_configure(sdrpp_ctx* ctx, int n_stages, const int* stage_decim, const int* stage_ntaps, const float* const* stage_taps,
                            float dc_rate, int conjugate);
/* The same for a chain that is RE-planned while the stream runs — what IQFrontEnd's setters do to their blocks (iq_frontend.cpp:76-130):
 *   keep & 1: the decimator's delay lines and offsets stay if the new description has the same stages (setSampleRate / setDCBlocking / setInvertIQ
 *             do not touch the decimator; setDecimation creates new stages — PowerDecimator::setRatio, power_decimator.h:91-108 — so it passes 0 here);
 *   keep & 2: the DC blocker continues from its estimate (DCBlocker::setRate swaps the rate only; a blocker switched off and on again is the same
 *             object, dc_blocker.h:54-60).
 * sdrpp_preproc_configure = keep 0: everything cleared. */
int sdrpp_preproc_reconfigure(sdrpp_ctx* ctx, int n_stages, const int* stage_decim, const int* stage_ntaps, const float* const* stage_taps,
                              float dc_rate, int conjugate, int keep);
/* The pre-processed samples of the most recent push — what Splitter hands to streams bound with bindIQStream (iq_frontend.cpp:132-138). */
int sdrpp_preproc_out_count(sdrpp_ctx* ctx);
int sdrpp_preproc_read(sdrpp_ctx* ctx, float* dst_host, int max);
int sdrpp_preproc_device_buffer(sdrpp_ctx* ctx, const float** iq, int* n);

/* ---- data path ------------------------------------------------------------------------------------------------------------ */
/* One block of IQ, as Splitter::run hands to every bound stream (splitter.h:46-61).  Host pointer: copied H2D first.
 * Device pointer: read in place (must stay valid until the next sdrpp_sync / stream synchronisation).  Runs the FFT
 * branch and every VFO; asynchronous on the context's stream — outputs are readable after sdrpp_sync (the read calls
 * synchronise themselves). */
int sdrpp_push(sdrpp_ctx* ctx, const float* iq_host, int64_t count);
int sdrpp_push_device(sdrpp_ctx* ctx, const float* iq_dev, int64_t count);
/* file_source path (source_modules/file_source/src/main.cpp:154-167): interleaved int16 IQ converted on the device
 * (x / 32768), halving the PCIe bytes.  Host pointer. */
int sdrpp_push_int16(sdrpp_ctx* ctx, const int16_t* iq_host, int64_t count);
/* The wire formats of the reference's sources, converted on the device: the bus carries the bytes the radio delivered (2 per complex sample for the
 * 8-bit formats, 4 for int16) instead of 8.  Interleaved I / Q in host memory, `count` complex samples; the caller's buffer is free on return.
 *   SDRPP_IQ_I8   (float)x * (1.0f / scalar)   volk_8i_s32f_convert_32f (generic)    hackrf_source / network_source / harogic_source: scalar 128;
 *                                                                                     an SDR++ server frame: 128.0f / scaler
 *   SDRPP_IQ_I16  (float)x * (1.0f / scalar)   volk_16i_s32f_convert_32f (generic)   file_source: 32768 (= sdrpp_push_int16, the same routine); kcsdr_source: 8192;
 *                                                                                     spyserver 16-bit: 32768.0f * gain; a server frame: 32768.0f / scaler
 *   SDRPP_IQ_U8   table[b]                     256 floats from sdrpp_design_u8_table  rtl_sdr_source, rtl_tcp_source, spyserver 8-bit
 * 1.0f / scalar is ONE float division, done on the host; the int -> float conversion of an 8- or 16-bit integer is exact and the product one float multiply,
 * so every value is exactly specified.  The U8 sources each subtract and scale in arithmetic of their own (double, float, mixed): the host computes the
 * 256 possible results in that arithmetic and the device only looks them up.  The table is copied at the call, so it may change from one push to the next.
 * scalar must be finite and non-zero (I8, I16), table non-NULL (U8), type one of the three: SDRPP_ERR_INVALID otherwise.
 * Works in every mode a push has: at once, deferred, pipelined, in launch groups (sdrpp_set_pipeline_group).  In a group a push joins only if its format
 * matches the held pushes' (type, the scalar's bits, for U8 the table's contents); otherwise what is held goes out first, as for any push of another kind.
 * NOT offered, on purpose:
 *   int32 (network_source): 8 bytes per sample like float — converting it on the device saves nothing;
 *   a landing job per push of a group: server frames whose scaler changes from frame to frame therefore ride one launch each;
 *   raw formats read in place from the caller's page-locked memory (what sdrpp_push_pinned_async does for floats): a raw push is always copied into the
 *   library's staging slot first. */
#define SDRPP_IQ_I8  0
#define SDRPP_IQ_I16 1
#define SDRPP_IQ_U8  2
typedef struct sdrpp_iq_format {
    int type;            /* SDRPP_IQ_*                                 */
    float scalar;        /* I8 / I16; ignored for U8                   */
    const float* table;  /* U8: 256 floats; ignored for I8 / I16       */
} sdrpp_iq_format;
int sdrpp_push_raw(sdrpp_ctx* ctx, const void* iq_host, int64_t count, const sdrpp_iq_format* fmt);
/* One frame of the SDR++ server protocol as the client receives it — [u16 0][u16 type][f32 scaler][data], what SampleStreamDecompressor::process
 * takes (core/src/dsp/compression/sample_stream_decompressor.h:13-34; the sink-side twin is sdrpp_vfo_read_compressed): type at byte 2, scaler at byte 4,
 * data from byte 8.  PCM_TYPE_F32 is a plain sdrpp_push, _I16 sdrpp_push_raw with scalar 32768.0f / scaler, _I8 with 128.0f / scaler.  *samples (may be
 * NULL) = the count the reference returns.  A frame shorter than 8 bytes: SDRPP_ERR_INVALID.  An unknown type gives 0 samples and SDRPP_OK as in the
 * reference, and so does a frame whose data holds no whole sample: nothing is pushed. */
int sdrpp_push_frame(sdrpp_ctx* ctx, const unsigned char* frame, int bytes, int* samples);
/* The 256-entry table of a U8 source, in the types that source computes in:
 *   source 0  rtl_sdr_source/src/main.cpp:535-536   ((float)b - 127.4) / 128.0f        the subtraction and the division in double (127.4 is a double), rounded to float
 *   source 1  rtl_tcp_client.cpp:86-87              ((double)b - 128.0) / 128.0        all in double, rounded to float
 *   source 2  spyserver_client.cpp:139-142          ((float)b - 128.0f) * (1.0f / (gain * 128.0f))   all in float
 * gain: source 2 only.  SDRPP_ERR_INVALID for another source or a NULL table. */
int sdrpp_design_u8_table(int source, float gain, float* table256);
int sdrpp_abi_sizeof_iq_format(void);

/* Page-locked host memory for buffers that are pushed from (the copy out of pageable memory is staged by the runtime and about three
 * times slower); NULL on failure.  The host blocks allocate their frame-buffer slots with it. */
void* sdrpp_host_alloc(size_t bytes);
void sdrpp_host_free(void* p);
/* Device memory on the context's GPU for buffers the host hands to sdrpp_fft_copy_device (e.g. the line a several-GPU host keeps per stream for
 * its RCCL gather, host/sdrpp_gpu_rccl.h) without linking the HIP runtime itself; NULL on failure. */
void* sdrpp_device_alloc(sdrpp_ctx* ctx, size_t bytes);
void sdrpp_device_free(sdrpp_ctx* ctx, void* p);
/* A synchronous copy on the context's GPU for the same kind of host: kind 0 host -> device, 1 device -> device, 2 device -> host; returns when the
 * bytes have arrived.  THE ONE CALL OF A CONTEXT THAT IS THREAD-SAFE: it may come from another thread while the context's own thread is inside any
 * other call (a several-GPU host's gather thread copies a front end's newest line while its worker pushes blocks).  It runs on a stream of its own
 * and is therefore NOT ordered with the work queued on the context's stream: use it for buffers whose content is complete (filled by an earlier
 * sdrpp_device_copy, or by sdrpp_fft_copy_device followed by sdrpp_sync), not to read what a push has just been asked to compute.  It never waits
 * for queued launches and sets no error text (sdrpp_last_error belongs to the context's thread): the return code is all there is. */
int sdrpp_device_copy(sdrpp_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
/* Deferred processing: sdrpp_push* only stage the samples (the H2D copy runs, the caller's buffer is free on return) and the next call
 * that observes results — sdrpp_sync, any *_lines / *_read* / *_count / *_device_buffer(s) / sdrpp_wf_* call — or changes the
 * configuration processes everything staged since the previous one as ONE pass over the device.  The results then cover ALL those
 * pushes, concatenated (lines, VFO blocks); every staged push still counts as a reference block of its own for the block-dependent
 * operations (sdrpp_set_reference_block), so the output is what pushing and reading block by block gives — only the launch sequence is
 * paid once per pass instead of once per block.  This is how a host that drains a queue of blocks (IQFrontEnd with buffering on) keeps
 * up at the reference's block size (sample_rate / 200), where a pass is launch-bound.  At most max_push samples can be staged:
 * a push beyond that returns SDRPP_ERR_INVALID (observe first).  Off (default): every push is processed at once. */
int sdrpp_set_deferred(sdrpp_ctx* ctx, int on);
/* Deferred mode, page-locked source (sdrpp_host_alloc): stage WITHOUT waiting for the copy — the device fetches the samples itself, the
 * call returns at once.  The buffer must stay untouched until sdrpp_push_wait (all such copies have landed) or the next call that
 * returns results of the pass (any *_read*, sdrpp_sync) has returned.  How a frame-buffer worker stages a whole backlog of blocks for the
 * price of a few kernel launches and ONE wait (host/sdrpp_gpu_blocks.h: SampleFrameBuffer::worker, frame_buffer.h:76-98).  Outside
 * deferred mode, or with memory that is not page-locked, it is sdrpp_push. */
int sdrpp_push_pinned_async(sdrpp_ctx* ctx, const float* iq_pinned, int64_t count);
int sdrpp_push_wait(sdrpp_ctx* ctx);
int64_t sdrpp_pending(sdrpp_ctx* ctx);   /* samples staged and not yet processed */

/* ---- pipelined execution: one launch per block, results a few blocks late ----------------------------------------------------------
 * At the reference's block size (sample_rate / 200 samples per swap(): core/src/dsp/stream.h:9, source_modules/file_source/src/main.cpp:157)
 * a block is far less than one wave of work for the GPU and an ordinary pass costs the SUM of its ~8 dependent launches.  The reference
 * itself is a pipeline at that grain — one thread per dsp::block, every stream<T> a hand-over between two of them (block.h:46-73,
 * stream.h:43-92): while the demodulator works on block n the VFO already has block n + 1.  Pipelined mode does the same on the device:
 * every sdrpp_push* launches ONE kernel ("tick") that runs the arrival of block n (its copy into device memory, the upload of its job
 * tables) next to the front end / FFT pass 1 of block n - 1, the first decimator / FFT pass 2 of block n - 2, ... — every stage of every
 * block exactly as in an ordinary pass (same kernels' bodies, same arithmetic: results are bit-identical), only not one after the
 * other.  A block's results are complete `depth` launches later (depth <= 18: where the block's last role stands; 6 for a WFM bank + 65536-point FFT whose outputs stay on the device, 7 with its VFO blocks delivered, 12 with the AF chain): with the next blocks, or at once when the
 * caller asks (sdrpp_pipeline_flush, sdrpp_result_wait, any observing call such as sdrpp_vfo_read / sdrpp_sync — these run the queued
 * stages without new input; sdrpp_fft_lines and sdrpp_vfo_out_count only report what the host already knows and do not).
 *   sdrpp_push_device        reads the caller's buffer IN PLACE one launch later at the earliest: it must stay valid until sdrpp_sync.
 *   sdrpp_push / _push_int16 / _push_raw copy into a page-locked staging slot (the caller's buffer is free on return), fetched by the next launch.
 *   sdrpp_push_pinned_async  page-locked memory is fetched by the launch itself; sdrpp_push_wait returns when all such fetches have run.
 * The pre-processing chain (sdrpp_preproc_configure, default arithmetic), the radio's AF chain (sdrpp_vfo_set_af) and the waterfall display
 * state (sdrpp_wf_configure) run that way too — their stages are further levels of the block; so do VFOs on the reference-rotator NCO
 * (nco_mode = 2: the recursion over the whole block is one of the launch's work items — such a stream is bound by that chain, ~26 cycles per
 * sample, but every VFO's results stay pipelined) and banks of any size, a single VFO included (the vector-unit front ends, one VFO per work
 * item of the launch).  What cannot (the
 * reference-order arithmetic of the pre-processing chain, a resampler in its register-blocked vector form, a retune hand-over in progress, more
 * FFT frames than one scratch chunk, a block the pre-processing decimator swallows whole) is processed as an ordinary
 * pass behind everything queued: always correct, pipelined where possible — and its results are delivered into the block's result slot
 * like any other block's (by plain copies and a wait inside the push: the slow path).
 * result_flags (sdrpp_set_pipelined): which results every block also delivers into page-locked host memory, ready for sdrpp_result_wait
 * without any copy call: 1 = every VFO's output block (the end of its chain: the AF chain's output where one is attached, else what
 * sdrpp_vfo_read returns), 2 = zoomed lines + palette indices, 4 = raw dB lines, 8 = the pre-processed IQ stream of the block (only with a
 * pre-processing chain configured: without one it is the input block itself), 16 = for every VFO with a recorder sink (sdrpp_vfo_set_rec) its block as the
 * sink converts it and one sdrpp_rec_info per push (sdrpp_result_rec below).  16 is independent of 1: with 16 alone no float frames cross the bus — a mono
 * int16 recording is 2 bytes per frame against 8.
 * At most SDRPP_RESULT_SLOTS (24) launches' results exist at a time (one block per launch unless sdrpp_set_pipeline_group says otherwise): release
 * them (a block whose slot is still held 24 launches later fails the push).
 * HOW FAR BEHIND TO ASK: a streaming host takes block t - lag when it has pushed block t.  With lag >= depth + 1 (sdrpp_pipeline_stats
 * out[4]: 6-7 levels for a radio bank + FFT, 10 for cfg 4's NFM / AM / SSB chains, 12 with AF chains, + the levels of a pre-processing chain)
 * sdrpp_result_wait finds the block complete.  With a smaller lag it must run the queued stages and WAIT for the device at every call: host
 * and device then take turns instead of overlapping (measured: cfg 4, lag 8 against 10 levels, 213 instead of 165 us per block).
 * sdrpp_gpu::IQFrontEnd and bench.py follow the reported depth (up to 22, leaving two of the 24 slots to the blocks in the making). */
/* Host blocks in pipelined mode without the library's own copy: sdrpp_push_stage hands out the page-locked staging slot the next block is
 * fetched from (room for max_push samples); the host fills it — with several threads if it likes: a 400 KB memcpy is the largest single
 * item of a 50 000-sample block's host time — and its own buffer is free as soon as it has; sdrpp_push_staged then launches the block
 * exactly like sdrpp_push.  One slot is open at a time. */
int sdrpp_push_stage(sdrpp_ctx* ctx, int64_t count, float** slot);
int sdrpp_push_staged(sdrpp_ctx* ctx, int64_t count);
/* The same with the host's copy threads still at work: the call plans the block at once (the job tables do not depend on the samples:
 * ~8 us of a 50 000-sample block's ~50 us of host time) and waits, on the host, for *pending to reach 0 before the first launch that
 * reads the slot.  `pending` = the number of unfinished parts of the caller's copy, decremented (release order) by the copying threads;
 * a word that does not reach 0 within 5 s fails the push.  sdrpp_gpu::IQFrontEnd's pipelined worker stages its blocks this way. */
int sdrpp_push_staged_when(sdrpp_ctx* ctx, int64_t count, const volatile uint32_t* pending);
#define SDRPP_RESULT_SLOTS 24
#define SDRPP_GROUP_MAX 32
typedef struct sdrpp_result {
    uint64_t ticket;          /* the block: 1 for the first push in pipelined mode, counted by sdrpp_ticket                          */
    int n_vfo;                /* VFO blocks delivered (0 without result flag 1), in sdrpp_vfo_add order                              */
    const int* ids;           /* [n_vfo] VFO handles                                                                                 */
    const int64_t* offsets;   /* [n_vfo] first sample (2 floats each) of the VFO's block in `samples`                                */
    const int* counts;        /* [n_vfo] samples                                                                                     */
    const float* samples;     /* page-locked host memory of the library, valid until sdrpp_result_release                            */
    int n_lines, fft_size, data_width;
    const float* zoomed;      /* [n_lines][data_width] (flag 2), else NULL                                                           */
    const int32_t* index;     /* [n_lines][data_width] (flag 2)                                                                      */
    const float* raw;         /* [n_lines][fft_size] (flag 4)                                                                        */
    int n_iq;                 /* pre-processed IQ samples of the block (flag 8 with a pre-processing chain configured), else 0       */
    const float* iq;          /* [n_iq] complex: what streams bound with bindIQStream receive (iq_frontend.cpp:32-39 -> Splitter)    */
} sdrpp_result;
int sdrpp_set_pipelined(sdrpp_ctx* ctx, int on, int result_flags);
/* Result flag 16: what VFO `id`'s recorder sink made of push `ticket` — *data: frames * channels packed samples in the block's result slot (page-locked
 * memory of the library; element aligned: in a launch group the group's converted block lies there in one piece and this push's share starts at its
 * own first frame), *info: the record of this push alone (either may be NULL).  Valid between sdrpp_result_wait and sdrpp_result_release of that
 * ticket, like the pointers a sdrpp_result holds; outside of that: SDRPP_ERR_INVALID.  SDRPP_ERR_NOT_FOUND: the VFO has no sink, or the block was pushed before the
 * sink was attached or without flag 16.  Blocks of a pipelined run that were processed as an ordinary pass deliver the same.  A call of its own, so
 * that sdrpp_result's layout and SDRPP_ABI_VERSION stay what they are. */
int sdrpp_result_rec(sdrpp_ctx* ctx, uint64_t ticket, int id, const void** data, sdrpp_rec_info* info);
/* Result flag 32: the RDS branches' samples (sdrpp_vfo_set_rds) travel in every block's result slot, about 40 KB/s per channel.  The flag has a
 * call of its own — sdrpp_set_pipelined keeps refusing values above 31, as it always has — to be made in pipelined mode, between blocks (what is
 * queued runs first); leaving pipelined mode or calling sdrpp_set_pipelined again clears it.  32 is independent of 1.
 * sdrpp_result_rds: *data = *count complex samples (2 floats each) VFO `id`'s branch made of push `ticket`, in the block's result slot (in a launch
 * group the group's samples lie there in one piece and every push gets its own share).  Validity as for sdrpp_result_rec: between
 * sdrpp_result_wait and sdrpp_result_release, else SDRPP_ERR_INVALID.  SDRPP_ERR_NOT_FOUND: the VFO has no branch or it was switched off, the
 * block was pushed before the attach, or without flag 32.  Blocks of a pipelined run processed as an ordinary pass deliver the same.  Either
 * output may be NULL. */
#define SDRPP_RESULT_RDS 32
int sdrpp_pipeline_set_rds_results(sdrpp_ctx* ctx, int on);
int sdrpp_result_rds(sdrpp_ctx* ctx, uint64_t ticket, int id, const float** data, int* count);
/* Result flag 64: the symbol branches' outputs (sdrpp_vfo_set_symbols) travel in every block's result slot — per branch the per-push counts, then room for
 * the block's capacity of soft values (4 bytes) and bits (1 byte): 5 bytes per possible symbol, about 12 KB/s per 2400-baud channel.  A call of its own,
 * with the rules of sdrpp_pipeline_set_rds_results; 64 is independent of 1 and 32.
 * sdrpp_result_sym: *soft / *bits = the *count symbols VFO `id`'s branch started inside push `ticket` (in a launch group the group's symbols lie in one
 * piece and every push gets its own count and slice).  Validity as for sdrpp_result_rds; SDRPP_ERR_NOT_FOUND likewise.  Any output may be NULL. */
#define SDRPP_RESULT_SYM 64
int sdrpp_pipeline_set_sym_results(sdrpp_ctx* ctx, int on);
int sdrpp_result_sym(sdrpp_ctx* ctx, uint64_t ticket, int id, const float** soft, const uint8_t** bits, int* count);
/* Result flag 128: the RDS demodulators' outputs (sdrpp_vfo_set_rds_demod) travel in every block's result slot, in the symbol branch's layout — per
 * demodulator the per-push counts, then room for the block's capacity of soft values (4 bytes) and decoded bits (1 byte): 5 bytes per possible symbol, about
 * 6 KB/s per channel.  A call of its own, with the rules of sdrpp_pipeline_set_rds_results; 128 is independent of 1, 32 and 64: a host that only wants the
 * bits leaves flag 32 off and stops paying for the 5 kS/s samples.
 * sdrpp_result_rds_bits: *soft / *bits = the *count symbols VFO `id`'s demodulator started inside push `ticket` (in a launch group the group's symbols lie
 * in one piece and every push gets its own count and slice).  Validity as for sdrpp_result_rds; SDRPP_ERR_NOT_FOUND likewise.  Any output may be NULL. */
#define SDRPP_RESULT_RDS_BITS 128
int sdrpp_pipeline_set_rds_bits_results(sdrpp_ctx* ctx, int on);
int sdrpp_result_rds_bits(sdrpp_ctx* ctx, uint64_t ticket, int id, const float** soft, const uint8_t** bits, int* count);
/* Result flag 256: the QPSK demodulators' outputs (sdrpp_vfo_set_qpsk) travel in every block's result slot, in the symbol branch's layout — per demodulator
 * the per-push counts, then room for the block's capacity of symbols.  By default the int8 pairs only (2 bytes per possible symbol: 144 KB/s per channel at
 * 72 000 symbols/s); with_soft != 0 adds the float pairs (8 bytes more).  A call of its own, with the rules of sdrpp_pipeline_set_rds_results.
 * sdrpp_result_qpsk: *soft_iq / *packed = the *count symbols VFO `id`'s demodulator started inside push `ticket` (in a launch group the group's symbols lie
 * in one piece and every push gets its own count and slice); *soft_iq is NULL where the float pairs were not asked for.  Validity as for sdrpp_result_rds;
 * SDRPP_ERR_NOT_FOUND likewise.  Any output may be NULL. */
#define SDRPP_RESULT_QPSK 256
int sdrpp_pipeline_set_qpsk_results(sdrpp_ctx* ctx, int on, int with_soft);
int sdrpp_result_qpsk(sdrpp_ctx* ctx, uint64_t ticket, int id, const float** soft_iq, const int8_t** packed, int* count);
/* Result flag 512: the framers' outputs (sdrpp_vfo_set_framer) travel in every block's result slot — per framer the per-push frame counts, then room for the
 * block's capacity of records: about 1.2 KB/s per M17 channel.  A call of its own, with the rules of sdrpp_pipeline_set_sym_results; 512 is independent of
 * every other flag: 64 is not needed for it.
 * sdrpp_result_frames: *records = the *count frames VFO `id`'s framer completed inside push `ticket` (in a launch group the group's records lie in one piece
 * and every push gets its own count and slice).  Validity as for sdrpp_result_rds; SDRPP_ERR_NOT_FOUND likewise.  Any output may be NULL. */
#define SDRPP_RESULT_FRAMES 512
int sdrpp_pipeline_set_frame_results(sdrpp_ctx* ctx, int on);
int sdrpp_result_frames(sdrpp_ctx* ctx, uint64_t ticket, int id, const uint8_t** records, int* count);
/* Signal meters of push `ticket` (sdrpp_wf_set_meters): *data = [*n_lines][*n_meters][2] floats in the block's result slot, for the lines this push's
 * own samples completed — the rows `zoomed` / `raw` give it — oldest first.  No result flag: while a table is set, EVERY pipelined block with the
 * FFT on carries its meters (n_lines * n_meters * 8 bytes), result_flags = 0 included — sdrpp_result_wait / _release then work for such blocks.
 * Valid between sdrpp_result_wait and sdrpp_result_release, else SDRPP_ERR_INVALID.  SDRPP_ERR_NOT_FOUND: the block was pushed before a table was
 * set (or with the FFT off).  A block that completed no line: *n_lines = 0.  n_meters is the size of the table the block was pushed with.  Blocks
 * of a pipelined run that were processed as an ordinary pass deliver the same.  Any of the three outputs may be NULL. */
int sdrpp_result_meters(sdrpp_ctx* ctx, uint64_t ticket, const float** data, int* n_lines, int* n_meters);
/* SEVERAL BLOCKS PER LAUNCH.  A launch costs the device a start ramp, a tail and the gap to the next one whatever the block holds, and the host one
 * plan: at the reference's block size (sample_rate / 200) that is most of a block's time, and a host that pushes faster than the device works
 * only makes the launch queue longer.  With max_blocks > 1 a push is HELD — nothing planned, nothing launched — until max_blocks pushes have come
 * together (or the next push cannot join: another kind of push, device / page-locked memory that does not continue where the last block ended,
 * more than max_push samples in all; or any call that observes results or changes the configuration, sdrpp_pipeline_flush, sdrpp_result_wait
 * for one of them).  The group then goes out as ONE launch: its blocks are planned as one block of the stream whose reference-block ends
 * (sdrpp_set_reference_block: AGC look-ahead, rotator calls) are the ends of the pushes — exactly what a deferred pass does with its staged
 * pushes — so every sample of every output is the one block-by-block processing gives (bit-identical: tests/test_pipelined.py::
 * test_grouped_launches_equal_block_by_block), and EVERY PUSH KEEPS ITS OWN TICKET AND RESULTS: sdrpp_result_wait(ticket) hands out that push's
 * share of every VFO's output block and the lines its samples completed (views into the group's result slot; SDRPP_RESULT_SLOTS now counts launch
 * groups, of up to SDRPP_GROUP_MAX blocks each).  Host pushes of a group land back to back in ONE page-locked staging slot and are fetched by
 * one landing copy; device / page-locked blocks must be contiguous to share a launch (a ring of blocks in one allocation is; the wrap-around
 * starts a new group).  The sum of a group's blocks is limited by max_push (sdrpp_create): size it for max_blocks blocks.
 * adaptive = 1: a push also goes out at once — with whatever is held — when the device has fewer than two launches in flight, i.e. the group size
 * follows what is queued: 1 while the host is the slower side (no added latency), max_blocks when the device is.  adaptive = 0: always wait for
 * max_blocks (deterministic: tests, benchmarks).  What it costs: a held block waits for its group, and a block's results are complete `depth`
 * LAUNCHES after its group went out — a streaming host asks (depth + 1) * max_blocks blocks behind (sdrpp_pipeline_stats out[4] is still the
 * depth in launches).  max_blocks = 1 (default): one launch per push, as before.  Groups do not form behind a pre-processing chain
 * (sdrpp_preproc_configure) or while a block cannot run as a launch of the pipeline at all: such pushes go out one by one.
 * `adaptive` is a set of flags: 1 as above; 2: the words handed to sdrpp_push_staged_when stay valid until their block has been LAUNCHED (not just for the
 * call) — a push that is merely held then returns at once instead of waiting for its copy threads, and the copy runs on under whatever the host does next
 * (the launch of the group waits for every word).  sdrpp_gpu::IQFrontEnd uses 2 with a ring of words and decides on the HOST side when a group goes out: full,
 * or no new block for a few microseconds (sdrpp_pipeline_launch_held) — at the stream seam the device is never the slower side, so rule 1 would never group. */
int sdrpp_set_pipeline_group(sdrpp_ctx* ctx, int max_blocks, int adaptive);
/* Launches what is held (nothing held: no-op).  Unlike sdrpp_pipeline_flush it does not run the queued stages of earlier blocks to completion. */
int sdrpp_pipeline_launch_held(sdrpp_ctx* ctx);
/* out[0] launch groups so far (single blocks included), [1] groups of more than one block, [2] the blocks in those, [3] the largest group,
 * [4] pushes held right now.  Returns the number of entries written. */
int sdrpp_pipeline_group_stats(sdrpp_ctx* ctx, int64_t* out, int max);
uint64_t sdrpp_ticket(sdrpp_ctx* ctx);                       /* ticket of the most recent push (pushes so far in pipelined mode)    */
int sdrpp_pipeline_flush(sdrpp_ctx* ctx);                    /* launch what is queued, no new input; does not wait                  */
int sdrpp_result_ready(sdrpp_ctx* ctx, uint64_t ticket);     /* 1 / 0 without blocking or flushing; SDRPP_ERR_NOT_FOUND: no slot    */
int sdrpp_result_wait(sdrpp_ctx* ctx, uint64_t ticket, sdrpp_result* out);   /* flushes if needed, waits, hands the slot out        */
int sdrpp_result_release(sdrpp_ctx* ctx, uint64_t ticket);
/* wait + copy + release in one call for a host that only wants a block's zoomed lines / palette indices (result flag 2): up to max_lines lines
 * of data_width values each go to zoomed_dst / index_dst (either may be NULL); *n_lines = lines the block completed.  SDRPP_ERR_INVALID if it
 * completed more than max_lines (the slot is released all the same). */
int sdrpp_result_take_lines(sdrpp_ctx* ctx, uint64_t ticket, float* zoomed_dst, int32_t* index_dst, int max_lines, int* n_lines);
/* How the blocks of a pipelined run were executed — for tests and bench.py, which assert the mode they mean to measure.
 * out[0] launches ("ticks") so far, [1] blocks that ran as ticks, [2] blocks that fell back to an ordinary pass, [3] ticks with more role
 * workgroups than the device holds at once (3 per CU: "crowded" order of the roles, tick_host.h), [4] levels of the most recent block (its
 * results are complete that many launches after its push), [5] number of roles R, [6] reserved, always 0, [7] bytes of job tables the most
 * recent block uploaded; then out[8 + r], r < R: workgroups
 * launched so far in role r (sdrpp_pipeline_role_name(r); e.g. "fcm16_132_4" = the front end in its small-block shape).
 * Returns the number of entries written (<= max).  Counters start at sdrpp_create. */
#define SDRPP_PIPELINE_STATS_HEAD 8
int sdrpp_pipeline_stats(sdrpp_ctx* ctx, int64_t* out, int max);
const char* sdrpp_pipeline_role_name(int role);
/* Which kernel forms the ORDINARY pass launched (sdrpp_push outside pipelined mode, and the blocks of a pipelined run that fell back to a
 * pass) — for tests, which assert the kernel they mean to test.  out[f] = launches of form f since sdrpp_create, names[f] its name (static
 * strings): f < R (sdrpp_pipeline_stats out[5]) are the forms that are also roles, named as sdrpp_pipeline_role_name(f); behind them the forms
 * an ordinary pass alone has: "polyb_4", "polyb_8", "polyb_4_odd", "polyb_8_odd" (the resampler with up to 4 / 8 phases whose Toeplitz table
 * does not fit, even / odd decimation), "s1_8|4|2", "s1d_8|4|2", "f2_8_44_3", "f2_8|4|2" (the VALU front ends with 8 / 4 / 2 VFOs per job), "rotx_1" (the one-wavefront reference rotator).
 * Either array may be NULL (ctx may be NULL when out is).  Returns the number of entries written (<= max); a launch of an FFT-branch kernel is
 * not counted. */
int sdrpp_pass_form_stats(sdrpp_ctx* ctx, int64_t* out, const char** names, int max);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------------------------------- */
/* Cumulative per-kernel-family device time measured with HIP events on the context's stream while timing is enabled.
 * family: 0 fft_pass1, 1 fft_pass2, 2 fft_single, 3 zoom, 4 vfo_stage1, 5 vfo_decim, 6 vfo_poly, 7 vfo_fir, 8 demod, 9 carry/misc,
 * 10 af_chain, 11 vfo_pipe (FM back ends as one launch), 12 tick (pipelined mode: one launch per block) */
#define SDRPP_NUM_KERNEL_FAMILIES 13
/* on = 0: off; 1: every family; 1 | (family_bitmask << 1): only the selected families (each timed launch costs two event
 * records on its stream, so a throughput run instruments just the kernel it reports). */
int sdrpp_timing_enable(sdrpp_ctx* ctx, int on);
int sdrpp_timing_read(sdrpp_ctx* ctx, double* ms_per_family, int64_t* launches_per_family);
const char* sdrpp_kernel_family_name(int family);

#ifdef __cplusplus
}
#endif
#endif /* SDRPP_GPU_H */
