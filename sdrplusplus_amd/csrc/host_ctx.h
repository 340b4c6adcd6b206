// The context: constants, per-stream / per-VFO state, struct sdrpp_ctx (what one IQ stream on one GPU owns).
// Part of the one translation unit sdrpp_gpu.hip (included there, in order; not a stand-alone header).
#pragma once

namespace {

constexpr int kArenaSlots = 24;     // >= kTickDepth + 2: a block's job tables are read for kTickDepth ticks after their upload
constexpr size_t kArenaBytes = 4u << 20;
constexpr int kRing = 4;            // pipelined mode: buffers per per-block stream (a consumer runs at most 2 ticks behind its producer; + the gather)
constexpr int kTickDepth = 18;      // pipelined mode: levels 0 .. kTickDepth of a block (see the level table at emit()): pre-processing chain 3 + VFO chain 5 + AF chain 5 + result copy
constexpr int kResSlots = SDRPP_RESULT_SLOTS;       // pipelined mode: page-locked result slots, one per LAUNCH GROUP (sdrpp_set_pipeline_group: 1 .. kGroupMax blocks) whose results the host has not released yet
constexpr int kGroupMax = SDRPP_GROUP_MAX;          // pipelined mode: blocks one launch may carry
constexpr int kResMeta = kResSlots * kGroupMax;     // ... and what the host knows about every block of those groups (ring by ticket)
constexpr int kStageSlots = 4;      // pipelined mode: page-locked staging buffers for pushes from pageable host memory
constexpr int kChanMaxTaps = 65536;  // channel filter (rx_vfo.h:60-70): a sanity bound only — its delay line is sized from the tap count and grown by sdrpp_vfo_set_channel_taps (CW: lowPass(25, 2.5, 3000) has 4 560 taps)
constexpr int kAfHpfMaxTaps = 65536;  // AF high-pass (sdrpp_vfo_set_af): a sanity bound only, its history is sized from the tap count (include/sdrpp_gpu.h)
constexpr int kFmifTile = SDRPP_FMIF_TILE;       // FMIF: outputs per matrix tile = the largest bin count (radio_module.h:31-36); its input stream remembers kFmifTile - 1 samples
constexpr int kFmifSeg = SDRPP_FMIF_SEG;       // ... and samples per segment job (one wavefront each): the cut depends on the block alone, never on the launch shape
constexpr size_t kScratchBytes = 64u << 20;
constexpr int kMaxLds = 64 * 1024;

enum Family { F_FFT1 = 0, F_FFT2, F_FFTS, F_ZOOM, F_S1, F_DECIM, F_POLY, F_FIR, F_DEMOD, F_MISC, F_AF, F_PIPE, F_TICK };
const char* kFamilyNames[SDRPP_NUM_KERNEL_FAMILIES] = { "fft_pass1", "fft_pass2", "fft_single", "zoom_palette", "vfo_stage1",
                                                        "vfo_decim", "vfo_poly",  "vfo_fir",    "demod",        "carry_misc", "af_chain",  "vfo_pipe", "tick" };

struct Stream {
    int width = 2;
    int hist_len = 0;
    float* data = nullptr;
    float* base = nullptr;  // the allocation `data` lives in (data = base + skew, see stream_alloc)
    size_t cap = 0;  // samples
    float* hist[2] = { nullptr, nullptr };
    int cur = 0;
    int n = 0;
    // pipelined mode: the other kRing - 1 data buffers (base allocations); `base` / `data` rotate through them block by block so that
    // the producer of block n + 1 does not overwrite what a consumer of block n still reads (stream_rotate)
    float* extra[kRing - 1] = {};
    int n_extra = 0, rot = 0;
    int clevel = 0;  // pipelined mode: level of the role that consumes this stream with memory (its history carry runs there)
    int wlevel = 0;  // pipelined mode: level of the role that WRITES this stream in the current block (0: not written by a role of this plan)
};

// Tap tables of the matrix-core FIR kernel (vfo_toep_kernel): zero-padded taps + per-lane base indices (one set per carried
// resampler phase).
struct ToepTab {
    float* d_tl = nullptr;
    int* d_lb = nullptr;  // [nvar][64]
    int tl_len = 0, nsteps = 0, s_in = 0, rows = 0, nvar = 0;
    bool ok = false;
};

// A description of a rate chain as all four entry points can fill it (rate_desc, host_util.h): the fields the public structs share under these names.
struct RateDesc {
    int n_stages = 0, stage_decim[SDRPP_MAX_DECIM_STAGES] = {}, stage_ntaps[SDRPP_MAX_DECIM_STAGES] = {};
    const float* stage_taps[SDRPP_MAX_DECIM_STAGES] = {};
    int interp = 1, decim = 1, resamp_ntaps = 0;
    const float* resamp_taps = nullptr;
};
// A rate chain: the reference's PowerDecimator (power-of-two decimator stages) and, where interp != decim, its PolyphaseResampler behind them — the RxVFO
// front end, the radio's AF chain, the WFM RDS branch and the IQ pre-processing chain each hold one (checked, built and freed by rate_* in host_util.h,
// planned by decim_step / poly_step).  Its streams live with its owner.
struct RateChain {
    // the description (a chain without a polyphase stage: interp = decim = 1, tpp = 0, no rtaps)
    int n_stages = 0, decim_s[SDRPP_MAX_DECIM_STAGES] = { 1, 1, 1, 1 };
    std::vector<float> staps[SDRPP_MAX_DECIM_STAGES], rtaps;
    int interp = 1, decim = 1, tpp = 0;
    // device constants
    float* d_staps[SDRPP_MAX_DECIM_STAGES] = { nullptr, nullptr, nullptr, nullptr };  // phase-major, padded (FirBJob); natural order where the owner asked for that (RateForm)
    int s_kp[SDRPP_MAX_DECIM_STAGES] = { 0, 0, 0, 0 };
    ToepTab tp_stage[SDRPP_MAX_DECIM_STAGES], tp_poly;
    float* d_bank = nullptr;
    bool bank_borrowed = false;  // d_bank is somebody else's allocation: rate_free leaves it alone
    // integer streaming state
    struct Pos { int soff[SDRPP_MAX_DECIM_STAGES]; int pphase, poff; } pos{};
    int ntaps(int s) const { return (int)staps[s].size(); }
    bool has_poly() const { return tpp > 0; }
    // History the input of block `stage` keeps (0 .. n_stages - 1: the decimators, n_stages: the polyphase stage): its consumer's taps - 1; behind the last
    // block of the chain whatever the owner's next consumer needs (`tail`).
    int need(int stage, int tail) const {
        if (stage < n_stages) { return ntaps(stage) - 1; }
        return (stage == n_stages && has_poly()) ? tpp - 1 : tail;
    }
};

struct Vfo {
    bool nco_exact = false;        // this VFO runs the reference's float rotator recursion (desc.nco_mode, else the context's mode)
    int id = 0;
    sdrpp_vfo_desc d{};  // demodulator, AGC, deviation, NCO mode; its rate-chain fields are not read once the VFO is built (`rate` holds them)
    RateChain rate;  // power-of-two decimators + resampler of the RxVFO (stage 0, or stages 0 and 1, inside the front-end kernels)
    std::vector<float> ctaps_chan, ataps;
    // NCO
    double theta = 0.0, phi = 0.0;
    std::vector<float2> modtaps;  // stage-1 modulated taps
    bool modtaps_dirty = true;
    long long seen = 0;  // input samples this VFO has consumed since it was added / reset (bounds its view of the IQ history)
    // device constants
    float* d_staps_nat[SDRPP_MAX_DECIM_STAGES] = { nullptr, nullptr, nullptr, nullptr };  // natural order (fused front kernel)
    float* d_cyc = nullptr;  // blocked polyphase: [interp][rows][lmax] cycle tap tables (one per carried phase)
    int cyc_rows = 0, cyc_lmax = 0;
    int chan_kp = 0, audio_kp = 0;
    float* d_chan = nullptr;
    int chan_ntaps = 0;
    std::vector<float> chan_stale;  // what the channel filter's delay line held when the filter was last bypassed (sdrpp_vfo_set_channel_taps)
    float* d_audio = nullptr;
    int audio_ntaps = 0;
    // device loop state: [AgcState agc][AgcState carrier][float dc]
    char* d_state = nullptr;
    double theta2 = 0.0, phi2 = 0.0;
    // streams: 0..nstages-1 decimator outputs (index 0 also used by the rotate-only path), then poly, chan, dem, out
    std::vector<Stream> st;
    int i_first = 0, i_poly = -1, i_chan = -1, i_dem = -1, i_out = -1, i_if = 0;
    int i_ifc = -1;  // the IF chain's output stream: a slot of `st` from the start, its buffers allocated when a chain is first attached (sdrpp_vfo_set_if)
    int i_fmi = -1;  // what FMIF reads while the blanker / squelch run in front of it (their output): a slot like i_ifc, allocated with the first such chain
    int lvl_if = 1, lvl_out = 1, lvl_af = 1, lvl_ifc = 1;  // levels (do_vfos_plan) at which the IF stream / the demodulator's output / the AF chain's output / the IF chain's output of the most recent block are written
    // radio IF chain between st[i_if] and the demodulator: NoiseBlanker -> PowerSquelch (sdrpp_vfo_set_if) -> FMIF (sdrpp_vfo_set_fmnr)
    struct Ifc {
        bool on = false;  // a chain is attached (both blocks may still be disabled: then nothing is planned for it)
        int nb_on = 0, sq_on = 0;
        float nb_rate = 0.0f, nb_level = 0.0f, sq_level = 0.0f;
        float* d_amp = nullptr;  // NoiseBlanker::amp (device, persistent)
        // FMIF (noise_reduction/fm_if.h): the last block of the chain, switched by a call of its own
        bool fm_on = false;
        int fm_bins = 32;            // radio_module.h:91
        std::vector<float> fm_line;  // FMIF's delay line (kFmifTile - 1 complex samples, newest last) while no stream's history holds it: see fmif_line_save
        bool nbsq() const { return on && (nb_on || sq_on); }
        bool active() const { return nbsq() || fm_on; }
    } ifc;
    // recorder sink (sdrpp_vfo_set_rec): parameters only, no streaming state; reads what result_stream() names
    struct Rec {
        bool on = false;
        float volume = 1.0f, gain = 1.0f;  // gain = powf(volume, 2) (audio/volume.h:14,22)
        int mono = 0, type = 1, ignore_silence = 0;
    } rec;
    // RDS branch of the WFM demodulator (sdrpp_vfo_set_rds): fed by the stream the demodulator reads, beside the audio low-pass.  Its streams are its own
    // (not in `st`: sdrpp_vfo_reset, which clears every history of `st`, leaves the branch alone, as BroadcastFM::reset leaves xlator and rdsResamp alone)
    struct Rds {
        bool attached = false, on = false;
        bool exact = false;            // the reference's float recursion (the VFO's nco_exact when the branch was attached)
        float pd_re = 1.0f, pd_im = 0.0f;
        double theta = 0.0, phi = 0.0;  // closed-form NCO: turns per sample, phase of the next sample
        float2* d_rot = nullptr;       // reference-rotator mode: FrequencyXlator::phase (device, persistent)
        RateChain rate;                  // stage 0 in closed form: natural-order taps, no matrix table; the polyphase bank is borrowed and has no table (5000 phases)
        unsigned long long bank_key = 0;  // the context's shared polyphase bank this branch holds a reference to (0: none)
        int tile = 0, pitch = 0;       // fused first stage: outputs per tile, LDS row pitch (rds_tile_geometry)
        std::vector<Stream> st;        // [exact: the rotated IF-rate stream,] the decimator stages' outputs, the polyphase stage's
        int i_stage0 = 0, i_poly = -1, i_last = 0;
        // the first decimator's delay line while the feed's history does not hold it (fresh attach: zeros; switched off, sdrpp_vfo_reset, moved: what the
        // branch was fed last): the K0 newest DISCRIMINATOR values, newest last; `frozen`: the next block reads it in place of the feed's history.  It stays
        // frozen until the branch has been fed K0 samples in a row since the last switch (`line_fed`): a block shorter than that is spliced onto the line
        // (vfo_rds_line_body, from d_line[line_cur] into the other side) — the feed's own history would still hold samples the branch never saw.  A line of
        // values, not of IF samples, has no seams: any number of switches may fall into that window
        float* d_line[2] = { nullptr, nullptr };
        int line_cur = 0, line_fed = 0;
        bool frozen = false;
        int lvl = 1;                   // level (do_vfos_plan) at which the branch's output of the most recent block is written
        bool ran = false;              // the most recent block was planned with the branch on
        std::vector<int> tk;           // a launch group: cumulative output counts at every push end
    } rds;
    // Stereo branch of the WFM demodulator (sdrpp_vfo_set_stereo; broadcast_fm.h:147-191): while it is on it REPLACES the audio low-pass job — pilot filter, PLL and
    // matrix write the VFO's output stream.  Its streams are its own, with histories like every stream: the discriminator values m (the two delay lines and,
    // through them, the two audio filters' lines), the pilot's angles (no memory) and the loop phases (the audio filters' lines).  The loop's (phase, freq) live
    // on the device.  Switching it on or off is BroadcastFM::setStereo -> reset(): stereo_reset_demod (vfo_ctl.h)
    struct Stereo {
        bool attached = false, on = false;
        std::vector<float> ptaps;      // K complex pilot taps, interleaved
        int K = 0, delay = 0;
        float alpha = 0.0f, beta = 0.0f, init_freq = 0.0f, min_freq = 0.0f, max_freq = 0.0f;
        float* d_ptaps = nullptr;
        float2* d_state = nullptr;     // PhaseControlLoop::phase, ::freq (device, persistent)
        std::vector<Stream> st;        // [0] m, [1] pilot angle, [2] loop phase: real streams at the IF rate
        bool ran = false;              // the most recent block was planned with the branch on
    } stereo;
    // Symbol branch of a RAW VFO (sdrpp_vfo_set_symbols; pocsag/dsp.h, clock_recovery/mm.h): discriminator -> shaping FIR (front) -> MM clock recovery (loop), off
    // the stream a demodulator would read.  Everything it remembers is its own and lives on the device — switched off it freezes while the VFO's streams move
    // on: the front's two carried lines in two sides (vfo_sym_kernels.h; `cur`: the side the next block reads) and the loop's four words.  Its per-block
    // buffers are streams without history, so that pipelined mode gives them its ring like every other per-block buffer.
    struct Sym {
        bool attached = false, on = false;
        float inv_deviation = 0.0f, omega = 0.0f, mu_gain = 0.0f, omega_gain = 0.0f, min_omega = 0.0f, max_omega = 0.0f;
        int K = 0, phases = 0, T = 0;
        std::vector<float> taps;
        unsigned long long bank_key = 0;  // the context's shared interpolator bank this branch holds a reference to (0: none)
        const float* d_bank = nullptr;    // ... borrowed
        float* d_taps = nullptr;
        float* d_lines = nullptr;         // two sides of K + T floats: K - 1 discriminator values and the previous phase, then T - 1 filter outputs (SymFrontJob)
        int cur = 0;
        float* d_state = nullptr;         // pcl.phase, pcl.freq, lastOut, offset
        int min_step = 1;                 // floorf(min_omega - |mu_gain|) >= 1: a block of n samples starts at most ceil(n / min_step) + 1 symbols
        std::vector<Stream> st;           // [0] the front's [T - 1][n] floats, [1] soft values, [2] bits (bytes), [3] symbols per push (ints)
        int lvl = 1;                      // level (do_vfos_plan) at which the loop of the most recent block runs
        bool ran = false;                 // the most recent block was planned with the branch on
        int n_if = 0, npush = 0, cap = 0; // ... its samples, its pushes, the symbols its outputs have room for
        int cap_of(int n) const { return (n + min_step - 1) / min_step + 1; }
    } sym;
    // RDS demodulator (sdrpp_vfo_set_rds_demod; decoder_modules/radio/src/rds_demod.h): AGC, two Costas loops around a complex band-pass, MM clock recovery, slicer,
    // differential decoder — one wavefront job per block (vfo_rdsd_kernels.h), behind the RDS branch's output (source 0, WFM) or behind the stream a demodulator
    // would read (source 1, RAW).  Everything it remembers is its own, in ONE device array updated in place; switched off it freezes.  Its per-block buffers are
    // streams without history, as the symbol branch's are.
    struct Rdsd {
        bool attached = false, on = false;
        int source = 0;
        float agc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };   // set point, max gain, rate, initial gain
        float loop[2][6] = {};                       // alpha, beta, initial phase, initial frequency, min / max frequency
        float omega = 0.0f, mu_gain = 0.0f, omega_gain = 0.0f, min_omega = 0.0f, max_omega = 0.0f;
        int K = 0, phases = 0, T = 0;
        unsigned long long bank_key = 0;  // the context's shared tap table + interpolator bank this demodulator holds a reference to (0: none)
        const float* d_taps = nullptr;    // ... borrowed
        const float* d_bank = nullptr;
        float* d_state = nullptr;         // SDRPP_RDSD_STATE_HEAD words, K - 1 complex values, T - 1 floats (RdsdJob)
        int min_step = 1;                 // as Sym::min_step
        std::vector<Stream> st;           // [0] soft values, [1] bits (bytes), [2] symbols per push (ints)
        int lvl = 1;                      // level (do_vfos_plan) at which the job of the most recent block runs
        bool ran = false;                 // the most recent block was planned with the demodulator on
        int n_in = 0, npush = 0, cap = 0; // ... its samples, its pushes, the symbols its outputs have room for
        int cap_of(int n) const { return (n + min_step - 1) / min_step + 1; }
    } rdsd;
    // Meteor QPSK demodulator (sdrpp_vfo_set_qpsk; decoder_modules/meteor_demodulator/src/meteor_demod.h): root-raised-cosine FIR, AGC, QPSK Costas loop, OQPSK
    // delay, complex MM — the filter as segment jobs over the stream a demodulator would read (RAW), everything sequential as one wavefront job a level behind
    // (vfo_qpsk_kernels.h).  Everything it remembers is its own: the filter's two-sided line (the host flips `cur` per block that has samples) and ONE device
    // array updated in place; switched off it freezes.  Its per-block buffers are streams without history.
    struct Qpsk {
        bool attached = false, on = false;
        float agc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };   // set point, max gain, rate, initial gain
        float loop[6] = {};                          // alpha, beta, initial phase, initial frequency, min / max frequency
        int broken = 0, oqpsk = 0;                   // MeteorCostas::_broken, Meteor::_oqpsk (sdrpp_vfo_qpsk_set_mode)
        float omega = 0.0f, mu_gain = 0.0f, omega_gain = 0.0f, min_omega = 0.0f, max_omega = 0.0f;
        float soft_scale = 0.0f;
        int K = 0, phases = 0, T = 0;
        unsigned long long bank_key = 0;  // the context's shared tap table + interpolator bank this demodulator holds a reference to (0: none)
        const float* d_taps = nullptr;    // ... borrowed
        const float* d_bank = nullptr;
        float* d_lines = nullptr;         // the filter's line: two sides of 2 K floats (QpskFrontJob)
        int cur = 0;                      // ... the side the next block reads
        float* d_state = nullptr;         // SDRPP_QPSK_STATE_HEAD words, T - 1 complex values (QpskLoopJob)
        int min_step = 1;                 // as Sym::min_step
        std::vector<Stream> st;           // [0] the filter's output (complex), [1] soft symbols (complex), [2] int8 pairs, [3] symbols per push (ints)
        int lvl = 2;                      // level (do_vfos_plan) at which the loop job of the most recent block runs
        bool ran = false;                 // the most recent block was planned with the demodulator on
        int n_in = 0, npush = 0, cap = 0; // ... its samples, its pushes, the symbols its outputs have room for
        int cap_of(int n) const { return (n + min_step - 1) / min_step + 1; }
    } qpsk;
    // Framer behind the symbol branch (sdrpp_vfo_set_framer; m17_decoder/src/m17dsp.h: M17Slice4FSK, M17FrameDemux): one wavefront job per block a level behind
    // the branch's loop (vfo_frame_kernels.h), reading the loop's soft values and per-push counts of the same block.  Everything it remembers is ONE device array
    // updated in place; switched off — or with the branch switched off — it freezes.  Its per-block buffers are streams without history, as the branch's are.
    struct Frame {
        bool attached = false, on = false;
        float high_cut = 0.0f;
        int n_sync = 0;
        uint16_t sync[4] = { 0, 0, 0, 0 };
        int frame_bits = 0, stride = 0;
        unsigned long long tab_key = 0;    // the context's shared table (interleave and scramble in one word per bit) this framer holds a reference to (0: none)
        const uint32_t* d_table = nullptr; // ... borrowed
        uint32_t* d_state = nullptr;       // SDRPP_FRAME_STATE_HEAD words, then the part-built frame, a byte per position (FrameJob)
        std::vector<Stream> st;            // [0] records (bytes), [1] frames per push (ints)
        int lvl = 3;                       // level (do_vfos_plan) at which the job of the most recent block runs
        bool ran = false;                  // the most recent block was planned with the framer (and its branch) on
        int npush = 0, cap = 0;            // ... its pushes, the records its output has room for
        int cap_of(int sym_cap) const { return (16 + 2 * sym_cap) / (16 + frame_bits) + 1; }
    } frame;
    std::vector<int> tk_if, tk_af;  // a launch group of several pushes: cumulative sample counts of the IF / demodulator stream and of the AF chain's output at every push end
    ToepTab tp_chan, tp_audio;
    // front end as one filter (what the fused translate + filter kernels evaluate): stages 0 (+ 1) of the plan
    bool fused_front = false;      // stages 0 and 1 run as one composite filter (front2_t2 > 0)
    bool no_fuse = false;          // stage-1 taps are not linear phase: the composite forms do not apply
    unsigned long long tap_hash = 0;  // of the stage-0 / stage-1 taps: only VFOs with identical taps share a front-end job
    float* d_h12 = nullptr;        // composite (or stage-0) taps, real, natural order — used by the retune hand-over kernel
    int h12_K = 0, h12_lgD = 0;
    // RxVFO::setOffset hand-over (closed-form NCO): retune points whose old-increment samples a filter window can still reach
    struct Retune { long long pos; double theta_before; };  // pos: input samples consumed (Vfo::seen) when the increment changed
    std::vector<Retune> recs;
    // reference-rotator mode (sdrpp_set_nco_mode): rotated full-rate stream + persistent float phases (main xlator, SSB xlator)
    int i_rot = -1;
    float2* d_rot = nullptr;
    // radio AF chain (sdrpp_vfo_set_af): RationalResampler<stereo_t> -> high-pass -> de-emphasis, fed by st[i_out]
    struct Af {
        bool on = false;
        RateChain rate;
        std::vector<float> htaps;
        ToepTab tp_hpf;
        float* d_hpf = nullptr;
        int hpf_kp = 0;
        float alpha = 0.0f;
        float2* d_last = nullptr;  // Deemphasis::lastOut: two slots, read from [state_cur], written to the other (DeempJob)
        int state_cur = 0;
        float4* d_seg = nullptr;   // per-segment affine maps of the de-emphasis scan
        int seg_cap = 0;
        int i_stage0 = -1, i_poly = -1, i_hpf = -1, i_deemp = -1, i_last = -1;  // indices into st (i_last: where the AF output is)
        int base = -1;  // first AF stream in st (they are appended behind the VFO's own streams)
    } af;
};
// Every stream of a VFO: its own, then its RDS branch's, its stereo branch's, its symbol branch's, its RDS demodulator's, its QPSK demodulator's and its framer's (the order plan_snapshot records them in).  ran_only: a branch's streams
// only if the most recent plan ran the branch.
template <class F>
void for_each_stream(Vfo& v, F&& f, bool ran_only = false) {
    for (auto& s : v.st) { f(s); }
    if (!ran_only || v.rds.ran) {
        for (auto& s : v.rds.st) { f(s); }
    }
    if (!ran_only || v.stereo.ran) {
        for (auto& s : v.stereo.st) { f(s); }
    }
    if (!ran_only || v.sym.ran) {
        for (auto& s : v.sym.st) { f(s); }
    }
    if (!ran_only || v.rdsd.ran) {
        for (auto& s : v.rdsd.st) { f(s); }
    }
    if (!ran_only || v.qpsk.ran) {
        for (auto& s : v.qpsk.st) { f(s); }
    }
    if (!ran_only || v.frame.ran) {
        for (auto& s : v.frame.st) { f(s); }
    }
}
template <class F>
void for_each_stream_that_ran(Vfo& v, F&& f) { for_each_stream(v, f, true); }

struct TimingPair { hipEvent_t a, b; int family; };

}  // namespace

struct sdrpp_ctx {
    int device = 0;
    int64_t max_push = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;         // main stream (VFO bank, copies); may be the caller's
    hipStream_t fft_stream = nullptr;     // FFT branch runs here, concurrently with the VFO bank (HBM-bound vs VALU-bound)
    hipStream_t launch_stream = nullptr;  // stream the next launches / timers go to
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    std::string devinfo;

    // input: landing buffers of host pushes / of a deferred pass (max_push complex each), ping-pong per pass so that the copies of the
    // next pass overlap the kernels of the current one; copies run on their own stream and are host-synchronised (the caller's
    // buffer is free again when sdrpp_push returns, like a dsp::stream read buffer after flush())
    float* iq_land[2] = { nullptr, nullptr };
    int16_t* iq_land16[2] = { nullptr, nullptr };   // the raw bytes of sdrpp_push_raw / _push_int16 (4 bytes per sample at most), converted into iq_land by ingest_kernel
    float* d_u8_tab = nullptr;                      // the SDRPP_IQ_U8 table of ordinary / deferred passes ...
    std::vector<float> u8_tab;                      // ... and what it holds (uploaded when a push brings another one)
    hipEvent_t land_ev[2] = { nullptr, nullptr };   // recorded behind the pass that read the buffer
    bool land_used[2] = { false, false };
    int land_cur = 0;
    hipStream_t copy_stream = nullptr;
    hipStream_t side_stream = nullptr;   // sdrpp_device_copy: copies that may come from ANOTHER thread than the one driving the context (created with the context, never changed)
    std::mutex side_mtx;                  // ... one at a time
    bool async_staged = false;     // sdrpp_push_pinned_async copies enqueued since the last pass (the pass waits for them on the device)
    bool async_inflight = false;   // ... and not yet known to have landed: cleared only by a HOST synchronisation of the copy stream (sdrpp_push_wait)
    hipEvent_t ev_copy = nullptr;
    // deferred processing (sdrpp_set_deferred): pushes are only staged; the next observing call processes them as ONE pass
    bool deferred = false;
    int64_t pending = 0;
    std::vector<int> pend_ends;       // cumulative end of every staged push
    float* iq_hist[2] = { nullptr, nullptr };
    int iq_hist_cap = 0;              // samples of history kept
    int iq_cur = 0;

    // IQFrontEnd pre-processing chain (sdrpp_preproc_configure): PowerDecimator -> DCBlocker -> Conjugate on the wideband stream,
    // in front of the FFT branch and the VFO bank (iq_frontend.cpp:32-39)
    struct Pre {
        bool ref_order = false;            // sdrpp_preproc_set_reference_order: the reference's own summation order / sequential DC blocker
        bool on = false;
        RateChain rate;  // decimator stages only
        float dc_rate = 0.0f;
        int conj = 0;
        Stream raw;               // history of the caller's buffer (data stays the caller's)
        std::vector<Stream> st;   // decimator stage outputs
        Stream out;               // DC blocker / conjugate output
        float2* d_off = nullptr;  // DCBlocker::offset: two slots like Vfo::Af::d_last
        int state_cur = 0;
        float4* d_seg = nullptr;
        int seg_cap = 0;
        const float* last = nullptr;  // what the chain handed on for the most recent push
        int last_n = 0;
    } pre;

    // WaterFall display state (sdrpp_wf_*): raw-line ring in HBM, FFT trace smoothing / hold
    struct Wf {
        int height = 0;
        float* d_ring = nullptr;  // [height][fft_size]
        int cur = 0, lines = 0;   // currentFFTLine, fftLines (waterfall.cpp:879-882)
        int width = 0;            // data_width the trace arrays were sized for
        float* d_latest = nullptr;
        float* d_smooth = nullptr;  // nullptr = smoothing off
        float* d_hold = nullptr;
        bool hold_on = false, have_latest = false;
        float alpha = 0.0f, beta = 1.0f, hold_speed = 0.0f;
    } wf;

    // signal meters (sdrpp_wf_set_meters): a table of bands, evaluated on every raw line a push completes (fft_kernels.h: wf_meter_body)
    struct Meters {
        std::vector<sdrpp_meter_desc> descs;  // the bands as frequencies: the table survives a change of the FFT size
        double whole_bandwidth = 0.0;
        std::vector<WfMeterOffs> offs;        // ... and as bin offsets at the current FFT size (wf_meter_offsets); pipelined blocks carry a copy among their job tables
        WfMeterOffs* d_offs = nullptr;        // the same in device memory, for ordinary passes
        float* d_out = nullptr;               // [lines][n][2] of the most recent ordinary pass
        size_t out_cap = 0;                   // floats
        int out_lines = 0, out_n = 0;         // what d_out holds
        int n() const { return (int)descs.size(); }
    } meters;

    char* d_pack = nullptr;  // scratch of the packed-sample reads (sdrpp_vfo_read_pcm / _compressed)
    size_t pack_cap = 0;
    float2* d_gather = nullptr;     // sdrpp_vfo_read_many: packed outputs + job table
    size_t gather_cap = 0;          // samples
    GatherJob* d_gather_jobs = nullptr;
    int gather_jobs_cap = 0;

    // job arena
    char* arena_host[kArenaSlots] = {};
    char* arena_host_dev[kArenaSlots] = {};  // device-side address of the same pinned memory
    hipEvent_t arena_ev[kArenaSlots] = {};
    bool arena_used[kArenaSlots] = {};
    char* arena_dev_slot[kArenaSlots] = {};  // a device arena per slot: the job tables of a block outlive its first launch in pipelined mode
    char* arena_dev = nullptr;               // = arena_dev_slot[arena_slot]
    int arena_slot = 0;
    size_t arena_off = 0;

    // FFT
    bool fft_on = false;
    int fft_size = 0, fft_lg = 0, nz = 0, skip = 0;
    float* d_window = nullptr;
    float2* d_tw1 = nullptr;   // tw(e, N1) / tw(e, N) for single pass, e < L/2
    float2* d_tw2 = nullptr;
    float2* d_twn = nullptr;   // [k1][n2] tw(n2*k1, N)
    float2* d_scratch = nullptr;
    float* d_lines = nullptr;
    float* d_lines_grp = nullptr;  // per line: maxima of aligned groups of zoom_grp bins (pass 2 writes them for the zoom kernel); N > 4096 only
    int zoom_grp = 0;
    size_t lines_cap = 0;
    int64_t fft_pos = 0, fft_next = 0;
    int n_lines = 0;
    // view
    int view_start = 0, view_size = 0, data_width = 0;
    float wf_min = -120.0f, wf_max = 0.0f;
    int32_t* d_zstart = nullptr;
    std::vector<int32_t> h_zstart, h_zcount;  // host copies of the view's pixel ranges (zoom_lanes)
    int zoom_tp_cache = 0, zoom_tp_grp = -1;     // lanes per pixel for (the view, zoom_grp == zoom_tp_grp)
    int32_t* d_zcount = nullptr;
    float* d_zoomed = nullptr;
    int32_t* d_index = nullptr;
    size_t zoom_cap = 0;
    // pipelined mode: the other kRing - 1 sets of the per-block FFT buffers (scratch, lines, group maxima, zoomed, index); the members
    // above rotate through them block by block (fft_ring_rotate), so they always name the buffers of the most recent block
    struct FftBufs { float2* scratch = nullptr; float* lines = nullptr; float* grp = nullptr; float* zoomed = nullptr; int32_t* index = nullptr; };
    FftBufs fft_extra[kRing - 1];
    int fft_extra_n = 0, fft_rot = 0;

    // reference block structure / NCO flavour (sdrpp_set_reference_block, sdrpp_set_nco_mode)
    int ref_block = 0;             // 0: one push = one reference block
    int nco_exact = 0;             // 1: the reference's float rotator recursion instead of the closed-form NCO
    int pipe_on = 1;               // FM back ends as one pipelined launch where that pays (sdrpp_set_backend_pipeline)
    bool pipe_launched = false;    // since the last host synchronisation that looked at the kernels' timeout counter (pipe_timeouts_check)
    int timeouts_seen = 0;         // value of the counter (h_tick_flag[8]) at that look
    std::vector<int> vfo_bounds;   // reference-block ends (cumulative sample counts) of the current push at the VFO bank's input

    // VFOs
    std::map<int, std::unique_ptr<Vfo>> vfos;
    std::vector<Vfo*> vfo_list;           // the same VFOs in id order (rebuilt on add / remove): what the per-block loops walk
    int next_id = 1;
    // cached stage-1 job tap arrays, keyed by membership signature
    std::map<std::string, float2*> s1_tap_cache;  // key = 16 raw bytes: two independent 64-bit hashes of (kind, member ids, increments)
    std::map<int, float*> fmif_tabs;      // FMIF's matrix per bin count in use (sdrpp_host::fmifMatrix), uploaded once
    struct RdsBank { float* d_bank = nullptr; int refs = 0; int interp = 0, tpp = 0; std::vector<float> taps; };
    std::map<unsigned long long, RdsBank> rds_banks;  // polyphase banks of the RDS branches, ONE per distinct description (2.4 MB each), freed with their last user

    struct SymBank { float* d_bank = nullptr; int refs = 0; int phases = 0, T = 0; std::vector<float> taps; };
    struct RdsdBank { float* d_taps = nullptr; float* d_bank = nullptr; int refs = 0; int K = 0, phases = 0, T = 0; std::vector<float> taps, bank; };
    std::map<unsigned long long, RdsdBank> rdsd_banks;  // tap table + interpolator bank of the RDS demodulators, ONE pair per distinct description, freed with their last user
    struct QpskBank { float* d_taps = nullptr; float* d_bank = nullptr; int refs = 0; int K = 0, phases = 0, T = 0; std::vector<float> taps, bank; };
    std::map<unsigned long long, QpskBank> qpsk_banks;  // real tap table + interpolator bank of the QPSK demodulators, ONE pair per distinct description, freed with their last user
    struct FrameTab { uint32_t* d_table = nullptr; int refs = 0; std::vector<uint32_t> words; };
    std::map<unsigned long long, FrameTab> frame_tabs;  // the framers' tables (interleave[k] | scramble[k] << 16), ONE per distinct pair, freed with their last user
    std::map<unsigned long long, SymBank> sym_banks;  // interpolator banks of the symbol branches, ONE per distinct bank, freed with their last user

    // ---- pipelined ("tick") execution: one launch per block, the stages of consecutive blocks skewed over consecutive launches
    //      (tick_kernels.h; sdrpp_set_pipelined) ----
    struct RoleLaunch { TickEntry e; size_t lds; int level; int fam; bool to_host; };  // to_host: a copy into a page-locked result slot
    struct Result {                       // what the host knows about one block's results (ring by ticket); the bytes live in its group's slot
        uint64_t ticket = 0;              // 0: entry free
        uint64_t done_tick = 0;           // its last level has run when this many ticks have completed
        bool held = false;                // handed out by sdrpp_result_wait, not yet released
        uint64_t group = 0;               // its launch group (alive while res_live still holds a region of that id)
        const char* base = nullptr;       // host address of the group's region in the result ring (stays valid for a held block when the ring is replaced by a larger one)
        int epoch = 0;                    // which ring `base` points into (res_epoch when the results were planned)
        std::vector<int> ids, counts;
        std::vector<int64_t> offsets;
        int n_lines = 0;
        int fft_size = 0, data_width = 0, flags = 0;        // what the block was PLANNED with (the view / FFT size / result flags may change before it is collected)
        size_t off_zoomed = 0, off_index = 0, off_raw = 0, off_iq = 0;  // byte offsets in the slot
        int n_iq = 0;                                        // pre-processed IQ samples delivered (result flag 8)
        std::vector<int> rds_ids, rds_counts;                // result flag 32: the VFOs whose RDS branch ran in the block, this push's samples
        std::vector<size_t> rds_off;                         // ... and where they lie in the slot
        std::vector<int> sym_ids, sym_push;                  // result flag 64: the VFOs whose symbol branch ran in the block, this push's index in its launch group
        std::vector<int> frame_ids, frame_push, frame_stride;  // result flag 512: the VFOs whose framer ran in the block, this push's index in its launch group, the record stride
        std::vector<size_t> frame_cnt_off, frame_rec_off;      // ... where the group's per-push frame counts and its records lie in the slot
        std::vector<size_t> sym_cnt_off, sym_soft_off, sym_bits_off;  // ... where the group's per-push counts, its soft values and its bits lie in the slot
        std::vector<int> rdsd_ids, rdsd_push;                // result flag 128: the VFOs whose RDS demodulator ran in the block, this push's index in its launch group
        std::vector<size_t> rdsd_cnt_off, rdsd_soft_off, rdsd_bits_off;  // ... where the group's per-push counts, its soft values and its bits lie in the slot (the symbol branch's layout)
        std::vector<int> qpsk_ids, qpsk_push;                // result flag 256: the VFOs whose QPSK demodulator ran in the block, this push's index in its launch group
        std::vector<size_t> qpsk_cnt_off, qpsk_soft_off, qpsk_packed_off;  // ... where the group's per-push counts, its float pairs (SIZE_MAX: not asked for) and its int8 pairs lie in the slot
        std::vector<int> rec_ids;                            // result flag 16: the VFOs that had a recorder sink when the block was planned,
        std::vector<size_t> rec_off, rec_info_off;           // ... where this push's converted samples and its sdrpp_rec_info lie in the slot
        int n_meters = -1;                                   // signal meters the block was pushed with (-1: no table then); its n_lines x n_meters x 2 floats
        size_t off_meters = 0;
    };
    bool pipelined = false;
    int res_flags = 0;                    // bit 0: gather every VFO's output, bit 1: zoomed lines + palette indices, bit 2: raw dB lines, bit 3: pre-processed IQ, bit 4: recorder sinks, bit 5: RDS branches (sdrpp_pipeline_set_rds_results), bit 6: symbol branches (sdrpp_pipeline_set_sym_results), bit 7: RDS demodulators (sdrpp_pipeline_set_rds_bits_results), bit 8: QPSK demodulators (sdrpp_pipeline_set_qpsk_results), bit 9: framers (sdrpp_pipeline_set_frame_results)
    bool res_qpsk_soft = false;           // ... with the float pairs beside the int8 pairs
    int num_cus = 256;
    int tick_l0_at = getenv("SDRPP_GPU_TICK_L0_AT") ? atoi(getenv("SDRPP_GPU_TICK_L0_AT")) : 0;  // (read when the context is created)
    // grid rules of the roles inside a tick (the stand-alone kernels size their grids for a GPU of their own; in a tick ~8 roles share it, and
    // fewer, longer workgroups amortise the per-workgroup prologues): environment overrides are for measurements
    // workgroups of a pass-1 / pass-2 launch (fft_walk_grid; 0: one tile per workgroup).  Measured on 65536-point frames, 2^24 samples per pass
    // (profiles/r03o_fft16_sweeps.log): pass 1 with 16 columns per workgroup 0.069 ms at one tile each, 0.064 walking from 1024 workgroups (four
    // per CU), 0.106 from 512; pass 2 0.0565 at one tile each, 0.057-0.061 walking (its tiles are contiguous 32 KB reads: nothing to hide)
    int fft_p1_grid = getenv("SDRPP_GPU_FFT_P1_GRID") ? atoi(getenv("SDRPP_GPU_FFT_P1_GRID")) : 1024;
    int fft_p2_grid = getenv("SDRPP_GPU_FFT_P2_GRID") ? atoi(getenv("SDRPP_GPU_FFT_P2_GRID")) : 0;
    int fft_tick_grid = getenv("SDRPP_GPU_FFT_TICK_GRID") ? atoi(getenv("SDRPP_GPU_FFT_TICK_GRID")) : 0;  // ... of a pass-1 / pass-2 role inside a tick (a shared GPU: 18.4 / 16.2 / 18.8 / 18.5 GS/s at 0 / 64 / 128 / 256; cfg 2: 61.7 / - / 57.0)
    // tiles a workgroup of those roles takes where no grid is forced (plan_fft.h: fft_tick_walk_grid): pass 1 the tiles of its columns from two consecutive
    // frames, pass 2 one pair of adjacent row tiles.  10^6-sample blocks, tick per block at 1 / 2 / 4 tiles for pass 1 (pass 2: 1 / 1 / 2 pairs): cfg 2
    // 13.25 / 12.0 / 17.3 us, cfg 3 45.28 / 45.43 / 48.3 us (parent 14.51 and 45.72: profiles/fft_roles_rate.md)
    int fft_tick_tiles = 2;
    int tick_zoom_groups = getenv("SDRPP_GPU_TICK_ZOOM_GROUPS") ? atoi(getenv("SDRPP_GPU_TICK_ZOOM_GROUPS")) : 8;
    int tick_fcm_waves = getenv("SDRPP_GPU_TICK_FCM_WAVES") ? atoi(getenv("SDRPP_GPU_TICK_FCM_WAVES")) : 768;
    // wavefronts the tiles of ONE matrix front-end job (vfo_frontcm / vfo_frontcl) are dealt out over, in a pass and in a tick alike; 0: the rules of
    // group_front / upload.  TEST-ONLY (a host never sets it: N wavefronts per job leave the device idle): small blocks then walk many tiles per wavefront, as 10^6-sample blocks do under the rules.
    int front_walk_waves = getenv("SDRPP_GPU_FRONT_WAVES") ? std::max(0, atoi(getenv("SDRPP_GPU_FRONT_WAVES"))) : 0;
    int tick_toep_blocks = getenv("SDRPP_GPU_TICK_TOEP_BLOCKS") ? atoi(getenv("SDRPP_GPU_TICK_TOEP_BLOCKS")) : 256;
    int tick_land_blocks = getenv("SDRPP_GPU_TICK_LAND_BLOCKS") ? std::max(1, atoi(getenv("SDRPP_GPU_TICK_LAND_BLOCKS"))) : 64;  // workgroups of a tick's landing copy (host-fed blocks), at most
    int tick_lds_cap = 24 * 1024;       // LDS window of the many-phase resampler as a role of a tick (launch_polyc)
    int tick_lds_cap_fir = 40 * 1024;   // ... of the register-blocked FIR roles (launch_fir)
    long arena_begins = 0;                // blocks planned so far (block_bounds: one per ordinary pass / per block of a pipelined run)
    int arena_allocs = 0;
    long test_fail_pass = 0;              // SDRPP_GPU_TEST_FAIL_ARENA (see arena_push)
    int test_fail_alloc = 0;
    bool pre_ref_order = false;           // survives sdrpp_preproc_configure (which rebuilds `pre`)
    float2 pre_dc_last = { 0.0f, 0.0f };  // the DC blocker's estimate when it was last looked at (sdrpp_preproc_reconfigure: the reference's block object lives on through every re-plan of the chain)
    std::vector<const volatile uint32_t*> stage_pend;  // sdrpp_push_staged_when: the block's first launch waits (on the host) for these words to reach 0
    bool rot_exact_single = getenv("SDRPP_GPU_ROT_EXACT_SINGLE") != nullptr;  // measurement switch: the one-wavefront form of the reference rotator
    // 32-output tiles per front-end job up to which the ratio-32 front end runs in its small-block shape (vfo_frontcm16_body); 0: never.
    // Unset: 256 for ordinary passes (sr/200 pushes 764 -> 814 MS/s) and for pipelined blocks that are read where they lie in device memory
    // (3.48 -> 3.96 GS/s), never for blocks the tick's landing copy fetches from host memory — workgroups that share a CU with a landing-copy
    // workgroup start 8 us late, which the longer front end hides and the short one does not (DESIGN_HISTORY.md 4b, profiles/r03zl-r03zn).
    int fcm16_max_tiles = getenv("SDRPP_GPU_FCM16_MAX_TILES") ? atoi(getenv("SDRPP_GPU_FCM16_MAX_TILES")) : -1;
    bool plan_block_from_host = false;    // the block being planned reaches the device through a landing copy
    // VFOs per workgroup of vfo_rotate_exact4_kernel (1 .. 64).  The chain wavefront costs the same for 1 or 64 VFOs (a lane each); the three
    // wavefronts that apply the phases take ~100 cycles per VFO and chunk: beyond ~16 VFOs they, not the chain, set the pace of the workgroup
    // and the input is 8 bytes per sample however often it is read.
    int rot_exact_vpw = [] { const char* e = getenv("SDRPP_GPU_ROTX_VPW"); const int v = e ? atoi(e) : 8; return v < 1 ? 1 : (v > 64 ? 64 : v); }();
    bool tick_planning = false;           // a block is being planned for the tick queue: emit() queues, plain launches abort the plan
    bool tick_abort = false;              // ... and met a launch that has no role in the tick kernel: the block runs as an ordinary pass
    int plan_top = 0;                     // highest level + 1 the block being planned uses
    int plan_lvl0 = 0;                    // levels the pre-processing chain of the block being planned takes in front of the FFT branch / VFO bank (pipelined mode; 0 in a pass)
    std::vector<RoleLaunch> emits;        // roles of the block being planned
    std::deque<std::vector<RoleLaunch>> tickq;  // [0]: roles of the next tick to launch, [1]: of the one after, ...
    uint64_t ticks = 0;                   // ticks launched so far
    uint64_t pushes = 0;                  // blocks accepted so far in pipelined mode (= ticket of the most recent one)
    uint64_t land_tick = 0;               // landing copies of every push so far have run when this many ticks have completed
    TickTable* next_tab = nullptr;        // device address of the role table of the next tick (uploaded by the tick before)
    int next_tab_n = 0;
    TickTable* empty_tab = nullptr;       // device: a table without roles
    unsigned* d_tick_counter = nullptr;   // device: finished workgroups, running total
    unsigned tick_target = 0;             // its value when every tick launched so far has finished
    unsigned* h_tick_flag = nullptr;      // page-locked: completed ticks (written by the last wavefront of each tick)
    unsigned* hd_tick_flag = nullptr;     // the same, device address
    uint64_t arena_tick[kArenaSlots] = {};  // pipelined: the tick that uploaded from this arena slot (+1; 0 = never)
    float* tick_land[3] = {};             // landing ring of host pushes (SDRPP_LAND_TABLE floats for a U8 table, then max_push complex each; allocated on first use)
    std::vector<float> tick_land_tab[3];  // the U8 table in front of each (empty: none uploaded yet)
    float* stage_host[kStageSlots] = {};  // page-locked staging of pushes from pageable memory (max_push complex each; allocated on first use)
    uint64_t stage_tick[kStageSlots] = {};  // the tick whose landing copy reads the slot (+1)
    int stage_cur = 0;
    int stage_open = -1;                  // slot handed out by sdrpp_push_stage and not yet pushed
    // Results in page-locked host memory: ONE ring of kResSlots x (what a launch of max_push samples can deliver), handed out in allocation order, a
    // region per launch group sized for what that group really delivers — 24 launches at the stream cap, ten times as many at the reference's block
    // size (a host that collects a fixed number of BLOCKS behind its pushes must not lose results because the groups happened to be small).  A region
    // is taken back, oldest first, when the ring comes round to it; one the host still holds fails the push that needs it.
    char* res_ring = nullptr;             // host address
    char* res_ring_dev = nullptr;         // ... and as the device sees it
    size_t res_ring_bytes = 0;
    size_t res_cap = 0;                   // what the largest possible launch delivers (tick_results_need)
    size_t res_head = 0;                  // next free byte
    int res_epoch = 0;                    // counts the rings (tick_results_ensure replaces the ring by a larger one)
    struct ResRegion { uint64_t gid; size_t off, bytes; int held; };
    std::deque<ResRegion> res_live;       // regions in use, in allocation order (front = oldest)
    struct ResRetired { char* ring; int epoch; int held; };
    std::vector<ResRetired> res_retired;  // smaller rings that held blocks the host had not released when the ring grew: its pointers stay valid until it does
    Result res[kResMeta];
    // ---- several blocks per launch (sdrpp_set_pipeline_group): pushes are HELD — nothing planned, nothing launched — until the group goes out as ONE
    //      block of the tick queue whose reference-block ends are the push ends (what a deferred pass does with its staged pushes, plan_push.h) ----
    int group_max = 1;                    // blocks per launch, at most
    int group_adaptive = 0;               // 1: a group goes out as soon as the device has fewer than two launches in flight (a host slower than the device: one block per launch)
    bool stage_pend_stable = false;       // sdrpp_set_pipeline_group flag 2: the words handed to sdrpp_push_staged_when stay valid until their block has been LAUNCHED — a held push does not wait for its copy
    struct Held {
        int kind = -1;                    // -1: nothing held; 0: device memory read in place; 1 / 2: float / raw (fmt_*: sdrpp_iq_format) samples in a page-locked staging slot; 3: the caller's page-locked memory
        int fmt_type = 0;                 // kind 2: the wire format every held push has
        float fmt_scalar = 0.0f;
        std::vector<float> fmt_table;     // ... SDRPP_IQ_U8: its 256 floats
        const char* base = nullptr;       // kind 0 / 3: address of the first block (the following ones are contiguous with it)
        int stage_slot = -1;              // kind 1 / 2
        int64_t total = 0;                // samples held
        std::vector<int> ends;            // cumulative end of every held push
    } held;
    std::vector<int> grp_ends;            // push ends of the group being planned (empty / one entry: a single block)
    int64_t plan_fft_pos0 = 0, plan_fft_next0 = 0;  // frame position in front of the block being planned (do_fft): which push of a group completes which line
    uint64_t groups = 0;                  // launch groups planned so far (a group's result slot: groups % kResSlots)
    int64_t stat_groups = 0, stat_group_blocks = 0, stat_group_max = 0;  // groups of more than one block, the blocks in them, the largest
    // Completion of a tick whose roles wrote RESULTS into page-locked host memory, as the host may rely on it: an event recorded behind the
    // launch.  The flag the kernel itself publishes (h_tick_flag) says that every workgroup has finished and its stores are acknowledged — but
    // a result block is megabytes of posted writes over the bus from every XCD, and the four bytes of the flag were measured to overtake them by
    // up to ~100 us (round 4: a host that copied a VFO block within microseconds of the flag met the slot's previous content).  The command
    // processor's end-of-kernel release behind an event is the ordering HIP guarantees for kernel writes to host memory.
    static constexpr int kTickEvents = 32;
    hipEvent_t tick_ev[kTickEvents] = {};
    uint64_t tick_ev_tick[kTickEvents] = {};   // the tick the event was last recorded behind (0: never)
    hipEvent_t tick_ev_start[kTickEvents] = {}; // timing on: the start event of that tick's launch (the pair is read out when the entry comes round again, or at timing_flush)
    int tick_ev_next = 0;
    uint64_t tick_ev_last = 0;                 // the newest tick an event stands behind
    void* bank_plan = nullptr;            // the context's BankPlan (plan_vfo.h), re-used block after block
    void (*bank_plan_free)(void*) = nullptr;
    // how the blocks of a pipelined run were executed (sdrpp_pipeline_stats: tests and bench.py assert the mode they mean to measure)
    int64_t stat_tick_blocks = 0, stat_pass_blocks = 0, stat_crowded = 0, stat_last_depth = 0, stat_last_table_bytes = 0;
    int64_t stat_role_wgs[64] = {};
    int64_t stat_pass_forms[96] = {};  // launches of an ordinary pass per form (sdrpp_pass_form_stats): [role] for the forms that are roles, then the PassForm extras (host_util.h)

    // timing
    bool timing = false;
    unsigned timing_mask = 0xffffffffu;  // families whose launches are bracketed by events while timing is on
    std::vector<TimingPair> tpairs;
    std::vector<hipEvent_t> ev_pool;
    double fam_ms[SDRPP_NUM_KERNEL_FAMILIES] = {};
    int64_t fam_launch[SDRPP_NUM_KERNEL_FAMILIES] = {};
};
