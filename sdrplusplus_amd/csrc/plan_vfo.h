// VFO bank of one block: per-VFO chains -> job lists per level -> front-end grouping -> launches / roles.
// Part of the one translation unit sdrpp_gpu.hip (included there, in order; not a stand-alone header).
#pragma once

namespace {

// ---- VFO bank: one push ------------------------------------------------------------------------------------------------------------
struct S1Member { Vfo* v; int K, lgD, off0, nout; double phi0; int min_idx; int fused, K2, lgD2, off2, nout2; unsigned long long taph;
                  int shift = 0, oshift = 0; };  // a push of a launch group: where its samples start in the group's block, where its outputs start in the group's output block

// Cache key of a front-end job's tap operand: membership (VFO ids) and NCO increments, as two independent 64-bit hashes (the job
// tables are rebuilt on every push: formatting 32 ids and doubles into a string cost more host time than the launch itself)
std::string member_key(char kind, const S1Member* m, int n) {
    unsigned long long h1 = 1469598103934665603ull ^ (unsigned char)kind, h2 = 0x9e3779b97f4a7c15ull + (unsigned char)kind;
    for (int i = 0; i < n; i++) {
        unsigned long long tb;
        memcpy(&tb, &m[i].v->theta, 8);
        const unsigned long long id = (unsigned long long)(unsigned)m[i].v->id;
        h1 = (h1 ^ id) * 1099511628211ull;
        h1 = (h1 ^ tb) * 1099511628211ull;
        h2 ^= id + 0x9e3779b97f4a7c15ull + (h2 << 6) + (h2 >> 2);
        h2 ^= tb + 0x9e3779b97f4a7c15ull + (h2 << 6) + (h2 >> 2);
    }
    char raw[16];
    memcpy(raw, &h1, 8);
    memcpy(raw + 8, &h2, 8);
    return std::string(raw, 16);
}

// Stage-2 outputs per block of the fused front kernel (0 = do not fuse: the recomputed overlap would dominate or LDS would overflow).
int front2_t2(int K1, int D1, int K2, int D2, int vt) {
    const int tile = 256;
    if (K2 >= tile) { return 0; }
    const int t2 = (tile - K2) / D2 + 1;
    if (t2 * D2 * 4 < tile * 3) { return 0; }  // more than 25 % of the stage-1 work would be recomputed overlap
    if (D2 < 2) { return 0; }
    const size_t lds = (std::max((size_t)D1 * (tile + (K1 - 1 + D1 - 1) / D1 + 1), (size_t)vt * (tile + 16)) + (size_t)vt) * sizeof(float2);
    return lds <= (size_t)kMaxLds ? t2 : 0;
}


// Matrix-core front kernel (composite stage 1 + 2 filter, one 32-output x 32-VFO tile per wavefront step): usable?  Picks the
// prefetch depth (IQ samples per lane) of the template variant.
bool frontcm_ok(int K1, int lgD1, int K2, int lgD2, int* pf) {
    const int K = K1 + (K2 - 1) * (1 << lgD1), lgD = lgD1 + lgD2;
    if (K < 9 || lgD < 1 || lgD > 5) { return false; }
    const int nsamp = (SDRPP_FCM_TILE - 1) * (1 << lgD) + K;
    if (nsamp > 16 * 64) { return false; }
    *pf = nsamp <= 6 * 64 ? 6 : (nsamp <= 10 * 64 ? 10 : 16);
    return (size_t)frontcm_layout(K, lgD).total * 4 <= (size_t)(160 * 1024 / 3);  // three blocks per CU
}

// ---- matrix-core FIR launches (vfo_toep_kernel): job construction, per-list planning (macro tiles per wavefront, grid, LDS), launch ----
ToepJob toep_job(const ToepTab& T, int var, StreamIn in, float* out, int base0, int nout, float inv_dev) {
    ToepJob j{};
    j.in = in;
    j.out = out;
    j.tl = T.d_tl;
    j.lbase = T.d_lb + (size_t)var * 64;
    j.tl_len = T.tl_len;
    j.nsteps = T.nsteps;
    j.s_in = T.s_in;
    j.rows = T.rows;
    j.base0 = base0;
    j.nout = nout;
    j.mt_per_wave = 1;
    j.inv_deviation = inv_dev;
    return j;
}

struct ToepPlan { int grid_x = 0; size_t lds = 0; };
ToepPlan toep_plan(std::vector<ToepJob>& jobs, int npl, int max_blocks = 2048) {
    ToepPlan P;
    if (jobs.empty()) { return P; }
    const int G = 2;
    int mtw = 1;
    // about two resident rounds (256 CUs x 4 blocks of four wavefronts, each job padded to whole blocks): alone the kernels do not
    // care (1 024 ... 8 192 blocks measured equal), but blocks that end let the FFT branch's blocks in — 2.5 % on the whole step
    for (; mtw < 16; mtw++) {
        size_t blocks = 0;
        for (auto& jb : jobs) { blocks += (size_t)((jb.nout + G * 16 * jb.rows - 1) / (G * 16 * jb.rows) + 4 * mtw - 1) / (size_t)(4 * mtw); }
        if (blocks <= (size_t)max_blocks) { break; }
    }
    for (auto& jb : jobs) {
        jb.mt_per_wave = mtw;
        const int nmt = (jb.nout + G * 16 * jb.rows - 1) / (G * 16 * jb.rows);
        P.grid_x = std::max(P.grid_x, (nmt + 4 * mtw - 1) / (4 * mtw));
        const int span = (G * 16 - 1) * jb.s_in + 4 * jb.nsteps, pl = (span + 8) & ~3;
        P.lds = std::max(P.lds, ((size_t)((jb.tl_len + 3) & ~3) + (size_t)4 * npl * pl) * sizeof(float));
    }
    return P;
}

void launch_toep(sdrpp_ctx* c, std::vector<ToepJob>& jobs, ToepJob* d_jobs, const ToepPlan& P, int width, bool quad) {
    if (jobs.empty() || P.grid_x == 0) { return; }
    const dim3 grid((unsigned)P.grid_x, (unsigned)jobs.size());
    if (quad) { launch(c, vfo_toep_kernel<1, 2, true>, grid, dim3(256), P.lds, (const ToepJob*)d_jobs); }
    else if (width == 2) { launch(c, vfo_toep_kernel<2, 2, false>, grid, dim3(256), P.lds, (const ToepJob*)d_jobs); }
    else { launch(c, vfo_toep_kernel<1, 2, false>, grid, dim3(256), P.lds, (const ToepJob*)d_jobs); }
}

// ---- pipelined FM back end (vfo_pipe_kernel) ----
constexpr int kPipeG = 1;    // groups of 16 tiles per macro tile: one keeps a job's LDS at ~30 KB, five workgroups per CU
constexpr int kPipeBpc = 5;     // workgroups per CU the kernel is built for (launch bounds; jobs of ~30 KB)
constexpr int kPipeBpcMin = 3;  // longer filters (NFM's 300-tap channel / audio filters: ~38 KB) run with fewer workgroups per CU
// LDS layout of one job; false = does not fit / stage 0 not register-staged -> the VFO keeps its separate launches
bool pipe_layout_try(PipeJob& J, int fifo_tiles, size_t* lds_bytes) {
    const int G = kPipeG;
    int off = 0;
    auto take = [&](int nfloats) { const int o = off; off += (nfloats + 3) & ~3; return o; };
    for (int s = 0; s < 4; s++) { J.tl_off[s] = take(J.st[s].tl_len); }
    int W[4], span[4], omt[4];
    for (int s = 0; s < 4; s++) {
        W[s] = G * 16 * J.st[s].s_in;
        span[s] = W[s] - J.st[s].s_in + 4 * J.st[s].nsteps;
        omt[s] = G * 16 * J.st[s].rows;
    }
    if (((span[0] + 1) >> 1) > (G == 1 ? 5 : 9) * 64) { return false; }  // stage 0's window is register-staged: five (G = 1) / nine sample pairs per lane
    J.win_off = take(2 * ((span[0] + 8) & ~3));
    J.zero_lo = off;
    for (int i = 0; i < 3; i++) {
        // R >= W + h + what the producer writes at a time, a multiple of W: windows start at multiples of W, no stall cycle.  (i = 2:
        // stage 3's own ring of discriminator outputs, which it fills a stage-2 macro tile at a time between two matrix loops.)
        const int s = i + 1, h = span[s] - W[s];
        if (h < 0) { return false; }
        const int R = std::max(2, (W[s] + h + omt[i] + W[s] - 1) / W[s]) * W[s];
        if (i < 2) {
            J.ring_len[i] = R;
            J.ring_mir[i] = h;
            J.ring_off[i] = take(2 * (R + h));
        }
        else {
            J.dring_len = R;
            J.dring_mir = h;
            J.dring_off = take(R + h);
        }
    }
    J.ring_len[2] = fifo_tiles * omt[2];  // IF phases on their way to the discriminator's difference: a plain FIFO of whole stage-2 macro tiles
    J.ring_mir[2] = 0;
    J.ring_off[2] = take(J.ring_len[2]);
    J.zero_hi = off;
    J.flag_off = take(8);
    *lds_bytes = (size_t)off * sizeof(float);
    return *lds_bytes <= (size_t)(160 * 1024) / kPipeBpcMin;
}
bool pipe_layout(PipeJob& J, size_t* lds_bytes) { return pipe_layout_try(J, 2, lds_bytes) || pipe_layout_try(J, 1, lds_bytes); }
// Segments per VFO, 0 = this push is better served by the separate launches.  A segment pays one warm-up macro tile per stage and the
// pipeline's fill: with fewer than ~12 last-stage macro tiles per segment of a full grid the four launches win (measured: 1 M-sample
// pushes of the 32-VFO bank, 2.6 tiles per segment, 14 % slower) — unless the push is so small that it is launch-bound anyway.
int pipe_segments(const std::vector<PipeJob>& pipes, int forced, size_t lds) {
    if (pipes.empty()) { return 0; }
    const int bpc = std::max(kPipeBpcMin, std::min(kPipeBpc, (int)((size_t)(160 * 1024) / std::max<size_t>(lds, 1))));
    int max_nmt = 1;
    for (auto& pj : pipes) { max_nmt = std::max(max_nmt, (pj.st[3].nout + kPipeG * 16 * pj.st[3].rows - 1) / (kPipeG * 16 * pj.st[3].rows)); }
    if (forced >= 2) { return std::min(forced, max_nmt); }
    const int s_full = (256 * bpc + (int)pipes.size() - 1) / (int)pipes.size();
    if (max_nmt >= 12 * s_full) { return s_full; }
    if (max_nmt <= 16) { return std::max(1, (max_nmt + 1) / 2); }  // two macro tiles per workgroup: the chain of hand-offs is what a small push waits for (B = 50 000: 53 us per push with one segment, 48.5 with three)
    return 0;
}

// ---- levels: the position of a launch in the data flow of one block ---------------------------------------------------------------------
constexpr int kLevels = 28;
template <class T>
struct Lev {
    std::vector<T> at[kLevels];
    T* dev[kLevels] = {};
    int top = 0;  // highest level in use + 1
    void add(int l, const T& j) {
        if (l >= kLevels) { l = kLevels - 1; }
        at[l].push_back(j);
        if (l + 1 > top) { top = l + 1; }
    }
};
template <class T>
bool arena_push_lev(sdrpp_ctx* c, Lev<T>& L) {
    for (int l = 0; l < L.top; l++) {
        if (L.at[l].empty()) { continue; }
        L.dev[l] = arena_push(c, L.at[l]);
        if (!L.dev[l]) { return false; }
    }
    return true;
}
// the job tables of a block do not fit the arena (arena_push returned null for a list that has jobs)
int arena_fail(sdrpp_ctx* c) { return fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }

// One block of the VFO bank, planned in steps: every VFO's chain is walked once (chain: a sequence of named parts — front_end, pipe_decide, the
// stage steps decim_step / poly_step / fir_step, if_chain, demod_fm / demod_am / demod_ssb, af_chain, phase_advance, history_carries — with
// outputs per stage from the integer streaming state and one job per stage in the list of its kind and LEVEL; a ChainCursor does every
// hand-over from one stream to the next), the first stages are grouped into front-end jobs (group_front), the job tables go into the arena in
// one piece (upload), then the launches — or, in pipelined mode, the roles — are emitted level by level (emit_front, emit_levels).  Every job
// carries the LEVEL of its launch in the block's data flow (level L reads what level L - 1 wrote): the front end is level 1 (level 0 = the
// block's arrival), every filter behind it one more.  A pass launches level by level; in pipelined mode level L of this block runs L ticks
// from now (tick_kernels.h).  Every Lev<> job list is named once, in for_each_list.
// One BankPlan lives with its context and is re-used block after block (begin() empties the lists and keeps their storage: with 128 VFOs a
// fresh plan per block was ~1 000 small allocations, a third of the 225 us of host time that had become cfg 4's limit once its tick took 135 us).
struct BankPlan {
    sdrpp_ctx* c;
    IqSrc src{};
    int n_in = 0;
    bool ticking = false;  // this block is planned for the tick queue (c->tick_planning when begin() ran; it does not change during a plan)
    int L0 = 0;  // levels the pre-processing chain takes in front (pipelined mode): the front end runs at level L0 + 1
    static constexpr int carry_last = kLevels - 1;
    static constexpr int carry_wave_max = 8192;  // floats: up to four rounds of a wavefront
    const std::vector<int>& fb;  // reference-block ends of this push (at least one entry: n_in)
    bool blocks = false;
    std::vector<S1Member> s1;
    std::vector<RotJob> rot;
    Lev<FirBJob> f_dec;  // register-blocked decimators (tap counts the matrix form does not cover; stage 0 only in reference-rotator mode)
    std::vector<RotXJob> rotx;                          // reference-rotator mode: full-rate float recursion, one lane per VFO
    std::vector<RetuneJob> retune;                      // closed-form NCO: first outputs after a setOffset
    Lev<PolyJob> poly;
    Lev<PolyBJob> polyb[4];  // [0]: LMAX 4, [1]: LMAX 8 (de-interleaved tile); [2], [3]: same with odd decimation (linear tile)
    Lev<FirBJob> chan;
    Lev<SeqJob> seq;
    // The wavefront-job role (TR_IFC, vfo_ifchain_kernels.h).  The chain walk fills one record list per kind; upload files every record under the role once it
    // has its address in the arena (file_wave): `wave` is the table the role reads, a level's jobs of every kind in one launch.
    Lev<WaveJob> wave;
    size_t wave_lds = 0;    // ... and the LDS its launches need (none unless a kind that uses it is filed: wave_kind_uses_lds)
    // radio IF chain (if_chain), between the channel filter's level and the demodulator's, for the VFOs that carry one: a blanker / squelch record and / or an FMIF record per VFO
    Lev<NbSqJob> nbsq;
    Lev<FmifJob> fmif;
    Lev<PreJob> pre;
    Lev<FirBJob> audio;     // AM: real stream -> low-pass -> stereo
    Lev<FirBJob> audio_fm;  // WFM/NFM: IF -> discriminator -> low-pass -> stereo, one kernel
    // the same work on the matrix cores (vfo_toep_kernel) whenever the VFO has a tap table for it
    Lev<ToepJob> t_dec, t_poly, t_chan, t_audio, t_audio_fm;
    std::vector<PipeJob> pipes;  // FM back ends that run as one pipelined launch (ordinary passes only)
    size_t pipe_lds = 0;
    PipeJob* d_pipes = nullptr;
    int pipe_seg = 0;  // segments per VFO of that launch
    int pipe_lvl = 0;  // its level: the latest at which any of its jobs starts (levels only order the launches of a pass)
    // radio AF chain (stereo frames have the layout of complex samples, so the same kernels serve)
    Lev<ToepJob> t_af_dec, t_af_poly, t_af_hpf;
    Lev<FirBJob> af_dec, af_hpf;
    Lev<PolyJob> af_poly;
    Lev<DeempJob> af_deemp;
    Lev<SsbRotXJob> ssbx_l;
    // RDS branch of the WFM demodulator (rds_branch): the fused first stage's records / the reference rotator's / the line splice's; the later stages go into
    // the AF chain's lists — complex_t and stereo_t are the same arithmetic there
    Lev<RdsJob> rdsj;
    Lev<RdsRotXJob> rdsx;
    Lev<RdsLineJob> rdsl;
    // stereo branch of the WFM demodulator (stereo_branch): its three kinds — the loop's per-VFO records SDRPP_ST_PACK to a job
    Lev<StereoPilotJob> stp;
    Lev<StereoLoopVfo> stl;
    Lev<StereoLoopJob> stlj;  // (filled by upload once stl's records have their addresses)
    Lev<StereoMatrixJob> stm;
    // symbol branch of a RAW VFO (sym_branch): the front's records, the loop's per-VFO records up to SDRPP_SYM_PACK to a job
    Lev<SymFrontJob> syf;
    Lev<SymLoopVfo> syl;
    Lev<SymLoopJob> sylj;  // (filled by upload once syl's records have their addresses)
    // RDS demodulator (rdsd_branch): a record, and a job, per VFO
    Lev<RdsdJob> rdsdj;
    // QPSK demodulator (qpsk_branch): a front record (file_wave cuts it into segment jobs) and a loop record per VFO
    Lev<QpskFrontJob> qpf;
    Lev<QpskLoopJob> qpl;
    // framer behind the symbol branch (frame_branch): a record, and a job, per VFO
    Lev<FrameJob> frj;
    Lev<CarryJob> carry;  // history carries at the level of the stream's consumer (a pass without pipelining: all at the last level)
    int max_rot = 0;
    // front-end jobs (group_front)
    struct S1Launch { int vt; std::vector<Stage1Job> jobs; int max_nout = 0; int tile = 256; size_t lds = 0; };
    struct F2Launch { int vt; std::vector<Front2Job> jobs; int max_blocks = 0; size_t lds = 0; };
    struct FCMLaunch { std::vector<FrontCMJob> jobs; int max_blocks = 0; size_t lds = 0; };
    S1Launch s1l[4];
    F2Launch f2l[4];
    FCMLaunch fcm[3];  // PF 6 / 10 / 16
    FCMLaunch fcl;     // long first stages (vfo_frontcl_kernel)
    int fcl_nw = 2;    // tile engines per workgroup of that launch: 4 as a role of a tick when four wavefronts' planes fit half a CU's LDS, 1 where two engines' exceed a workgroup's
    const int vts[4] = { 8, 4, 2, 1 };
    // device addresses of the job tables (upload)
    Stage1Job* d_s1[4] = {};
    Front2Job* d_f2[4] = {};
    FrontCMJob* d_fcl = nullptr;
    FrontCMJob* d_fcm[3] = {};
    RotXJob* d_rotx = nullptr;
    RotXHead* d_rotx_head = nullptr;  // pipelined: what the TR_ROTX16 role finds behind its job pointer
    RetuneJob* d_retune = nullptr;
    RotJob* d_rot = nullptr;
    const int* d_fb = nullptr;
    struct ToepList { Lev<ToepJob>* L; int npl, width; bool quad; int fam; int role; };
    static constexpr int kToepLists = 8;
    ToepList tlists[kToepLists] = { { &t_dec, 2, 2, false, F_DECIM, TR_TOEP_C },      { &t_poly, 2, 2, false, F_POLY, TR_TOEP_C },       { &t_chan, 2, 2, false, F_FIR, TR_TOEP_C },
                                    { &t_audio, 1, 1, false, F_FIR, TR_TOEP_R },      { &t_audio_fm, 2, 1, true, F_FIR, TR_TOEP_Q },     { &t_af_dec, 2, 2, false, F_AF, TR_TOEP_C },
                                    { &t_af_poly, 2, 2, false, F_AF, TR_TOEP_C },     { &t_af_hpf, 2, 2, false, F_AF, TR_TOEP_C } };
    ToepPlan tplan[kToepLists][kLevels];

    // THE enumeration of the Lev<> job lists, in the order their tables lie in the arena (the matrix-core lists of tlists[] first), for begin(),
    // upload() and emit_levels().  A new list is one more f(...) here (a matrix-core list: one more row of tlists[]; a record list of the wavefront-job
    // role: one more file_wave line in upload as well).  The last three are not filled by the chain walk: upload derives them from lists in front of them
    // once those have their addresses in the arena (stlj from stl, sylj from syl, wave from every record list of the role), and pushes them itself.
    template <class F>
    void for_each_list(F&& f) {
        for (auto& t : tlists) { f(*t.L); }
        f(f_dec); f(poly);
        for (auto& q : polyb) { f(q); }
        f(chan); f(seq); f(nbsq); f(fmif); f(rdsj); f(rdsx); f(rdsl); f(stp); f(stl); f(stm); f(syf); f(syl); f(rdsdj); f(qpf); f(qpl); f(frj); f(pre); f(audio); f(audio_fm);
        f(af_dec); f(af_hpf); f(af_poly); f(af_deemp);
        f(ssbx_l); f(carry);
        f(stlj); f(sylj); f(wave);
    }

    explicit BankPlan(sdrpp_ctx* c_) : c(c_), fb(c_->vfo_bounds) {
        for (int i = 0; i < 4; i++) { s1l[i].vt = vts[i]; f2l[i].vt = vts[i]; }
    }
    template <class T>
    static void lev_reset(Lev<T>& L) {
        for (int l = 0; l < L.top; l++) {
            L.at[l].clear();
            L.dev[l] = nullptr;
        }
        L.top = 0;
    }
    // a new block: every list empty (storage kept), every per-block scalar back to its initial value
    void begin(const IqSrc& src_, int64_t count, const CarryJob& iq_carry) {
        src = src_;
        n_in = (int)count;
        ticking = c->tick_planning;
        L0 = ticking ? c->plan_lvl0 : 0;
        blocks = fb.size() > 1;
        s1.clear(); rot.clear(); rotx.clear(); retune.clear(); pipes.clear();
        for_each_list([](auto& L) { lev_reset(L); });
        pipe_lds = 0;
        wave_lds = 0;
        d_pipes = nullptr;
        pipe_seg = 0;
        pipe_lvl = 0;
        max_rot = 0;
        fcl_nw = 2;
        for (int i = 0; i < 4; i++) {
            s1l[i].jobs.clear(); s1l[i].max_nout = 0; s1l[i].tile = 256; s1l[i].lds = 0;
            f2l[i].jobs.clear(); f2l[i].max_blocks = 0; f2l[i].lds = 0;
            d_s1[i] = nullptr;
            d_f2[i] = nullptr;
        }
        for (int i = 0; i < 3; i++) {
            fcm[i].jobs.clear(); fcm[i].max_blocks = 0; fcm[i].lds = 0;
            d_fcm[i] = nullptr;
        }
        fcl.jobs.clear(); fcl.max_blocks = 0; fcl.lds = 0;
        d_fcl = nullptr; d_rotx = nullptr; d_retune = nullptr; d_rot = nullptr; d_fb = nullptr;
        for (auto& row : tplan) {
            for (auto& q : row) { q = ToepPlan{}; }
        }
        carry.add(ticking ? L0 + 1 : carry_last, iq_carry);  // job 0 of its level: the shared IQ stream
    }
    BankPlan(const BankPlan&) = delete;
    BankPlan& operator=(const BankPlan&) = delete;

    // ---- one VFO's chain: stage by stage, a job per stage in the list of its kind and level ----
    // Where the walk down a chain stands: the stream the next stage reads and the level at which that stream is written.
    struct ChainCursor {
        Stream* cur;
        int lvl;
        // The hand-over of a stage that runs `levels` levels behind the writer of `cur`: it is `cur`'s consumer (in pipelined mode the history
        // carry of `cur` runs at that level, history_carries) and writes n_out samples of `nxt`, which the next stage reads.
        void step(Stream& nxt, int n_out, int levels = 1) {
            lvl += levels;
            cur->clevel = lvl;
            nxt.n = n_out;
            nxt.wlevel = lvl;
            cur = &nxt;
        }
    };
    // What the parts of one chain() call share.
    struct ChainCtx {
        Vfo& v;
        ChainCursor at;
        bool ifc_on = false;    // the radio's IF chain runs for this VFO
        std::vector<int> bnd;   // reference-block ends, carried down to the demodulator's rate for the block-dependent operations there; empty where none runs
        const int* d_bnd = nullptr;  // their copy in the arena once that rate is reached
        int nbnd = 0;
        bool split = false;     // a launch group of several pushes (sdrpp_set_pipeline_group)
        std::vector<int>* tk;   // its PUSH ends, carried down to the stream the results are read from (tick_results_describe): v.tk_if, then v.tk_af; empty unless `split`
        S1Member mem{};
        int first_sep = 0;  // first decimator stage that runs as its own FIR launch
        double phi_end = 0.0;
        bool have_phi_end = false;  // (a launch group: the NCO phase after its last push, advanced push by push as block-by-block processing does)
        // the FM back end as one pipelined launch (pipe_decide): the stage steps collect their matrix-form jobs here instead of in the lists
        bool piped = false;
        PipeJob pj;  // INDETERMINATE unless `piped`: pipe_decide sets it up for a candidate only (clearing it for every VFO of every block is host time)
        size_t pj_lds = 0;
        ChainCtx(Vfo& v_, int lvl) : v(v_), at{ &v_.st[(size_t)v_.i_first], lvl }, tk(&v_.tk_if) {}
        ToepJob* pipe(int s) { return piped ? &pj.st[s] : nullptr; }
        void through_decim(int off, int D) { bounds_decim(bnd, off, D); bounds_decim(*tk, off, D); }  // (an empty list: nothing to do)
        void through_poly(int poff, int pphase, int L, int M) { bounds_poly(bnd, poff, pphase, L, M); bounds_poly(*tk, poff, pphase, L, M); }
    };

    // ---- one step per stage kind, for the VFO's chain and the AF chain alike: it advances the stage's `off` / `phase`.  `toep` is the list of the matrix form
    // (taken whenever the stage has a tap table), the other list that of the VALU form; with `pipe` set the matrix-form job goes there instead of into `toep`.
    // (Forced inline: as calls the three steps cost a 128-VFO bank 3 - 4 us of the 34 us its chains take per block, profiles/planner_split_host_time.md.) ----
    static void place(Lev<ToepJob>& toep, ToepJob* pipe, int l, const ToepJob& j) {
        if (pipe) { *pipe = j; }
        else { toep.add(l, j); }
    }
    __attribute__((always_inline)) void decim_step(ChainCtx& x, Stream& nxt, RateChain& R, int s, Lev<ToepJob>& toep, Lev<FirBJob>& firb, ToepJob* pipe = nullptr) {
        const Stream& in = *x.at.cur;
        const ToepTab& tp = R.tp_stage[s];
        const int K = R.ntaps(s), D = R.decim_s[s];
        int& off = R.pos.soff[s];
        const int l = x.at.lvl + 1;
        const int no = decim_nout(in.n, off, D);
        x.through_decim(off, D);
        if (tp.ok) { place(toep, pipe, l, toep_job(tp, 0, stream_in(in), nxt.data, off - (K - 1), no, 0.0f)); }
        else { firb.add(l, FirBJob{ stream_in(in), nxt.data, R.d_staps[s], K, ilog2(D), off, no, R.s_kp[s] }); }
        off = off + no * D - in.n;
        x.at.step(nxt, no);
    }
    // (`d_cyc`: the cycle tables of the register-blocked form, which the RxVFO's resampler alone has)
    __attribute__((always_inline)) void poly_step(ChainCtx& x, Stream& nxt, RateChain& R, const float* d_cyc, int cyc_rows, int cyc_lmax, Lev<ToepJob>& toep, Lev<PolyJob>& valu, ToepJob* pipe = nullptr) {
        const Stream& in = *x.at.cur;
        const ToepTab& tp = R.tp_poly;
        const int L = R.interp, M = R.decim, tpp = R.tpp;
        int &phase = R.pos.pphase, &off = R.pos.poff;
        const int l = x.at.lvl + 1;
        const int no = poly_nout(in.n, off, phase, L, M);
        x.through_poly(off, phase, L, M);
        if (tp.ok) { place(toep, pipe, l, toep_job(tp, phase, stream_in(in), nxt.data, off - (tpp - 1), no, 0.0f)); }
        else if (d_cyc) {
            polyb[(cyc_lmax == 4 ? 0 : 1) + ((M & 1) ? 2 : 0)].add(l, PolyBJob{ stream_in(in), (float2*)nxt.data, d_cyc + (size_t)phase * cyc_rows * cyc_lmax, L, M,
                                                                                      tpp, off, no, cyc_rows });
        }
        else { valu.add(l, PolyJob{ stream_in(in), (float2*)nxt.data, R.d_bank, L, M, tpp, phase, off, no }); }
        const long long A = (long long)phase + (long long)no * M;
        phase = (int)(A % L);
        off = off + (int)(A / L) - in.n;
        x.at.step(nxt, no);
    }
    __attribute__((always_inline)) void fir_step(ChainCtx& x, Stream& nxt, const ToepTab& tp, const float* d_taps, int K, int kp, float inv_dev, Lev<ToepJob>& toep, Lev<FirBJob>& firb, ToepJob* pipe = nullptr) {
        const Stream& in = *x.at.cur;
        const int l = x.at.lvl + 1;
        if (tp.ok) { place(toep, pipe, l, toep_job(tp, 0, stream_in(in), nxt.data, -(K - 1), in.n, inv_dev)); }
        else { firb.add(l, FirBJob{ stream_in(in), nxt.data, d_taps, K, 0, 0, in.n, kp, inv_dev }); }
        x.at.step(nxt, in.n);
    }

    int chain(Vfo& v) {
        ChainCtx x(v, L0 + 1);
        for_each_stream(v, [](Stream& s) { s.clevel = 0; s.wlevel = 0; });
        x.at.cur->wlevel = x.at.lvl;
        const bool agc_mode = v.d.demod == SDRPP_DEMOD_AM || (v.d.demod >= SDRPP_DEMOD_USB && v.d.demod <= SDRPP_DEMOD_CW);
        x.ifc_on = v.ifc.active() && v.i_ifc >= 0 && v.st[(size_t)v.i_ifc].base;
        const bool need_bnd = (agc_mode && (blocks || v.nco_exact)) || (x.ifc_on && v.ifc.sq_on && blocks) || (v.rds.on && v.rds.exact && blocks);
        if (need_bnd) { x.bnd = fb; }
        x.split = c->grp_ends.size() > 1;
        v.tk_if.clear();
        v.tk_af.clear();
        if (x.split) { v.tk_if = c->grp_ends; }
        front_end(x);
        pipe_decide(x);
        const int last_dec = v.rate.n_stages - 1;
        for (int s = x.first_sep; s < v.rate.n_stages; s++) {
            Stream& nxt = v.st[(size_t)v.i_first + s];
            const bool to_pipe = x.piped && s == last_dec;
            decim_step(x, nxt, v.rate, s, t_dec, f_dec, to_pipe ? x.pipe(0) : nullptr);
            if (to_pipe) {
                x.pj.keep[0] = std::max(0, nxt.n - nxt.hist_len);
                x.pj.dec_stage = s;
                x.pj.lvl = x.at.lvl;
            }
        }
        if (v.i_poly >= 0) {
            Stream& nxt = v.st[(size_t)v.i_poly];
            poly_step(x, nxt, v.rate, v.d_cyc, v.cyc_rows, v.cyc_lmax, t_poly, poly, x.pipe(1));
            if (x.piped) { x.pj.keep[1] = std::max(0, nxt.n - nxt.hist_len); }
        }
        if (v.i_chan >= 0 && v.chan_ntaps > 0) {
            fir_step(x, v.st[(size_t)v.i_chan], v.tp_chan, v.d_chan, v.chan_ntaps, v.chan_kp, 0.0f, t_chan, chan, x.pipe(2));
            if (x.piped) { x.pj.keep[2] = 0; }  // the IF stream is the RxVFO's output: all of it
        }
        v.i_if = (int)(x.at.cur - &v.st[0]);
        v.lvl_if = x.at.lvl;
        v.lvl_out = x.at.lvl;
        if (need_bnd) {
            x.d_bnd = arena_push(c, x.bnd);
            if (!x.d_bnd) { return arena_fail(c); }
            x.nbnd = (int)x.bnd.size();
        }
        if_chain(x);
        const ChainCursor feed = x.at;  // the stream the demodulator reads
        v.stereo.ran = v.stereo.on;
        if (v.stereo.on) { stereo_branch(x); }  // (WFM only: stereo_apply)
        else if (v.d.demod == SDRPP_DEMOD_WFM || v.d.demod == SDRPP_DEMOD_NFM) { demod_fm(x); }
        else if (v.d.demod == SDRPP_DEMOD_AM) { demod_am(x); }
        else if (v.d.demod >= SDRPP_DEMOD_USB && v.d.demod <= SDRPP_DEMOD_CW) { demod_ssb(x); }
        if (v.af.on && v.i_out >= 0) { af_chain(x); }
        int last_lvl = x.at.lvl;
        v.rds.ran = v.rds.on;
        if (v.rds.on) {
            rds_branch(x, feed);
            last_lvl = std::max(last_lvl, x.at.lvl);
        }
        else {
            for (auto& s : v.rds.st) { s.n = 0; }
        }
        v.sym.ran = v.sym.attached && v.sym.on;
        if (v.sym.ran) {
            if (int rc = sym_branch(x, feed)) { return rc; }
            last_lvl = std::max(last_lvl, v.sym.lvl);
        }
        else {
            for (auto& s : v.sym.st) { s.n = 0; }
        }
        v.frame.ran = v.frame.attached && v.frame.on && v.sym.ran;
        if (v.frame.ran) {
            frame_branch(x);
            last_lvl = std::max(last_lvl, v.frame.lvl);
        }
        else {
            for (auto& s : v.frame.st) { s.n = 0; }
        }
        v.rdsd.ran = v.rdsd.attached && v.rdsd.on && (v.rdsd.source == 1 || v.rds.ran);
        if (v.rdsd.ran) {
            if (int rc = rdsd_branch(x, feed)) { return rc; }
            last_lvl = std::max(last_lvl, v.rdsd.lvl);
        }
        else {
            for (auto& s : v.rdsd.st) { s.n = 0; }
        }
        v.qpsk.ran = v.qpsk.attached && v.qpsk.on;
        if (v.qpsk.ran) {
            if (int rc = qpsk_branch(x, feed)) { return rc; }
            last_lvl = std::max(last_lvl, v.qpsk.lvl);
        }
        else {
            for (auto& s : v.qpsk.st) { s.n = 0; }
        }
        phase_advance(x);
        x.at.lvl = last_lvl;
        history_carries(x);
        c->plan_top = std::max(c->plan_top, x.at.lvl + 2);
        return SDRPP_OK;
    }

    // The front end of one VFO: its membership of a front-end job (group_front builds the jobs), or the translation alone.  Leaves the cursor on
    // the first stream a separate stage reads.
    void front_end(ChainCtx& x) {
        Vfo& v = x.v;
        Stream* cur = x.at.cur;
        if (v.nco_exact) {
            // the reference's own data flow: rotate at the full rate (float recursion), then every stage of the plan as a plain FIR
            Stream* tgt = (v.rate.n_stages == 0) ? cur : &v.st[(size_t)v.i_rot];
            rotx.push_back(RotXJob{ (float2*)tgt->data, v.d_rot, v.d.phase_delta_re, v.d.phase_delta_im });
            tgt->n = n_in;
            tgt->wlevel = x.at.lvl;
            x.at.cur = tgt;
            return;
        }
        if (v.rate.n_stages == 0) {
            rot.push_back(RotJob{ v.theta, v.phi, (float2*)cur->data, n_in });
            cur->n = n_in;
            max_rot = std::max(max_rot, n_in);
            return;
        }
        int* so = v.rate.pos.soff;
        const int D = v.rate.decim_s[0];
        const int nout = decim_nout(n_in, so[0], D);
        if (v.modtaps_dirty) { build_modtaps(v); }
        const int K0 = v.rate.ntaps(0);
        S1Member& mem = x.mem;
        mem = S1Member{ &v, K0, ilog2(D), so[0], nout, v.phi, 0, 0, 0, 0, 0, 0, v.tap_hash };
        int need = K0 - 1;
        x.first_sep = 1;
        x.through_decim(so[0], D);
        if (v.fused_front) {
            const int D2 = v.rate.decim_s[1];
            mem.fused = 1;
            mem.K2 = v.rate.ntaps(1);
            mem.lgD2 = ilog2(D2);
            mem.off2 = so[1];
            mem.nout2 = decim_nout(nout, so[1], D2);
            need = K0 - 1 + D * (mem.K2 - 1);
            x.first_sep = 2;
            x.through_decim(so[1], D2);
        }
        mem.min_idx = (v.seen >= need) ? -need : -(int)v.seen;  // older samples predate this VFO: zero
        if (!x.split) { s1.push_back(mem); }
        else { front_split(x, need); }
        retune_job(x);
        so[0] = so[0] + nout * D - n_in;
        cur->n = nout;
        if (mem.fused) {
            Stream* nxt = &v.st[(size_t)v.i_first + 1];
            so[1] = so[1] + mem.nout2 * v.rate.decim_s[1] - nout;
            cur->n = 0;  // the stage-1 stream is never materialised
            nxt->n = mem.nout2;
            nxt->wlevel = x.at.lvl;
            x.at.cur = nxt;
        }
    }
    // A launch group: ONE front-end job per push, with the offsets, the NCO phase and the history bound block-by-block processing would
    // have given that push (the closed-form NCO is anchored at the start of a job: tile phasor x in-tile table — one job over the whole
    // group would round the same samples differently), reading its samples where they lie in the group's block and writing its outputs
    // behind those of the pushes in front.  Everything behind the front end is a plain FIR over the stream, indifferent to the cuts.
    void front_split(ChainCtx& x, int need) {
        Vfo& v = x.v;
        const S1Member& mem = x.mem;
        const int D = v.rate.decim_s[0];
        int so0 = v.rate.pos.soff[0], so1 = v.rate.pos.soff[1], prev_e = 0, oshift = 0;
        long long seen = v.seen;
        double ph = v.phi;
        for (size_t j = 0; j < c->grp_ends.size(); j++) {
            const int nj = c->grp_ends[j] - prev_e;
            S1Member m = mem;
            m.off0 = so0;
            m.nout = decim_nout(nj, so0, D);
            m.phi0 = ph;
            int outs = m.nout;
            if (mem.fused) {
                m.off2 = so1;
                m.nout2 = decim_nout(m.nout, so1, v.rate.decim_s[1]);
                outs = m.nout2;
            }
            m.min_idx = ((seen >= need) ? -need : -(int)seen) + prev_e;
            m.shift = prev_e;
            m.oshift = oshift;
            if (outs > 0) { s1.push_back(m); }
            so0 = so0 + m.nout * D - nj;
            if (mem.fused) { so1 = so1 + m.nout2 * v.rate.decim_s[1] - m.nout; }
            const double pj = ph + (double)nj * v.theta;
            ph = pj - std::floor(pj);
            seen += nj;
            oshift += outs;
            prev_e = c->grp_ends[j];
        }
        x.phi_end = ph;
        x.have_phi_end = true;
    }
    // setOffset hand-over: outputs whose window still reaches in front of the latest retune point are recomputed with the
    // piecewise phase (vfo_retune_fix_kernel); retune points no window can reach any more are forgotten
    void retune_job(ChainCtx& x) {
        Vfo& v = x.v;
        const S1Member& mem = x.mem;
        const int D1 = v.rate.decim_s[0], K0 = mem.K, Kc = v.h12_K;
        const int off = mem.fused ? mem.off0 + (mem.off2 - (mem.K2 - 1)) * D1 - (K0 - 1) : mem.off0 - (K0 - 1);
        const int nout_f = mem.fused ? mem.nout2 : mem.nout;
        while (!v.recs.empty() && v.recs.front().pos - v.seen <= (long long)off) { v.recs.erase(v.recs.begin()); }
        while (v.recs.size() > SDRPP_RETUNE_MAX_SEG - 1) { v.recs.erase(v.recs.begin()); }
        if (v.recs.empty() || nout_f <= 0) { return; }
        const long long r_last = v.recs.back().pos - v.seen;  // push-relative, <= 0
        const long long Dc = 1ll << v.h12_lgD;
        const int nfix = (int)std::min<long long>((long long)nout_f, (r_last - off + Dc - 1) / Dc);  // outputs m with off + m * Dc < r_last
        if (nfix <= 0) { return; }
        RetuneJob rj{};
        rj.out = (float2*)v.st[(size_t)v.i_first + (mem.fused ? 1 : 0)].data;
        rj.taps = v.d_h12;
        rj.K = Kc;
        rj.log2_decim = v.h12_lgD;
        rj.off = off;
        rj.nfix = nfix;
        rj.min_idx = mem.min_idx;
        const int nr = (int)v.recs.size();
        rj.nseg = nr + 1;
        // segment q >= 1 starts at retune point q - 1 and runs with the increment that was in effect from there on (the
        // newest with the current one); segment 0 = everything in front of the oldest remembered point, anchored there.
        // Phases are continuous across the points, evaluated backwards from the current phase.
        double P = v.phi + v.theta * (double)r_last;  // phase at the newest point
        for (int q = nr; q >= 1; q--) {
            const long long Sq = v.recs[(size_t)q - 1].pos - v.seen;
            rj.start[q] = (int)std::max<long long>(Sq, -2000000000ll);
            rj.theta[q] = (q == nr) ? v.theta : v.recs[(size_t)q].theta_before;
            rj.phi[q] = P - std::floor(P);
            if (q >= 2) {  // phase at the start of the segment in front: back along ITS increment
                const long long Sp = v.recs[(size_t)q - 2].pos - v.seen;
                P = P + v.recs[(size_t)q - 1].theta_before * (double)(Sp - Sq);
            }
        }
        rj.start[0] = rj.start[1];
        rj.theta[0] = v.recs[0].theta_before;
        rj.phi[0] = rj.phi[1];
        retune.push_back(rj);
    }
    // the FM back end as one pipelined launch (ordinary passes): last decimator, resampler, channel filter, discriminator + audio low-pass all
    // in their matrix form, and the pipeline's LDS layout fits
    void pipe_decide(ChainCtx& x) {
        Vfo& v = x.v;
        const int last_dec = v.rate.n_stages - 1;
        x.piped = c->pipe_on && !ticking && !x.ifc_on && !v.stereo.on && (v.d.demod == SDRPP_DEMOD_WFM || v.d.demod == SDRPP_DEMOD_NFM) && last_dec >= x.first_sep && v.rate.tp_stage[last_dec].ok &&
                  v.i_poly >= 0 && v.rate.tp_poly.ok && v.i_chan >= 0 && v.chan_ntaps > 0 && v.tp_chan.ok && v.tp_audio.ok;
        if (!x.piped) { return; }
        x.pj = PipeJob{};
        const ToepTab* tabs[4] = { &v.rate.tp_stage[last_dec], &v.rate.tp_poly, &v.tp_chan, &v.tp_audio };
        for (int s = 0; s < 4; s++) { x.pj.st[s] = toep_job(*tabs[s], 0, StreamIn{}, nullptr, 0, 0, 0.0f); }  // (the layout needs the tables' geometry only)
        x.pj.timeouts = c->hd_tick_flag ? (int*)(c->hd_tick_flag + 8) : nullptr;
        x.piped = pipe_layout(x.pj, &x.pj_lds);
    }
    // the radio's IF chain: a level of its own per part (blanker / squelch, then FMIF) between the IF stream (which stays RxVFO::out) and whatever
    // follows — the demodulator's levels below move down by as many for this VFO, and read the chain's buffer in place of the IF
    void if_chain(ChainCtx& x) {
        Vfo& v = x.v;
        if (v.i_fmi >= 0) { v.st[(size_t)v.i_fmi].n = 0; }
        if (!x.ifc_on) {
            if (v.i_ifc >= 0) { v.st[(size_t)v.i_ifc].n = 0; }
            return;
        }
        Stream& fs = v.st[(size_t)v.i_ifc];
        const bool fm = v.ifc.fm_on;
        if (v.ifc.nbsq()) {
            const Stream& in = *x.at.cur;
            Stream& to = fm ? v.st[(size_t)v.i_fmi] : fs;  // in front of FMIF: the stream whose history is FMIF's delay line
            const bool per_block = v.ifc.sq_on && blocks;
            nbsq.add(x.at.lvl + 1, NbSqJob{ (const float2*)in.data, (float2*)to.data, v.ifc.d_amp, in.n, v.ifc.nb_on, v.ifc.nb_rate, 1.0f - v.ifc.nb_rate, v.ifc.nb_level, v.ifc.sq_on, v.ifc.sq_level,
                                            per_block ? x.d_bnd : nullptr, per_block ? x.nbnd : 0 });
            x.at.step(to, in.n);
        }
        if (fm) {
            // FMIF: one level behind the blanker / squelch job (a closed block is zeroed only at that job's end); file_wave cuts the record into a job
            // per segment of kFmifSeg samples — parallel over samples, the stream's history in front of the first
            const Stream& in = *x.at.cur;
            fmif.add(x.at.lvl + 1, FmifJob{ (const float2*)in.data, (float2*)fs.data, in.n, v.ifc.fm_bins, in.hist[in.cur], in.hist_len, c->fmif_tabs[v.ifc.fm_bins] });
            x.at.step(fs, in.n);
        }
        v.lvl_ifc = x.at.lvl;
        v.lvl_out = x.at.lvl;
    }
    void demod_fm(ChainCtx& x) {
        Vfo& v = x.v;
        fir_step(x, v.st[(size_t)v.i_out], v.tp_audio, v.d_audio, v.audio_ntaps, v.audio_kp, v.d.inv_deviation, t_audio_fm, audio_fm, x.pipe(3));
        if (x.piped) {
            pipes.push_back(x.pj);
            pipe_lds = std::max(pipe_lds, x.pj_lds);
        }
        v.lvl_out = x.at.lvl;
    }
    // Stereo branch of the WFM demodulator (broadcast_fm.h:147-191) in place of the audio low-pass job: pilot (discriminator, pilot filter, angle), loop (the
    // PLL's recursion), matrix (phasor, L-R, the two audio low-passes), a level each, off the stream the demodulator reads.  Pilot and matrix: a job per run of
    // SDRPP_ST_SEG samples; loop: a record per VFO (upload packs them into jobs).  Nothing here depends on where a block or a push ends: a launch group is one block.
    void stereo_branch(ChainCtx& x) {
        Vfo& v = x.v;
        Vfo::Stereo& s = v.stereo;
        const Stream& in = *x.at.cur;
        const int n = in.n, lvl = x.at.lvl;
        Stream &sm = s.st[0], &sa = s.st[1], &sp = s.st[2], &out = v.st[(size_t)v.i_out];
        const StreamIn sin = stream_in(in);
        for (int lo = 0; lo < n; lo += SDRPP_ST_SEG) {
            stp.add(lvl + 1, StereoPilotJob{ sin, sm.data, sa.data, s.d_ptaps, s.K, lo, std::min(lo + SDRPP_ST_SEG, n), v.d.inv_deviation });
        }
        x.at.step(sm, n);
        sa.n = n;
        sa.wlevel = lvl + 1;
        sa.clevel = lvl + 2;
        if (n > 0) { stl.add(lvl + 2, StereoLoopVfo{ sa.data, sp.data, s.d_state, s.alpha, s.beta, s.min_freq, s.max_freq, n }); }
        sp.n = n;
        sp.wlevel = lvl + 2;
        sp.clevel = lvl + 3;
        StreamIn min_ = stream_in(sm), pin = stream_in(sp);
        for (int lo = 0; lo < n; lo += SDRPP_ST_SEG) {
            stm.add(lvl + 3, StereoMatrixJob{ min_, pin, reinterpret_cast<float2*>(out.data), v.d_audio, v.audio_ntaps, s.delay, lo, std::min(lo + SDRPP_ST_SEG, n) });
        }
        x.at.step(out, n, 2);
        v.lvl_out = x.at.lvl;
    }
    // envelope (one level), AGC / DC loop (the next), then the audio filter on the real stream `dem`: the IF stream's consumers have no memory
    void demod_am(ChainCtx& x) {
        Vfo& v = x.v;
        const Stream& in = *x.at.cur;
        const int nif = in.n, lvl = x.at.lvl;
        Stream& dem = v.st[(size_t)v.i_dem];
        AgcState* agc = (AgcState*)v.d_state;
        float* dc = (float*)(v.d_state + 2 * sizeof(AgcState));
        if (!v.d.am_carrier_agc) { pre.add(lvl + 1, PreJob{ 2, nif, (const float2*)in.data, dem.data, 0.0, 0.0 }); }
        seq.add(lvl + 2, SeqJob{ 2, nif, (const float2*)in.data, dem.data, nullptr, agc, agc + 1, dc, v.d.dc_block_rate, v.d.am_carrier_agc, x.d_bnd, x.nbnd });
        dem.n = nif;
        dem.wlevel = lvl + 2;
        x.at = ChainCursor{ &dem, lvl + 2 };
        fir_step(x, v.st[(size_t)v.i_out], v.tp_audio, v.d_audio, v.audio_ntaps, v.audio_kp, 0.0f, t_audio, audio);
        v.lvl_out = x.at.lvl;
    }
    // second translation (one level), AGC loop straight into the stereo output (the next); `dem` is scratch, no stream of the chain
    void demod_ssb(ChainCtx& x) {
        Vfo& v = x.v;
        const Stream& in = *x.at.cur;
        const int nif = in.n, lvl = x.at.lvl;
        Stream& dem = v.st[(size_t)v.i_dem];
        Stream& out = v.st[(size_t)v.i_out];
        AgcState* agc = (AgcState*)v.d_state;
        float* dc = (float*)(v.d_state + 2 * sizeof(AgcState));
        if (v.nco_exact) { ssbx_l.add(lvl + 1, SsbRotXJob{ (const float2*)in.data, dem.data, v.d_rot + 1, v.d.ssb_phase_delta_re, v.d.ssb_phase_delta_im, x.d_bnd, x.nbnd }); }
        else if (x.split) {  // a launch group: the second translation anchored push by push, like the first (its phase advances as block-by-block processing advances it)
            int lo = 0;
            for (size_t j = 0; j < v.tk_if.size(); j++) {
                const int nj = v.tk_if[j] - lo;
                if (nj > 0) { pre.add(lvl + 1, PreJob{ v.d.demod, nj, (const float2*)in.data + lo, dem.data + (size_t)lo * (size_t)dem.width, v.theta2, v.phi2 }); }
                const double q2 = v.phi2 + (double)nj * v.theta2;
                v.phi2 = q2 - std::floor(q2);
                lo = v.tk_if[j];
            }
        }
        else { pre.add(lvl + 1, PreJob{ v.d.demod, nif, (const float2*)in.data, dem.data, v.theta2, v.phi2 }); }
        seq.add(lvl + 2, SeqJob{ v.d.demod, nif, (const float2*)in.data, dem.data, out.data, agc, agc + 1, dc, 0.0f, 0, x.d_bnd, x.nbnd });
        x.at.lvl += 2;
        dem.n = 0;  // scratch only
        out.n = nif;
        out.wlevel = x.at.lvl;
        v.lvl_out = x.at.lvl;
        if (!x.split || v.nco_exact) {
            const double p2 = v.phi2 + (double)nif * v.theta2;
            v.phi2 = p2 - std::floor(p2);
        }
    }
    // radio AF chain on the demodulator's stereo output
    void af_chain(ChainCtx& x) {
        Vfo& v = x.v;
        Vfo::Af& a = v.af;
        x.at.cur = &v.st[(size_t)v.i_out];
        x.bnd.clear();  // (the reference's blocks end at the demodulator; the push ends go on, in a list of the AF chain's own)
        if (x.split) { v.tk_af = v.tk_if; }
        x.tk = &v.tk_af;
        for (int s = 0; s < a.rate.n_stages; s++) { decim_step(x, v.st[(size_t)a.i_stage0 + s], a.rate, s, t_af_dec, af_dec); }
        if (a.i_poly >= 0) { poly_step(x, v.st[(size_t)a.i_poly], a.rate, nullptr, 0, 0, t_af_poly, af_poly); }
        if (a.i_hpf >= 0) { fir_step(x, v.st[(size_t)a.i_hpf], a.tp_hpf, a.d_hpf, (int)a.htaps.size(), a.hpf_kp, 0.0f, t_af_hpf, af_hpf); }
        if (a.i_deemp >= 0) {
            const Stream& in = *x.at.cur;
            Stream& nxt = v.st[(size_t)a.i_deemp];
            const int nseg = std::min(a.seg_cap, (in.n + SDRPP_DEEMP_SEG - 1) / SDRPP_DEEMP_SEG);
            af_deemp.add(x.at.lvl + 1, DeempJob{ (const float2*)in.data, (float2*)nxt.data, in.n, a.alpha, a.d_last + a.state_cur, a.d_last + (a.state_cur ^ 1),
                                                 a.d_seg + (size_t)a.state_cur * ((size_t)a.seg_cap + 1), nseg, 0 });
            if (nseg > 0) { a.state_cur ^= 1; }  // (a block without audio leaves the state where it is)
            nxt.n = in.n;
            x.at.lvl += 2;  // (the de-emphasis is two dependent launches: segment maps, then the outputs; a recursion over the block, no window into the last one)
            nxt.wlevel = x.at.lvl;
            x.at.cur = &nxt;
        }
        a.i_last = (int)(x.at.cur - &v.st[0]);
        v.lvl_af = x.at.lvl;
    }
    // RDS branch of the WFM demodulator (broadcast_fm.h:144-215, _rdsOut): beside the audio low-pass, off the stream the demodulator reads (`feed`).
    // Closed form: discriminator, translation and first decimator are ONE job list (vfo_rds_front_body) — a job per run of kRdsSegTiles tiles of every push,
    // anchored at its push: a launch group is anchored push by push, so grouped samples equal ungrouped ones bit for bit.  Reference rotator: one job per VFO
    // writes the rotated IF-rate stream, the first decimator follows as a plain FIR.  The later decimators and the polyphase stage are decim_step / poly_step.
    static constexpr int kRdsSegTiles = 4;
    void rds_branch(ChainCtx& x, const ChainCursor& feed) {
        Vfo& v = x.v;
        Vfo::Rds& r = v.rds;
        const Stream& in = *feed.cur;
        const int lvl = feed.lvl, nif = in.n;
        x.bnd.clear();  // (what the rotator needs of them is in the arena already)
        r.tk.clear();
        if (x.split) { r.tk = v.tk_if; }
        x.tk = &r.tk;
        x.at = feed;
        const float2* prev0 = reinterpret_cast<const float2*>(in.hist[in.cur]) + (in.hist_len - 1);  // the discriminator's previous sample
        RateChain& R = r.rate;
        const int K0 = R.ntaps(0), D0 = R.decim_s[0];
        if (r.exact) {
            Stream& rot = r.st[0];
            rdsx.add(lvl + 1, RdsRotXJob{ reinterpret_cast<const float2*>(in.data), prev0, reinterpret_cast<float2*>(rot.data), r.d_rot, r.pd_re, r.pd_im, v.d.inv_deviation, nif, x.d_bnd, x.nbnd });
            x.at.step(rot, nif);
            decim_step(x, r.st[(size_t)r.i_stage0], R, 0, t_af_dec, af_dec);
        }
        else {
            Stream& nxt = r.st[(size_t)r.i_stage0];
            StreamIn sin = stream_in(in);
            if (r.frozen) { sin.hist_len = 0; }  // the delay line the branch was left with (RdsJob::dline), not what the stream has seen since: nothing in front of the block is read
            RdsJob j{ sin, prev0, reinterpret_cast<float2*>(nxt.data), R.d_staps[0], r.frozen ? r.d_line[r.line_cur] : nullptr, K0, ilog2(D0), R.pos.soff[0], 0, 0,
                      r.tile, r.pitch, 0, v.d.inv_deviation, r.theta, r.phi };
            const size_t npush = x.split ? v.tk_if.size() : 1;
            int lo = 0, so = R.pos.soff[0], m = 0;
            for (size_t q = 0; q < npush; q++) {
                const int hi = x.split ? v.tk_if[q] : nif, nq = hi - lo;
                const int mq = decim_nout(nq, so, D0);
                j.anchor = lo;
                j.phi = r.phi;
                for (int a = m; a < m + mq; a += kRdsSegTiles * r.tile) {
                    j.m_lo = a;
                    j.m_hi = std::min(a + kRdsSegTiles * r.tile, m + mq);
                    rdsj.add(lvl + 1, j);
                }
                so = so + mq * D0 - nq;
                m += mq;
                const double p = r.phi + (double)nq * r.theta;
                r.phi = p - std::floor(p);
                lo = hi;
            }
            x.through_decim(R.pos.soff[0], D0);
            R.pos.soff[0] = so;
            x.at.step(nxt, m);
            if (r.frozen && nif > 0) {
                // the feed's history is the branch's delay line again only once the branch has seen K0 samples of it in a row; until then the block's
                // discriminator values are spliced onto the line it was left with (a job beside the first stage's, which reads the other side)
                r.line_fed += nif;
                if (r.line_fed >= K0) { r.frozen = false; }
                else {
                    rdsl.add(lvl + 1, RdsLineJob{ reinterpret_cast<const float2*>(in.data), prev0, r.d_line[r.line_cur], r.d_line[r.line_cur ^ 1], nif, K0, v.d.inv_deviation });
                    r.line_cur ^= 1;
                }
            }
        }
        for (int s = 1; s < R.n_stages; s++) { decim_step(x, r.st[(size_t)r.i_stage0 + s], R, s, t_af_dec, af_dec); }
        if (r.i_poly >= 0) { poly_step(x, r.st[(size_t)r.i_poly], R, nullptr, 0, 0, t_af_poly, af_poly); }  // (5000 phases: the branch keeps no matrix table)
        r.i_last = (int)(x.at.cur - &r.st[0]);
        r.lvl = x.at.lvl;
    }
    // Symbol branch of a RAW VFO (pocsag/dsp.h, clock_recovery/mm.h): front (discriminator, shaping FIR: a job per run of SDRPP_SYM_SEG samples) one level behind
    // the stream a demodulator would read (`feed`), loop (MM's recursion: a record per VFO, upload packs them into jobs) the level after.  The front reads one
    // side of the branch's carried lines and its last job writes the other: the sides flip with every block that has samples.  A launch group is one block
    // to the front; the loop is handed the push ends at the stream's rate and counts the symbols push by push.  A block without samples still files the loop's
    // record: it writes the zeros of its counts and leaves the state as it is.
    int sym_branch(ChainCtx& x, const ChainCursor& feed) {
        Vfo& v = x.v;
        Vfo::Sym& y = v.sym;
        const Stream& in = *feed.cur;
        const int lvl = feed.lvl, n = in.n;
        Stream &buf = y.st[0], &soft = y.st[1], &bits = y.st[2], &cnt = y.st[3];
        y.n_if = n;
        y.npush = x.split ? (int)v.tk_if.size() : 1;
        y.cap = y.cap_of(n);
        y.lvl = lvl + 2;
        for (int lo = 0; lo < n; lo += SDRPP_SYM_SEG) {  // (the branch's delay lines are its own: the feed's history is not read)
            syf.add(lvl + 1, SymFrontJob{ reinterpret_cast<const float2*>(in.data), y.d_lines, buf.data, y.d_taps, n, y.cur, y.K, y.T, lo, std::min(lo + SDRPP_SYM_SEG, n), y.inv_deviation, 0 });
        }
        if (n > 0) { y.cur ^= 1; }
        const int* d_ends = nullptr;
        if (x.split) {
            d_ends = arena_push(c, v.tk_if);
            if (!d_ends) { return arena_fail(c); }
        }
        syl.add(lvl + 2, SymLoopVfo{ buf.data, soft.data, reinterpret_cast<uint8_t*>(bits.data), reinterpret_cast<int*>(cnt.data), y.d_state, y.d_bank, d_ends, y.mu_gain, y.omega_gain, y.min_omega,
                                     y.max_omega, y.phases, y.T, n, y.npush, y.cap, 0 });
        buf.n = n;
        soft.n = y.cap;
        bits.n = (y.cap + 3) / 4;
        cnt.n = y.npush;
        for (auto& s : y.st) { s.wlevel = lvl + 2; }
        buf.wlevel = lvl + 1;
        return SDRPP_OK;
    }
    // Framer behind the symbol branch (m17_decoder/src/m17dsp.h: M17Slice4FSK, M17FrameDemux): ONE job per VFO and block (vfo_frame_kernels.h), one level behind the
    // branch's loop, whose soft values and per-push symbol counts of this block it reads.  Its state is one device array updated in place.  A launch group is one
    // block to the job: it counts the frames push by push.  A block without symbols still files the job: it writes the zeros of its counts.
    void frame_branch(ChainCtx& x) {
        Vfo& v = x.v;
        Vfo::Frame& f = v.frame;
        const Vfo::Sym& y = v.sym;
        Stream &recs = f.st[0], &cnt = f.st[1];
        f.npush = y.npush;
        f.cap = f.cap_of(y.cap);
        f.lvl = y.lvl + 1;
        FrameJob j{};
        j.soft = y.st[1].data;
        j.sym_counts = reinterpret_cast<const int*>(y.st[3].data);
        j.state = f.d_state;
        j.recs = reinterpret_cast<uint8_t*>(recs.data);
        j.counts = reinterpret_cast<int*>(cnt.data);
        j.table = f.d_table;
        j.high_cut = f.high_cut;
        j.n_sync = f.n_sync;
        for (int s = 0; s < f.n_sync; s++) {  // (stream order is LSB first in the job's words: the sync word's first bit in bit 0)
            uint32_t r = 0;
            for (int b = 0; b < 16; b++) { r |= (uint32_t)((f.sync[s] >> (15 - b)) & 1) << b; }
            j.sync[s] = r;
        }
        j.frame_bits = f.frame_bits;
        j.stride = f.stride;
        j.npush = f.npush;
        j.sym_cap = y.cap;
        j.rec_cap = f.cap;
        frj.add(f.lvl, j);
        recs.n = (f.cap * f.stride + 3) / 4;
        cnt.n = f.npush;
        for (auto& s : f.st) { s.wlevel = f.lvl; }
    }
    // RDS demodulator (radio/src/rds_demod.h): ONE job per VFO and block (vfo_rdsd_kernels.h), one level behind the polyphase stage of the RDS chain (source 0)
    // or behind the stream a demodulator would read (source 1).  Its state is one device array updated in place.  A launch group is one block to the job; it is
    // handed the push ends at its input's rate and counts the symbols push by push.  A block without samples still files the job: it writes the zeros of its counts.
    int rdsd_branch(ChainCtx& x, const ChainCursor& feed) {
        Vfo& v = x.v;
        Vfo::Rdsd& y = v.rdsd;
        const bool from_rds = y.source == 0;
        const Stream& in = from_rds ? v.rds.st[(size_t)v.rds.i_last] : *feed.cur;
        const int lvl = from_rds ? v.rds.lvl : feed.lvl, n = in.n;
        const std::vector<int>& tk = from_rds ? v.rds.tk : v.tk_if;
        Stream &soft = y.st[0], &bits = y.st[1], &cnt = y.st[2];
        y.n_in = n;
        y.npush = x.split ? (int)tk.size() : 1;
        y.cap = y.cap_of(n);
        y.lvl = lvl + 1;
        const int* d_ends = nullptr;
        if (x.split) {
            d_ends = arena_push(c, tk);
            if (!d_ends) { return arena_fail(c); }
        }
        rdsdj.add(lvl + 1, RdsdJob{ reinterpret_cast<const float2*>(in.data), soft.data, reinterpret_cast<uint8_t*>(bits.data), reinterpret_cast<int*>(cnt.data), y.d_state, y.d_taps, y.d_bank, d_ends,
                                    y.agc[0], y.agc[1], y.agc[2], y.loop[0][0], y.loop[0][1], y.loop[0][4], y.loop[0][5], y.loop[1][0], y.loop[1][1], y.loop[1][4], y.loop[1][5],
                                    y.mu_gain, y.omega_gain, y.min_omega, y.max_omega, y.K, y.T, y.phases, n, y.npush, y.cap, 0 });
        soft.n = y.cap;
        bits.n = (y.cap + 3) / 4;
        cnt.n = y.npush;
        for (auto& s : y.st) { s.wlevel = lvl + 1; }
        return SDRPP_OK;
    }
    // Meteor QPSK demodulator (meteor_demodulator/src/meteor_demod.h; vfo_qpsk_kernels.h): the shaping filter one level behind the stream a demodulator would
    // read — ONE record, which file_wave cuts into a job per segment of SDRPP_QPSK_SEG samples, as FMIF's — and everything sequential as ONE job a level behind
    // that.  The filter's line is two-sided (the block reads side `cur`, its last segment writes the other; flipped here per block that has samples); the loop's
    // state is one device array updated in place.  A launch group is one block to both; the loop is handed the push ends at the stream's rate and counts the
    // symbols push by push.  A block without samples files no front job and still files the loop: it writes the zeros of its counts.
    int qpsk_branch(ChainCtx& x, const ChainCursor& feed) {
        Vfo& v = x.v;
        Vfo::Qpsk& y = v.qpsk;
        const Stream& in = *feed.cur;
        const int lvl = feed.lvl, n = in.n;
        Stream &buf = y.st[0], &soft = y.st[1], &packed = y.st[2], &cnt = y.st[3];
        y.n_in = n;
        y.npush = x.split ? (int)v.tk_if.size() : 1;
        y.cap = y.cap_of(n);
        y.lvl = lvl + 2;
        if (n > 0) {
            qpf.add(lvl + 1, QpskFrontJob{ reinterpret_cast<const float2*>(in.data), y.d_lines, reinterpret_cast<float2*>(buf.data), y.d_taps, n, y.cur, y.K, 0 });
            y.cur ^= 1;
        }
        const int* d_ends = nullptr;
        if (x.split) {
            d_ends = arena_push(c, v.tk_if);
            if (!d_ends) { return arena_fail(c); }
        }
        qpl.add(lvl + 2, QpskLoopJob{ reinterpret_cast<const float2*>(buf.data), reinterpret_cast<float2*>(soft.data), reinterpret_cast<int8_t*>(packed.data), reinterpret_cast<int*>(cnt.data), y.d_state, y.d_bank,
                                      d_ends, y.agc[0], y.agc[1], y.agc[2], y.loop[0], y.loop[1], y.loop[4], y.loop[5], y.mu_gain, y.omega_gain, y.min_omega, y.max_omega, y.soft_scale,
                                      y.broken, y.oqpsk, y.T, y.phases, n, y.npush, y.cap, 0 });
        buf.n = n;
        soft.n = y.cap;
        packed.n = (y.cap + 1) / 2;
        cnt.n = y.npush;
        for (auto& s : y.st) { s.wlevel = lvl + 2; }
        buf.wlevel = lvl + 1;
        return SDRPP_OK;
    }
    void phase_advance(ChainCtx& x) {
        Vfo& v = x.v;
        if (x.have_phi_end) { v.phi = x.phi_end; }
        else {
            const double p = v.phi + (double)n_in * v.theta;
            v.phi = p - std::floor(p);
        }
        v.seen += n_in;
    }
    // history carries for every stream that has a consumer with memory
    void history_carries(ChainCtx& x) {
        Vfo& v = x.v;
        auto carry_at = [this](int cl, const Stream& s) { carry.add(cl, CarryJob{ s.data, s.hist[s.cur], s.hist[s.cur ^ 1], s.hist_len, s.n, s.width, s.hist_len }); };
        const Stream* phantom = (v.fused_front && v.rate.n_stages >= 2 && !v.nco_exact) ? &v.st[(size_t)v.i_first] : nullptr;  // stage-1 output of a fused front end: never written, never read
        for (auto& s : v.st) {
            const bool idle_fmi = v.i_fmi >= 0 && &s == &v.st[(size_t)v.i_fmi] && !(x.ifc_on && v.ifc.fm_on && v.ifc.nbsq());  // (no chain writes it: nothing to carry)
            if (s.hist_len > 0 && s.data && &s != phantom && !idle_fmi && (x.ifc_on || v.i_ifc < 0 || &s != &v.st[(size_t)v.i_ifc])) {
                // pipelined: at the level of the consumer (its window of the NEXT block reads the new history one tick later, the carry of
                // the next block overwrites the old one one tick later still); a stream nobody reads with memory (a consumer may be attached
                // later: sdrpp_vfo_set_af, a taps change): one level behind the role that WRITES it — not behind the whole chain, which with
                // an AF chain is up to a dozen levels later, when the stream's ring buffer (kRing = 4) already holds a later block
                const int cl = !ticking ? carry_last : (s.clevel > 0 ? s.clevel : (s.wlevel > 0 ? s.wlevel + 1 : x.at.lvl + 1));
                carry_at(cl, s);
            }
        }
        if (v.stereo.ran) {  // the stereo branch's own streams
            for (auto& s : v.stereo.st) {
                if (s.hist_len > 0 && s.data) { carry_at(!ticking ? carry_last : s.clevel, s); }
            }
        }
        if (v.rds.ran) {  // the RDS branch's own streams (every one of them is written and read whenever the branch runs)
            for (auto& s : v.rds.st) {
                if (s.hist_len > 0 && s.data) { carry_at(!ticking ? carry_last : (s.clevel > 0 ? s.clevel : s.wlevel + 1), s); }
            }
        }
    }

    // ---- front-end jobs: the tap operand on the device, the in-tile phasors, one function per path that builds a job and files it ----
    static constexpr double kTwoPi = 2.0 * 3.14159265358979323846;
    // NCO advance inside a tile: exp(j * 2 * pi * step * jj) for jj = 0 .. n - 1, written to out[jj * stride]
    static void tile_phasors(float2* out, size_t stride, int n, double step) {
        for (int jj = 0; jj < n; jj++) {
            double tt = step * (double)jj;
            tt -= std::rint(tt);
            const double a = kTwoPi * tt;
            out[(size_t)jj * stride] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    }
    // Tap operand of a front-end job, cached on the device under its membership key: `fill` writes the n (zeroed) entries of a table that is
    // not there yet.  The one place that owns the cache's policy, the upload and its synchronisation.
    template <class Fill>
    int front_taps(const std::string& key, size_t n, Fill&& fill, float2** d_taps) {
        auto it = c->s1_tap_cache.find(key);
        if (it != c->s1_tap_cache.end()) {
            *d_taps = it->second;
            return SDRPP_OK;
        }
        std::vector<float2> host(n, make_float2(0.0f, 0.0f));
        fill(host);
        if (c->s1_tap_cache.size() > 4096) {  // retune churn: drop everything (rare)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (auto& e : c->s1_tap_cache) { (void)hipFree(e.second); }
            c->s1_tap_cache.clear();
        }
        *d_taps = nullptr;
        int rc = dev_alloc(c, d_taps, host.size());
        if (rc) { return rc; }
        HIPCHK(c, hipMemcpyAsync(*d_taps, host.data(), host.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // `host` is pageable and goes out of scope
        c->s1_tap_cache[key] = *d_taps;
        return SDRPP_OK;
    }
    // composite matrix table of members m[0 .. vt) (h, K, NP4: add_matrix_job): [NP4][64] floats (= NP4 * 32 float2; rows >= NP are zero padding) followed by [32][TILE] float2
    static void fill_composite(std::vector<float2>& host, const S1Member& h, bool m_long, int K, int NP4, const S1Member* m, int vt) {
        const int D1 = 1 << h.lgD, NP = (K + 1) / 2;
        float* at = reinterpret_cast<float*>(host.data());
        std::vector<double> h12((size_t)K);
        const double kc = 0.5 * (double)(K - 1);
        for (int i = 0; i < vt; i++) {
            const Vfo& vv = *m[i].v;
            // composite taps h12 = h1 (*) upsample(h2, D1) in double precision (both are linear phase, so is h12)
            std::fill(h12.begin(), h12.end(), 0.0);
            for (int k2 = 0; k2 < h.K2; k2++) {
                const double w2 = m_long ? 1.0 : (double)vv.rate.staps[1][(size_t)k2];
                for (int k1 = 0; k1 < h.K; k1++) { h12[(size_t)k2 * D1 + k1] += w2 * (double)vv.rate.staps[0][(size_t)k1]; }
            }
            for (int pz = 0; pz < NP; pz++) {
                double t = ((double)pz - kc) * vv.theta;  // modulation centred on the filter: g[K-1-k] = conj(g[k])
                t -= std::rint(t);
                const double a = kTwoPi * t;
                double gr = h12[(size_t)pz] * std::cos(a), gi = h12[(size_t)pz] * std::sin(a);
                if ((K & 1) && pz == NP - 1) { gr = h12[(size_t)pz]; gi = 0.0; }
                at[(size_t)pz * 64 + i] = (float)gr;
                at[(size_t)pz * 64 + 32 + i] = (float)-gi;
            }
        }
        for (int i = 0; i < SDRPP_FCM_VT; i++) {
            tile_phasors(&host[(size_t)NP4 * 32 + (size_t)i * SDRPP_FCM_TILE], 1, SDRPP_FCM_TILE, i < vt ? m[i].v->theta * (double)(1 << (h.lgD + h.lgD2)) : 0.0);
        }
    }
    // VALU pair table of members m[0 .. vt): [tap pairs][vt] modulated taps followed by [256][vt] phasors
    static void fill_pairs(std::vector<float2>& host, const S1Member* m, int vt) {
        const int K = (m[0].K + 1) / 2;  // tap pairs
        for (int k = 0; k < K; k++) {
            for (int i = 0; i < vt; i++) { host[(size_t)k * vt + i] = m[i].v->modtaps[(size_t)k]; }
        }
        // NCO advance inside a 256-output tile: exp(j*2*pi*theta*D1*j) (fused front kernel)
        for (int i = 0; i < vt; i++) { tile_phasors(&host[(size_t)K * vt + i], (size_t)vt, 256, m[i].v->theta * (double)(1 << m[0].lgD)); }
    }
    // what every front-end job says about its members m[0 .. vt), in n entries (the matrix kernels read all of theirs: the last member again)
    template <class Job>
    static void job_members(Job& job, const S1Member* m, int vt, int n, int stream) {
        job.nv = vt;
        job.min_idx = m[0].min_idx;
        job.anchor = m[0].shift;
        for (int i = 0; i < n; i++) {
            const S1Member& mi = m[std::min(i, vt - 1)];
            job.theta[i] = mi.v->theta;
            job.phi0[i] = mi.phi0;  // phase (turns) of push-relative sample 0
            job.out[i] = (float2*)mi.v->st[(size_t)mi.v->i_first + stream].data + m[0].oshift;
        }
    }
    // One job of the matrix-core path for members m[0 .. vt): its FrontCMJob, built and filed in its launch.  The job's filter is the composite
    // of stages 1 + 2, or a long first stage alone (m_pf: the prefetch depth frontcm_ok picked for a composite).
    int add_matrix_job(const S1Member* m, int vt, bool m_long, int m_pf) {
        S1Member h = m[0];  // the job's geometry (that of its first member)
        if (m_long) { h.K2 = 1; h.lgD2 = 0; h.off2 = 0; h.nout2 = h.nout; }  // the "composite" is the first stage alone
        const int D1 = 1 << h.lgD, K = h.K + (h.K2 - 1) * D1, lgD = h.lgD + h.lgD2;
        const int NP4 = ((K + 1) / 2 + 31) / 32 * 32;  // rows of the tap operand table, zero padded (the kernels read whole rings: up to 32 rows — eight steps of four pairs — at a time)
        float2* d_taps = nullptr;
        int rc = front_taps(member_key(m_long ? 'L' : 'M', m, vt), (size_t)NP4 * 32 + (size_t)SDRPP_FCM_VT * SDRPP_FCM_TILE, [&](std::vector<float2>& host) { fill_composite(host, h, m_long, K, NP4, m, vt); }, &d_taps);
        if (rc) { return rc; }
        FrontCMJob job{};
        job_members(job, m, vt, SDRPP_FCM_VT, m_long ? 0 : 1);
        job.ntaps = K;
        job.log2_decim = lgD;
        job.off = h.off0 + (h.off2 - (h.K2 - 1)) * D1 - (h.K - 1) + h.shift;
        job.nout = h.nout2;
        // (a long first stage with at most 16 VFOs runs in the 16 x 16 x 4 shape: 16 outputs per tile, vfo_frontcl_impl<PF, true>)
        const int tile_n = (m_long && vt <= 16) ? 16 : SDRPP_FCM_TILE;
        const int ntiles = (h.nout2 + tile_n - 1) / tile_n;
        // one resident round: 256 CUs x 3 blocks x 4 wavefronts (a second, partly filled round would cost as much as the first);
        // the long-stage kernel runs 2 wavefronts per block, its LDS footprint decides how many blocks fit
        const int long_blocks = m_long ? std::max(1, (int)((size_t)(160 * 1024) / ((size_t)frontcl_lds_floats(K, lgD, fcl_nw) * 4))) : 0;
        // (a launch group brings one job per push: together they get the wavefronts one job of the whole block would)
        const int nsub = std::max<int>(1, (int)c->grp_ends.size());
        const int resident = std::max(64, (m_long ? 256 * long_blocks * fcl_nw : (ticking ? std::min(3072, c->tick_fcm_waves) : 3072)) / nsub);
        job.tiles_per_wave = std::max(1, (ntiles + resident - 1) / resident);
        if (c->front_walk_waves > 0) { job.tiles_per_wave = std::max(1, (ntiles + c->front_walk_waves - 1) / c->front_walk_waves); }
        job.atab = reinterpret_cast<const float*>(d_taps);
        job.ptab = d_taps + (size_t)NP4 * 32;
        FCMLaunch& L = m_long ? fcl : fcm[m_pf == 6 ? 0 : (m_pf == 10 ? 1 : 2)];
        const int waves = (m_long ? fcl_nw : 4) * job.tiles_per_wave;  // tiles a workgroup walks
        L.jobs.push_back(job);
        L.max_blocks = std::max(L.max_blocks, (ntiles + waves - 1) / waves);
        L.lds = std::max(L.lds, m_long ? (size_t)frontcl_lds_floats(K, lgD, fcl_nw) * 4 : (size_t)frontcm_layout(K, lgD).total * 4);
        return SDRPP_OK;
    }
    // One job of the VALU path for members m[0 .. vts[li]), built and filed in launch class li: a Front2Job (stages 1 + 2 fused) or a Stage1Job
    int add_valu_job(const S1Member* m, int li) {
        const int vt = vts[li];
        const S1Member& h = m[0];
        float2* d_taps = nullptr;  // tap array for this membership (cached on the device)
        int rc = front_taps(member_key('V', m, vt), (size_t)((h.K + 1) / 2) * vt + (size_t)256 * vt, [&](std::vector<float2>& host) { fill_pairs(host, m, vt); }, &d_taps);
        if (rc) { return rc; }
        const int D1 = 1 << h.lgD;
        if (h.fused) {
            Front2Job job{};
            job_members(job, m, vt, vt, 1);
            job.ntaps1 = h.K;
            job.log2_decim1 = h.lgD;
            job.off1 = h.off0 + h.shift;
            job.ntaps2 = h.K2;
            job.log2_decim2 = h.lgD2;
            job.off2 = h.off2;
            job.nout2 = h.nout2;
            job.t2 = front2_t2(h.K, D1, h.K2, 1 << h.lgD2, 8);
            job.ctaps = d_taps;
            job.ptab = d_taps + (size_t)((h.K + 1) / 2) * vt;
            job.taps2 = h.v->d_staps_nat[1];
            f2l[li].jobs.push_back(job);
            f2l[li].max_blocks = std::max(f2l[li].max_blocks, (job.nout2 + job.t2 - 1) / job.t2);
            f2l[li].lds = std::max(f2l[li].lds, (std::max((size_t)D1 * (256 + (h.K - 1 + D1 - 1) / D1 + 1), (size_t)vt * 272) + (size_t)vt) * sizeof(float2));
            return SDRPP_OK;
        }
        Stage1Job job{};
        job_members(job, m, vt, vt, 0);
        job.ntaps = h.K;
        job.log2_decim = h.lgD;
        job.off0 = h.off0 + h.shift;
        job.nout = h.nout;
        job.ctaps = d_taps;
        s1l[li].jobs.push_back(job);
        s1l[li].max_nout = std::max(s1l[li].max_nout, job.nout);
        const int tile = pick_tile(D1, h.K, 8);
        if (tile == 0 && h.lgD < 5) { return fail(c, SDRPP_ERR_UNSUPPORTED, "stage-1 filter (decim %d, %d taps) does not fit in LDS", D1, h.K); }
        if (tile > 0) { s1l[li].tile = std::min(s1l[li].tile, tile); }
        return SDRPP_OK;
    }

    // ---- stage 1 (optionally fused with stage 2): group VFOs with identical geometry, VT per job ----
    int group_front() {
        auto same = [](const S1Member& a, const S1Member& b) {
            return a.fused == b.fused && a.K == b.K && a.lgD == b.lgD && a.off0 == b.off0 && a.nout == b.nout && a.min_idx == b.min_idx && a.K2 == b.K2 &&
                   a.lgD2 == b.lgD2 && a.off2 == b.off2 && a.nout2 == b.nout2 && a.taph == b.taph && a.shift == b.shift && a.oshift == b.oshift;
        };
        std::sort(s1.begin(), s1.end(), [](const S1Member& a, const S1Member& b) {
            if (a.fused != b.fused) { return a.fused < b.fused; }
            if (a.K != b.K) { return a.K < b.K; }
            if (a.lgD != b.lgD) { return a.lgD < b.lgD; }
            if (a.off0 != b.off0) { return a.off0 < b.off0; }
            if (a.nout != b.nout) { return a.nout < b.nout; }
            if (a.min_idx != b.min_idx) { return a.min_idx < b.min_idx; }
            if (a.K2 != b.K2) { return a.K2 < b.K2; }
            if (a.lgD2 != b.lgD2) { return a.lgD2 < b.lgD2; }
            if (a.off2 != b.off2) { return a.off2 < b.off2; }
            if (a.nout2 != b.nout2) { return a.nout2 < b.nout2; }
            if (a.taph != b.taph) { return a.taph < b.taph; }
            if (a.shift != b.shift) { return a.shift < b.shift; }
            if (a.oshift != b.oshift) { return a.oshift < b.oshift; }
            return a.v->id < b.v->id;
        });
        if (ticking) {
            fcl_nw = 4;
            for (auto& m : s1) {
                if (!m.fused && m.lgD >= 5 && m.K >= 9 && (size_t)frontcl_lds_floats(m.K, m.lgD, 4) * 4 > (size_t)(160 * 1024 / 2)) { fcl_nw = 2; }
            }
        }
        // A long first stage whose TWO engines' planes exceed a workgroup's LDS while one engine's fit (plan 8192's /128 stage of 726 taps: 77 056 B
        // against 38 656 B) runs with one tile engine per workgroup, and the launch with it: a launch has one engine count (aux).  Only where
        // such a stage has a job to fill (two VFOs of one geometry): a launch without one keeps the count it had.
        auto one_engine_only = [](const S1Member& m) {
            return !m.fused && m.lgD >= 5 && m.K >= 9 && (size_t)frontcl_lds_floats(m.K, m.lgD, 2) * 4 > (size_t)kMaxLds && (size_t)frontcl_lds_floats(m.K, m.lgD, 1) * 4 <= (size_t)kMaxLds;
        };
        for (size_t a = 0; a < s1.size();) {
            size_t b = a;
            while (b < s1.size() && same(s1[b], s1[a])) { b++; }
            if (b - a >= 2 && one_engine_only(s1[a])) { fcl_nw = 1; }
            a = b;
        }
        size_t i = 0;
        while (i < s1.size()) {
            size_t j = i;
            while (j < s1.size() && same(s1[j], s1[i])) { j++; }
            size_t g = i;
            // ---- matrix-core path: >= 17 fused VFOs of one geometry -> jobs of up to 32 VFOs, stages 1 + 2 as one composite FIR ----
            int m_pf = 0;
            const bool m_fused = s1[i].fused && frontcm_ok(s1[i].K, s1[i].lgD, s1[i].K2, s1[i].lgD2, &m_pf);
            // ... or a long first stage on its own (decimation >= 32: no fusion, vfo_frontcl_kernel)
            const bool m_long = !m_fused && !s1[i].fused && s1[i].lgD >= 5 && s1[i].K >= 9 && (size_t)frontcl_lds_floats(s1[i].K, s1[i].lgD, fcl_nw == 1 ? 1 : 2) * 4 <= (size_t)kMaxLds;
            const bool m_ok = m_fused || m_long;
            // worth it from 17 VFOs against the fused VALU kernel (8 VFOs per work-item); a long first stage has no good VALU form (its
            // per-VFO windows do not fit LDS), there the matrix kernel pays off from 2 VFOs on
            const size_t m_min = m_long ? 2 : 17;
            while (m_ok && j - g >= m_min) {
                const int vt = (int)std::min<size_t>(j - g, SDRPP_FCM_VT);
                int rc = add_matrix_job(&s1[g], vt, m_long, m_pf);
                if (rc) { return rc; }
                g += (size_t)vt;
            }
            while (g < j) {
                const size_t left = j - g;
                int li = left >= 8 ? 0 : (left >= 4 ? 1 : (left >= 2 ? 2 : 3));
                if (ticking) { li = 3; }  // (pipelined: one VFO per job — the forms that are roles of the tick kernel, TR_S1_1 / TR_S1D_1 / TR_F2_1; same sums per VFO)
                int rc = add_valu_job(&s1[g], li);
                if (rc) { return rc; }
                g += (size_t)vts[li];
            }
            i = j;
        }
        return SDRPP_OK;
    }

    // ---- job tables into the arena (one upload for the whole block) ----
    // a table that is not a Lev<> list: false = it has jobs and they did not fit
    template <class T>
    bool push_table(const std::vector<T>& jobs, T*& dev) {
        dev = arena_push(c, jobs);
        return jobs.empty() || dev;
    }
    int upload() {
        for (int k = 0; k < 4; k++) {
            for (auto& jb : s1l[k].jobs) { s1l[k].lds = std::max(s1l[k].lds, fir_lds(s1l[k].tile, 1 << jb.log2_decim, jb.ntaps, 8)); }
            if (!push_table(s1l[k].jobs, d_s1[k])) { return arena_fail(c); }
        }
        for (int k = 0; k < 4; k++) {
            if (!push_table(f2l[k].jobs, d_f2[k])) { return arena_fail(c); }
        }
        if (!fcl.jobs.empty()) {
            // Tiles per wavefront of the long first stages, chosen over ALL their jobs (round 5, profiles/r05h_fcl_tiles_per_wave*.log): a tile is
            // mostly start-up (window fetch, tile phasor, epilogue) around a matrix loop of 3 us (16 rows) .. 12 us (32 rows), and a wavefront that
            // walks several tiles fetches the next window under the current loop — but the walks must still fill the device: the best setting
            // put ~0.7 of the resident wavefront slots to work (cfg 4 at 10^6-sample blocks: 2 tiles per 32-row, 4 per 16-row wavefront, 8.29 ->
            // 8.89 GS/s; at 307 200: 1 and 2, 5.11 -> 5.26; twice that was 15 % slower at either size).
            size_t lds_max = 0;
            for (auto& jb : fcl.jobs) { lds_max = std::max(lds_max, (size_t)frontcl_lds_floats(jb.ntaps, jb.log2_decim, fcl_nw) * 4); }
            const int long_blocks = std::max(1, (int)((size_t)(160 * 1024) / std::max<size_t>(lds_max, 1)));
            const double target = 0.7 * 256.0 * (double)long_blocks * (double)fcl_nw;
            fcl.max_blocks = 0;
            // Round 6: the jobs of a tick differ in what a tile costs — 257 .. 400 taps (NFM / USB / AM at 61.44 MS/s), 32-row or 16-row tiles — and a walk of
            // the SAME number of tiles took 1.5x as long in one job as in another: the tick ended on the 400-tap jobs' workgroups (last end 337 us against a
            // mean life of 220, profiles/r06q_tick_timeline_cfg4_B1000000_group4.txt).  Walk lengths now follow a cost model, tile ~ c0 + c1 * taps (16-row
            // tiles: 0.45 of the matrix part), so that every wavefront of the role is busy about equally long; the total number of wavefronts still follows
            // the 0.7-of-the-resident-slots rule (profiles/r06s_fcl_balance.log).
            constexpr double c0 = 1.5, c1 = 0.031;
            auto tile_cost = [&](const FrontCMJob& jb) { return c0 + c1 * (double)jb.ntaps * (jb.nv <= 16 ? 0.45 : 1.0); };
            double total_cost = 0.0;
            for (auto& jb : fcl.jobs) {
                const int tile_n = jb.nv <= 16 ? 16 : SDRPP_FCM_TILE;
                total_cost += tile_cost(jb) * (double)((jb.nout + tile_n - 1) / tile_n);
            }
            const double per_wave = total_cost / target;  // what one wavefront should carry
            for (auto& jb : fcl.jobs) {
                const int tile_n = jb.nv <= 16 ? 16 : SDRPP_FCM_TILE;
                const int ntiles = (jb.nout + tile_n - 1) / tile_n;
                // (ticks: the rule above.  An ordinary pass has the device to itself and its pushes are long: one resident round per JOB as before —
                // the 0.7 rule gave walks of 34 tiles at 2^24-sample pushes and lost 17 % there, profiles/r05z_bench_default.json vs r05d)
                const int resident = 256 * long_blocks * fcl_nw;
                int tpw = ticking ? std::max(1, (int)((double)ntiles * (double)fcl.jobs.size() / target + 0.75)) : std::max(1, (ntiles + resident - 1) / resident);
                if (ticking && fcl.jobs.size() > 1) { tpw = std::max(1, (int)(per_wave / tile_cost(jb) + 0.5)); }
                if (c->front_walk_waves > 0) { tpw = std::max(1, (ntiles + c->front_walk_waves - 1) / c->front_walk_waves); }
                jb.tiles_per_wave = tpw;
                fcl.max_blocks = std::max(fcl.max_blocks, (ntiles + fcl_nw * tpw - 1) / (fcl_nw * tpw));
            }
        }
        if (!push_table(fcl.jobs, d_fcl)) { return arena_fail(c); }
        for (int k = 0; k < 3; k++) {
            if (!push_table(fcm[k].jobs, d_fcm[k])) { return arena_fail(c); }
        }
        if (!push_table(rotx, d_rotx) || !push_table(retune, d_retune) || !push_table(rot, d_rot)) { return arena_fail(c); }
        d_fb = (!rotx.empty()) ? arena_push(c, fb) : nullptr;
        d_rotx_head = nullptr;
        if (!rotx.empty() && !d_fb) { return arena_fail(c); }
        if (!rotx.empty() && ticking) {
            std::vector<RotXHead> head{ RotXHead{ d_rotx, d_fb, (int)rotx.size(), (int)fb.size(), c->rot_exact_vpw, 0 } };
            if (!push_table(head, d_rotx_head)) { return arena_fail(c); }
        }
        // Pipelined back ends: ONE launch — or none, when this push is better served by the separate launches
        pipe_seg = pipe_segments(pipes, c->pipe_on, pipe_lds);
        if (!pipes.empty() && pipe_seg == 0) {  // not this push: the same four jobs go to the separate launches
            for (auto& pj : pipes) {
                t_dec.add(pj.lvl, pj.st[0]);
                t_poly.add(pj.lvl + 1, pj.st[1]);
                t_chan.add(pj.lvl + 2, pj.st[2]);
                t_audio_fm.add(pj.lvl + 3, pj.st[3]);
            }
            pipes.clear();
        }
        if (!pipes.empty()) {
            for (auto& pj : pipes) { pipe_lvl = std::max(pipe_lvl, pj.lvl); }
            d_pipes = arena_push(c, pipes);
            if (!d_pipes) { return arena_fail(c); }
        }
        // 1. every list the chain walk filled goes into the arena
        int rc = SDRPP_OK, i = 0;
        for_each_list([&](auto& L) {
            if constexpr (std::is_same_v<decltype(L), Lev<ToepJob>&>) {  // the registry's first kToepLists, in tlists[]' order: list i
                // (the plan of a list sets its jobs' macro tiles per wavefront: before the jobs are copied into the arena)
                for (int l = 0; l < L.top && !rc; l++) {
                    if (L.at[l].empty()) { continue; }
                    tplan[i][l] = toep_plan(L.at[l], tlists[i].npl, ticking ? std::min(2048, c->tick_toep_blocks) : 2048);
                    if (tplan[i][l].lds > (size_t)kMaxLds) { rc = fail(c, SDRPP_ERR_UNSUPPORTED, "matrix-core FIR window does not fit in LDS"); }
                }
                i++;
            }
            if (!rc && !arena_push_lev(c, L)) { rc = arena_fail(c); }
        });
        if (rc) { return rc; }
        if (i != kToepLists) { return fail(c, SDRPP_ERR_INVALID, "for_each_list: %d matrix-core lists, tlists[] has %d rows", i, kToepLists); }
        // ... and the stereo loops' per-VFO records SDRPP_ST_PACK to a job — the fewer rows a wavefront stages, the longer its chunks (SDRPP_ST_LOOP_CHUNK
        // elements together); rows lie an odd number of floats apart in its LDS
        for (int l = 0; l < stl.top; l++) {
            for (size_t k = 0; k < stl.at[l].size(); k += SDRPP_ST_PACK) {
                const int nv = (int)std::min<size_t>(SDRPP_ST_PACK, stl.at[l].size() - k);
                const int chunk = SDRPP_ST_LOOP_CHUNK / nv;
                int nmax = 0;
                for (int q = 0; q < nv; q++) { nmax = std::max(nmax, stl.at[l][k + (size_t)q].n); }
                stlj.add(l, StereoLoopJob{ stl.dev[l] + k, nv, chunk, chunk | 1, nmax });
            }
        }
        if (!arena_push_lev(c, stlj)) { return arena_fail(c); }
        // ... and the symbol loops' per-VFO records, a lane each: as few jobs as SDRPP_SYM_PACK lanes allow, the records spread evenly over them
        for (int l = 0; l < syl.top; l++) {
            const size_t N = syl.at[l].size();
            if (N == 0) { continue; }
            const size_t njobs = (N + SDRPP_SYM_PACK - 1) / SDRPP_SYM_PACK, per = (N + njobs - 1) / njobs;
            for (size_t k = 0; k < N; k += per) { sylj.add(l, SymLoopJob{ syl.dev[l] + k, (int)std::min(per, N - k), 0 }); }
        }
        if (!arena_push_lev(c, sylj)) { return arena_fail(c); }
        // 2. every record under the role, kind by kind: the order of a level's jobs, four neighbours to a workgroup
        file_wave(nbsq, WK_NBSQ);
        file_wave(fmif, WK_FMIF);
        file_wave(rdsj, WK_RDS_FRONT);
        file_wave(rdsl, WK_RDS_LINE);
        file_wave(rdsx, WK_RDS_ROTX);
        file_wave(stp, WK_ST_PILOT);
        file_wave(stlj, WK_ST_LOOP);
        file_wave(stm, WK_ST_MATRIX);
        file_wave(syf, WK_SYM_FRONT);
        file_wave(sylj, WK_SYM_LOOP);
        file_wave(rdsdj, WK_RDS_DEMOD);
        file_wave(qpl, WK_QPSK_LOOP);  // (in front of the filter's jobs: a loop job filed at its filter's level would read the buffer BEFORE it is written wherever wavefronts start in table order — the emulator — and the tests see it)
        file_wave(qpf, WK_QPSK_FRONT);
        file_wave(frj, WK_SYM_FRAME);
        // 3. the role's table
        if (!arena_push_lev(c, wave)) { return arena_fail(c); }
        HostScope hs("arena_commit (H2D)");
        return arena_commit(c);
    }

    // The records of one kind, in the arena already, as jobs of the wavefront-job role: a job per record — FMIF's records a job per segment of kFmifSeg
    // samples, the QPSK front's a job per segment of SDRPP_QPSK_SEG samples, the segment's first sample in WaveJob::arg.
    template <class T>
    void file_wave(const Lev<T>& recs, WaveKind kind) {
        for (int l = 0; l < recs.top; l++) {
            for (size_t k = 0; k < recs.at[l].size(); k++) {
                int n = 1, step = 1;
                if constexpr (std::is_same_v<T, FmifJob>) { n = recs.at[l][k].n; step = kFmifSeg; }
                if constexpr (std::is_same_v<T, QpskFrontJob>) { n = recs.at[l][k].n; step = SDRPP_QPSK_SEG; }
                for (int lo = 0; lo < n; lo += step) { wave.add(l, WaveJob{ recs.dev[l] + k, kind, lo }); }
                if (wave_kind_uses_lds(kind)) { wave_lds = (size_t)4 * SDRPP_WAVE_LDS_FLOATS * sizeof(float); }
            }
        }
    }

    // ---- level 1: the front end ----
    // f(std::integral_constant<int, VT>) for the VFOs per work-item of a VALU launch class (vts[]): its kernels take them as a template argument
    template <class F>
    static void with_vt(int vt, F&& f) {
        switch (vt) {
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 1>{}); break;
        }
    }
    int emit_front() {
        {
            FamilyTimer t(c, F_S1);
            if (!rotx.empty() && n_in > 0) {
                if (c->rot_exact_single) {
                    count_form(c, PF_ROTX_1);
                    launch(c, vfo_rotate_exact_kernel, dim3(((unsigned)rotx.size() + 63) / 64), dim3(64), (size_t)64 * 65 * sizeof(float2), src, (const RotXJob*)d_rotx, (int)rotx.size(), d_fb, (int)fb.size());
                }
                else if (ticking) {  // pipelined: the chain as a role of the tick (level 1: its VFOs' first stages follow at level 2)
                    emit(c, L0 + 1, F_S1, TR_ROTX16, ((int)rotx.size() + c->rot_exact_vpw - 1) / c->rot_exact_vpw, 1, SDRPP_ROTX4_LDS_BYTES, d_rotx_head, &src);
                }
                else {
                    const int vpw = c->rot_exact_vpw;
                    const dim3 grid(((unsigned)rotx.size() + vpw - 1) / vpw);
                    count_form(c, TR_ROTX16);
                    launch(c, vfo_rotate_exact4_kernel<16>, grid, dim3(256), SDRPP_ROTX4_LDS_BYTES, src, (const RotXJob*)d_rotx, (int)rotx.size(), d_fb, (int)fb.size(), vpw);
                }
            }
            for (int k = 0; k < 4; k++) {
                if (s1l[k].jobs.empty() || s1l[k].max_nout == 0) { continue; }
                bool direct = true;  // every job of the class decimates by >= 32: stream from global memory, no LDS tile
                for (auto& jb : s1l[k].jobs) { direct = direct && jb.log2_decim >= 5; }
                if (direct) {
                    if (ticking && s1l[k].vt == 1) {
                        emit(c, L0 + 1, F_S1, TR_S1D_1, (s1l[k].max_nout + 255) / 256, (int)s1l[k].jobs.size(), 0, d_s1[k], &src);
                        continue;
                    }
                    const dim3 grid((s1l[k].max_nout + 255) / 256, (unsigned)s1l[k].jobs.size());
                    count_form(c, s1l[k].vt == 8 ? (int)PF_S1D_8 : (s1l[k].vt == 4 ? (int)PF_S1D_4 : (s1l[k].vt == 2 ? (int)PF_S1D_2 : (int)TR_S1D_1)));
                    with_vt(s1l[k].vt, [&](auto vt) { launch(c, vfo_stage1_direct_kernel<decltype(vt)::value>, grid, dim3(256), 0, src, (const Stage1Job*)d_s1[k]); });
                    continue;
                }
                if (ticking && s1l[k].vt == 1) {
                    emit(c, L0 + 1, F_S1, TR_S1_1, (s1l[k].max_nout + s1l[k].tile - 1) / s1l[k].tile, (int)s1l[k].jobs.size(), s1l[k].lds, d_s1[k], &src, s1l[k].tile);
                    continue;
                }
                const dim3 grid((s1l[k].max_nout + s1l[k].tile - 1) / s1l[k].tile, (unsigned)s1l[k].jobs.size());
                const dim3 block(s1l[k].tile);
                count_form(c, s1l[k].vt == 8 ? (int)PF_S1_8 : (s1l[k].vt == 4 ? (int)PF_S1_4 : (s1l[k].vt == 2 ? (int)PF_S1_2 : (int)TR_S1_1)));
                with_vt(s1l[k].vt, [&](auto vt) { launch(c, vfo_stage1_kernel<decltype(vt)::value>, grid, block, s1l[k].lds, src, (const Stage1Job*)d_s1[k]); });
            }
            for (int k = 0; k < 4; k++) {
                if (f2l[k].jobs.empty() || f2l[k].max_blocks == 0) { continue; }
                if (ticking && f2l[k].vt == 1) {
                    emit(c, L0 + 1, F_S1, TR_F2_1, f2l[k].max_blocks, (int)f2l[k].jobs.size(), f2l[k].lds, d_f2[k], &src);
                    continue;
                }
                const dim3 grid((unsigned)f2l[k].max_blocks, (unsigned)f2l[k].jobs.size());
                const dim3 block(256);
                // all jobs of a launch class share VT; the (44 taps, /8) first stage of the ratio-32 plan (10 MS/s -> 312.5 kS/s) has a
                // fully unrolled instance, everything else runs the generic loop
                bool all_44_3 = true;
                for (auto& jb : f2l[k].jobs) { all_44_3 = all_44_3 && jb.ntaps1 == 44 && jb.log2_decim1 == 3; }
                count_form(c, f2l[k].vt == 8 ? (int)(all_44_3 ? PF_F2_8_44_3 : PF_F2_8) : (f2l[k].vt == 4 ? (int)PF_F2_4 : (f2l[k].vt == 2 ? (int)PF_F2_2 : (int)TR_F2_1)));
                if (f2l[k].vt == 8 && all_44_3) { launch(c, vfo_front2_kernel<8, 44, 3>, grid, block, f2l[k].lds, src, (const Front2Job*)d_f2[k]); }
                else { with_vt(f2l[k].vt, [&](auto vt) { launch(c, vfo_front2_kernel<decltype(vt)::value, 0, 0>, grid, block, f2l[k].lds, src, (const Front2Job*)d_f2[k]); }); }
            }
            for (int k = 0; k < 3; k++) {
                if (fcm[k].jobs.empty() || fcm[k].max_blocks == 0) { continue; }
                bool all_132_4 = true;  // ratio-32 plan: fir_32_8 (44 taps, /8) + fir_4_2 (12 taps, /2) -> 132 composite taps, /16
                for (auto& jb : fcm[k].jobs) { all_132_4 = all_132_4 && jb.ntaps == 132 && jb.log2_decim == 4; }
                const int role = (k == 1 && all_132_4) ? TR_FCM_132_4 : (k == 0 ? TR_FCM_6 : (k == 1 ? TR_FCM_10 : TR_FCM_16));
                // small blocks: every wavefront of the 32 x 32 x 2 form would have ONE tile and spend 4 us in its matrix loop alone — a workgroup
                // per tile in the 16 x 16 x 4 shape instead (same sums in the same order: bit-identical), up to fcm16_max_tiles tiles per job
                int max_tiles = 0;
                bool one_tile = true;
                for (auto& jb : fcm[k].jobs) {
                    max_tiles = std::max(max_tiles, (jb.nout + SDRPP_FCM_TILE - 1) / SDRPP_FCM_TILE);
                    one_tile = one_tile && jb.tiles_per_wave == 1;
                }
                const int small_limit = c->fcm16_max_tiles >= 0 ? c->fcm16_max_tiles : ((ticking && c->plan_block_from_host) ? 0 : 256);
                if (role == TR_FCM_132_4 && one_tile && max_tiles > 0 && max_tiles <= small_limit) {
                    if (getenv("SDRPP_TICK_DEBUG")) { fprintf(stderr, "[sdrpp] front end in its small-block shape: %d tiles x %zu jobs\n", max_tiles, fcm[k].jobs.size()); }
                    emit(c, L0 + 1, F_S1, TR_FCM16_132_4, max_tiles, (int)fcm[k].jobs.size(), (size_t)frontcm16_layout(132, 4).total * 4, d_fcm[k], &src);
                    continue;
                }
                emit(c, L0 + 1, F_S1, role, fcm[k].max_blocks, (int)fcm[k].jobs.size(), fcm[k].lds, d_fcm[k], &src);
            }
            if (!fcl.jobs.empty() && fcl.max_blocks > 0) {
                bool pf_ok = true;  // every window of the launch fits the register prefetch
                for (auto& jb : fcl.jobs) { pf_ok = pf_ok && (SDRPP_FCM_TILE - 1) * (1 << jb.log2_decim) + jb.ntaps <= 64 * SDRPP_FCL_PF; }
                emit(c, L0 + 1, F_S1, pf_ok ? TR_FCL_PF : TR_FCL_0, fcl.max_blocks, (int)fcl.jobs.size(), fcl.lds, d_fcl, &src, fcl_nw);
            }
            if (!rot.empty() && max_rot > 0) { emit(c, L0 + 1, F_S1, TR_ROT, std::min((max_rot + 255) / 256, 4096), (int)rot.size(), 0, d_rot, &src); }
            if (!retune.empty()) {
                int mx = 0;
                for (auto& r : retune) { mx = std::max(mx, r.nfix); }
                launch(c, vfo_retune_fix_kernel, dim3((unsigned)mx, (unsigned)retune.size()), dim3(64), 0, src, (const RetuneJob*)d_retune);
            }
        }
        return SDRPP_OK;
    }

    int launch_fir(int level, int fam, std::vector<FirBJob>& jobs, FirBJob* d_jobs, int width, bool stereo, bool quad = false) {
            if (jobs.empty()) { return SDRPP_OK; }
            const int R = SDRPP_FIR_R;
            int max_nout = 0, threads = 256;
            auto lds_for = [&](const FirBJob& jb, int nt) {
                size_t b = (size_t)(1 << jb.log2_decim) * R * (size_t)(nt + jb.kp_pad / R + 1) * width * 4;
                if (quad) { b += ((size_t)nt * R + jb.ntaps + 2) * 4; }  // phase scratch of the fused discriminator
                return b;
            };
            for (auto& jb : jobs) {
                max_nout = std::max(max_nout, jb.nout);
                int nt = 256;
                // (a role of a tick: every workgroup of the launch gets the largest role's LDS — stay near the other roles' ~40 KB where the filter allows)
                while (ticking && nt > 64 && lds_for(jb, nt) > (size_t)c->tick_lds_cap_fir) { nt >>= 1; }
                while (nt >= 32 && lds_for(jb, nt) > (size_t)kMaxLds) { nt >>= 1; }
                if (nt < 32) {
                    if (width != 2 || quad || stereo) { return fail(c, SDRPP_ERR_UNSUPPORTED, "FIR (decim %d, %d taps) does not fit in LDS", 1 << jb.log2_decim, jb.ntaps); }
                    threads = 0;  // complex stream: the untiled kernel takes the whole list
                    break;
                }
                threads = std::min(threads, nt);
            }
            if (threads == 0) {
                for (auto& jb : jobs) { max_nout = std::max(max_nout, jb.nout); }
                if (max_nout > 0) {
                    if (ticking) { emit(c, level, fam, TR_FIRD, std::min((max_nout + 255) / 256, 1024), (int)jobs.size(), 0, d_jobs); }
                    else {
                        count_form(c, TR_FIRD);
                        launch(c, vfo_fir_direct_kernel<false>, dim3((unsigned)std::min((max_nout + 255) / 256, 1024), (unsigned)jobs.size()), dim3(256), 0, (const FirBJob*)d_jobs);
                    }
                }
                return SDRPP_OK;
            }
            if (max_nout == 0) { return SDRPP_OK; }
            // enough blocks to load-balance 256 CUs: shrink the tile while the grid has fewer than ~8 blocks per CU
            // (also as a role of a tick: a wider tile — fewer, longer workgroups in a tick that holds the long first stages' LDS anyway — measured neutral, profiles/r05zk)
            while (threads > 64 && (size_t)((max_nout + threads * R - 1) / (threads * R)) * jobs.size() < 2048) { threads >>= 1; }
            size_t lds = 0;
            for (auto& jb : jobs) { lds = std::max(lds, lds_for(jb, threads)); }
            const int tile = threads * R;
            emit(c, level, fam, width == 2 ? TR_FIRB_C : (quad ? TR_FIRB_Q : (stereo ? TR_FIRB_S : TR_FIRB_R)), (max_nout + tile - 1) / tile, (int)jobs.size(), lds, d_jobs, nullptr, threads);
            return SDRPP_OK;
    }
    // resamplers with many phases (L > 8, e.g. 96/125): cycle-major kernel — one LDS window serves all L phases of up to 64 cycles;
    // a filter whose single cycle does not fit falls back to the per-output kernel
    int launch_polyc(int level, int fam, std::vector<PolyJob>& jobs, PolyJob* d_jobs) {
            if (jobs.empty()) { return SDRPP_OK; }
            // LDS window of a tile: all 64 KB for a launch of its own (64 cycles per tile); as a role of a tick — whose workgroups all get the
            // largest role's LDS — about 24 KB (e.g. 19 cycles of the 96 / 125 resampler) unless a single cycle needs more
            int cap2 = kMaxLds / (int)sizeof(float2);
            if (ticking) {
                int need = c->tick_lds_cap / (int)sizeof(float2);
                for (auto& jb : jobs) { need = std::max(need, jb.tpp + 2 * jb.decim + 1); }
                cap2 = std::min(cap2, need);
            }
            bool fits = true;
            int max_nout = 0, max_tiles = 0;
            for (auto& jb : jobs) {
                max_nout = std::max(max_nout, jb.nout);
                const int ct = std::min(64, (cap2 - jb.tpp - jb.decim) / jb.decim);
                if (ct < 1) { fits = false; continue; }
                const int ncyc = (jb.nout + jb.interp - 1) / jb.interp;
                max_tiles = std::max(max_tiles, (ncyc + ct - 1) / ct);
            }
            if (max_nout == 0) { return SDRPP_OK; }
            if (fits) {
                // phase groups (a tick: always — a role's workgroup life is what the tick waits for): two phases per wavefront when the launch is a
                // handful of tiles (sr/200 blocks: 13 us -> 9 us of workgroup life, 767 -> 2 081 MS/s with the AF chain on 32 VFOs), six when there are
                // many (every group loads the tile's whole window again: 1 152 workgroups of 13.5 us were a third of a 10^6-sample tick's slot time)
                const int ppw = (long long)max_tiles * (long long)jobs.size() >= 64 ? 6 : 2;
                int G = 1;
                for (auto& jb : jobs) { G = std::max(G, ((jb.interp + 3) / 4 + ppw - 1) / ppw); }
                if (!ticking && (long long)max_tiles * (long long)jobs.size() >= 1024) { G = 1; }
                G = std::max(1, std::min(G, 128));
                emit(c, level, fam, TR_POLYC, max_tiles * G, (int)jobs.size(), (size_t)cap2 * sizeof(float2), d_jobs, nullptr, cap2 | ((G - 1) << 24));
                return SDRPP_OK;
            }
            size_t lds = 0;
            const int tile = 256;
            for (auto& jb : jobs) {
                const size_t ns = (size_t)((long long)tile * jb.decim / jb.interp) + jb.tpp + 4;
                lds = std::max(lds, ns * sizeof(float2));
            }
            if (lds > (size_t)kMaxLds) { return fail(c, SDRPP_ERR_UNSUPPORTED, "polyphase tile does not fit in LDS"); }
            if (ticking) { emit(c, level, fam, TR_POLY, (max_nout + tile - 1) / tile, (int)jobs.size(), lds, d_jobs); }
            else {
                count_form(c, TR_POLY);
                launch(c, vfo_poly_kernel, dim3((max_nout + tile - 1) / tile, (unsigned)jobs.size()), dim3(tile), lds, (const PolyJob*)d_jobs);
            }
            return SDRPP_OK;
    }
    int launch_polyb(int li, std::vector<PolyBJob>& jobs, PolyBJob* d_jobs) {
            if (jobs.empty()) { return SDRPP_OK; }
            int max_cycles = 0, threads = 256;
            size_t lds = 0;
            auto lds_for = [&](const PolyBJob& jb, int nt) { return (size_t)jb.decim * (size_t)(nt + jb.rows / jb.decim + 2) * sizeof(float2); };
            for (auto& jb : jobs) {
                max_cycles = std::max(max_cycles, (jb.nout + jb.interp - 1) / jb.interp);
                int nt = 256;
                while (nt >= 32 && lds_for(jb, nt) > (size_t)kMaxLds) { nt >>= 1; }
                if (nt < 32) { return fail(c, SDRPP_ERR_UNSUPPORTED, "polyphase tile does not fit in LDS"); }
                threads = std::min(threads, nt);
            }
            if (max_cycles == 0) { return SDRPP_OK; }
            while (threads > 64 && (size_t)((max_cycles + threads - 1) / threads) * jobs.size() < 2048) { threads >>= 1; }
            for (auto& jb : jobs) { lds = std::max(lds, lds_for(jb, threads)); }
            const dim3 grid((max_cycles + threads - 1) / threads, (unsigned)jobs.size());
            count_form(c, PF_POLYB_4 + li);
            if (li == 0) { launch(c, vfo_polyb_kernel<4, false>, grid, dim3(threads), lds, (const PolyBJob*)d_jobs); }
            else if (li == 1) { launch(c, vfo_polyb_kernel<8, false>, grid, dim3(threads), lds, (const PolyBJob*)d_jobs); }
            else if (li == 2) { launch(c, vfo_polyb_kernel<4, true>, grid, dim3(threads), lds, (const PolyBJob*)d_jobs); }
            else { launch(c, vfo_polyb_kernel<8, true>, grid, dim3(threads), lds, (const PolyBJob*)d_jobs); }
            return SDRPP_OK;
    }
    void emit_toep(int i, int l) {
            Lev<ToepJob>& L = *tlists[i].L;
            if (l >= L.top || L.at[l].empty() || tplan[i][l].grid_x == 0) { return; }
            emit(c, l, tlists[i].fam, tlists[i].role, tplan[i][l].grid_x, (int)L.at[l].size(), tplan[i][l].lds, L.dev[l]);
    }
    // the history carries of one level: job 0 of the IQ stream's level is the shared IQ stream (up to a whole FFT frame long), the per-VFO
    // histories are a few hundred samples
    void launch_carry(int l) {
            std::vector<CarryJob>& cj = carry.at[l];
            if (cj.empty()) { return; }
            const bool has_iq = (l == (ticking ? L0 + 1 : carry_last));
            const int iq_elems = has_iq ? cj[0].need * cj[0].width : 0;
            int mx = 0;
            for (size_t k = has_iq ? 1 : 0; k < cj.size(); k++) { mx = std::max(mx, cj[k].need * cj[k].width); }
            // (carry_body moves 4 floats per access and up to 8 accesses per work-item: 8 192 floats per workgroup and round, 2 048 per wavefront)
            // The per-VFO histories, a few hundred samples each: one WAVEFRONT per job, four jobs per workgroup (carry_body, njw > 0) unless a
            // history is long enough to want a workgroup's worth of loads in flight; the shared IQ history: an entry of its own.
            auto per_vfo = [&](const CarryJob* dev, int njobs) {
                if (njobs <= 0) { return; }
                if (mx <= carry_wave_max) { emit(c, l, F_MISC, TR_CARRY, 1, (njobs + 3) / 4, 0, dev, nullptr, njobs); }
                else { emit(c, l, F_MISC, TR_CARRY, std::max(1, std::min((mx + 8191) / 8192, 64)), njobs, 0, dev); }
            };
            if (!ticking && iq_elems > carry_wave_max && iq_elems <= 128 * 1024 * 2 && cj.size() > 1) {
                // an ordinary pass: one launch for the IQ history (up to a 65 536-point frame: 32 workgroups stride over it) and the per-VFO histories
                // (their workgroups beyond the first find nothing to do) — a kernel and its dispatch bubble less per push
                emit(c, l, F_MISC, TR_CARRY, 32, (int)cj.size(), 0, carry.dev[l]);
            }
            else if (has_iq && (iq_elems > carry_wave_max || cj.size() == 1)) {
                emit(c, l, F_MISC, TR_CARRY, std::max(1, std::min((iq_elems + 8191) / 8192, 512)), 1, 0, carry.dev[l]);
                per_vfo(carry.dev[l] + 1, (int)cj.size() - 1);
            }
            else {  // (no IQ history at this level, or one as short as the others)
                mx = std::max(mx, iq_elems);
                per_vfo(carry.dev[l], (int)cj.size());
            }
    }

    // ---- levels 2 ...: everything behind the front end, level by level (within a level the launches are independent of each other) ----
    int emit_levels() {
        int rc = SDRPP_OK;
        int top = d_pipes ? pipe_lvl + 1 : 0;
        for_each_list([&](auto& L) { top = std::max(top, L.top); });
        for (int l = 1; l < top; l++) {
            {
                FamilyTimer t(c, F_DECIM);
                emit_toep(0, l);
                if (l < f_dec.top) {
                    rc = launch_fir(l, F_DECIM, f_dec.at[l], f_dec.dev[l], 2, false);
                    if (rc) { return rc; }
                }
            }
            if (d_pipes && l == pipe_lvl) {
                FamilyTimer t(c, F_PIPE);
                c->pipe_launched = true;
                emit(c, l, F_PIPE, TR_PIPE, pipe_seg, (int)pipes.size(), pipe_lds, d_pipes);
            }
            {
                FamilyTimer t(c, F_POLY);
                emit_toep(1, l);
                if (l < poly.top) {
                    rc = launch_polyc(l, F_POLY, poly.at[l], poly.dev[l]);
                    if (rc) { return rc; }
                }
                for (int li = 0; li < 4; li++) {
                    if (l < polyb[li].top) {
                        rc = launch_polyb(li, polyb[li].at[l], polyb[li].dev[l]);
                        if (rc) { return rc; }
                    }
                }
            }
            {
                FamilyTimer t(c, F_FIR);
                emit_toep(2, l);
                if (l < chan.top) {
                    rc = launch_fir(l, F_FIR, chan.at[l], chan.dev[l], 2, false);
                    if (rc) { return rc; }
                }
            }
            if (l < wave.top && !wave.at[l].empty()) {
                FamilyTimer t(c, F_DEMOD);
                const int nj = (int)wave.at[l].size();
                emit(c, l, F_DEMOD, TR_IFC, (nj + 3) / 4, 1, wave_lds, wave.dev[l], nullptr, nj);
            }
            if ((l < pre.top && !pre.at[l].empty()) || (l < seq.top && !seq.at[l].empty()) || (l < ssbx_l.top && !ssbx_l.at[l].empty())) {
                FamilyTimer t(c, F_DEMOD);
                if (l < ssbx_l.top && !ssbx_l.at[l].empty()) {
                    const int nj = (int)ssbx_l.at[l].size();
                    if (ticking) { emit(c, l, F_DEMOD, TR_SSBX, (nj + 3) / 4, 1, 0, ssbx_l.dev[l], nullptr, nj); }
                    else {
                        count_form(c, TR_SSBX);
                        launch(c, vfo_ssb_rotate_exact_kernel, dim3((unsigned)nj), dim3(64), 0, (const SsbRotXJob*)ssbx_l.dev[l]);
                    }
                }
                if (l < pre.top && !pre.at[l].empty()) {
                    int mx = 0;
                    for (auto& q : pre.at[l]) { mx = std::max(mx, q.n); }
                    if (mx > 0) { emit(c, l, F_DEMOD, TR_PRE, std::min((mx + 255) / 256, 1024), (int)pre.at[l].size(), 0, pre.dev[l]); }
                }
                if (l < seq.top && !seq.at[l].empty()) { emit(c, l, F_DEMOD, TR_SEQ, (int)seq.at[l].size(), 1, 0, seq.dev[l], nullptr, (int)seq.at[l].size()); }
            }
            {
                FamilyTimer t(c, F_FIR);
                emit_toep(3, l);
                emit_toep(4, l);
                if (l < audio.top) {
                    rc = launch_fir(l, F_FIR, audio.at[l], audio.dev[l], 1, true);
                    if (rc) { return rc; }
                }
                if (l < audio_fm.top) {
                    rc = launch_fir(l, F_FIR, audio_fm.at[l], audio_fm.dev[l], 1, true, true);
                    if (rc) { return rc; }
                }
            }
            if (l < std::max({ t_af_dec.top, t_af_poly.top, t_af_hpf.top, af_dec.top, af_hpf.top, af_poly.top, af_deemp.top })) {
                FamilyTimer t(c, F_AF);
                emit_toep(5, l);
                if (l < af_dec.top) {
                    rc = launch_fir(l, F_AF, af_dec.at[l], af_dec.dev[l], 2, false);
                    if (rc) { return rc; }
                }
                emit_toep(6, l);
                if (l < af_poly.top) {
                    rc = launch_polyc(l, F_AF, af_poly.at[l], af_poly.dev[l]);
                    if (rc) { return rc; }
                }
                emit_toep(7, l);
                if (l < af_hpf.top) {
                    rc = launch_fir(l, F_AF, af_hpf.at[l], af_hpf.dev[l], 2, false);
                    if (rc) { return rc; }
                }
                if (l < af_deemp.top && !af_deemp.at[l].empty()) {
                    int max_seg = 0;
                    for (auto& jb : af_deemp.at[l]) { max_seg = std::max(max_seg, jb.nseg); }
                    if (max_seg > 0) {  // segment maps at this level, the outputs (and the state the next block starts from) one level later
                        emit(c, l, F_AF, TR_DEEMP_P0, max_seg, (int)af_deemp.at[l].size(), 3 * 256 * sizeof(float), af_deemp.dev[l]);
                        emit(c, l + 1, F_AF, TR_DEEMP_P1, max_seg, (int)af_deemp.at[l].size(), 3 * 256 * sizeof(float), af_deemp.dev[l]);
                    }
                }
            }
            if (l < carry.top && !carry.at[l].empty()) {
                FamilyTimer t(c, F_MISC);
                launch_carry(l);
            }
        }
        return SDRPP_OK;
    }
};

int do_vfos_plan(sdrpp_ctx* c, const IqSrc& src, int64_t count, const CarryJob& iq_carry) {
    if (c->vfos.empty()) { return SDRPP_OK; }
#ifdef SDRPP_TOEP_KNOCK
    {   // diagnostic build: SDRPP_TOEP_KNOCK=<mask> (1: no stores, 2: no loads, 4: no matrix loop) in vfo_toep_kernel
        static bool once = false;
        if (!once) {
            once = true;
            const int m = getenv("SDRPP_TOEP_KNOCK") ? atoi(getenv("SDRPP_TOEP_KNOCK")) : 0;
            (void)hipMemcpyToSymbol(HIP_SYMBOL(sdrpp_k::g_toep_knock), &m, sizeof(int));
        }
    }
#endif
    HostScope hs_all("plan: vfo bank");
    if (!c->bank_plan) {
        c->bank_plan = new BankPlan(c);
        c->bank_plan_free = [](void* q) { delete static_cast<BankPlan*>(q); };
    }
    BankPlan* P = static_cast<BankPlan*>(c->bank_plan);
    P->begin(src, count, iq_carry);
    int rc = SDRPP_OK;
    {
        HostScope hs("plan: chains");
        for (size_t i = 0; i < c->vfo_list.size(); i++) {
            rc = P->chain(*c->vfo_list[i]);
            if (rc) { return rc; }
        }
    }
    {
        HostScope hs("plan: group_front");
        rc = P->group_front();
    }
    if (!rc) {
        HostScope hs("plan: upload");
        rc = P->upload();
    }
    if (!rc) {
        HostScope hs("plan: emit");
        rc = P->emit_front();
        if (!rc) { rc = P->emit_levels(); }
    }
    if (rc) { return rc; }
    // flip the ping-pong side of every carried stream
    for (Vfo* v : c->vfo_list) {
        for_each_stream_that_ran(*v, [](Stream& s) {
            if (s.hist_len > 0 && s.data) { s.cur ^= 1; }
        });
    }
    return SDRPP_OK;
}

}  // namespace
