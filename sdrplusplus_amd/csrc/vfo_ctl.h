// The per-VFO control surface behind the C-ABI: lookup, which stream is what, building / re-planning / replacing a VFO with the reference's hand-overs,
// its IF and AF chains, read-out.  The extern "C" entry points in sdrpp_gpu.hip check their arguments, flush, look the VFO up and call one of these.
// Part of the one translation unit sdrpp_gpu.hip (included there, in order; not a stand-alone header).
#pragma once

namespace {

// The VFO behind a caller's id; nullptr for an id the context does not know, with the message of SDRPP_ERR_NOT_FOUND set (LOOKUP_VFO returns the code).
Vfo* vfo_lookup(sdrpp_ctx* c, int id) {
    auto it = c->vfos.find(id);
    if (it != c->vfos.end()) { return it->second.get(); }
    fail(c, SDRPP_ERR_NOT_FOUND, "no VFO %d", id);
    return nullptr;
}

// ---- which stream is what -----------------------------------------------------------------------------------------------------------
// The stream the channel filter reads: the resampler's output, else the last decimator stage's (stream 0 of a VFO without stages).
Stream& chan_feed(Vfo& v) { return v.st[(size_t)((v.i_poly >= 0) ? v.i_poly : v.i_first + std::max(v.rate.n_stages, 1) - 1)]; }
// RxVFO::out as the VFO is configured NOW: the channel filter's output, or its input while the filter is bypassed (st[i_if]: where the last push's lies).
Stream& rx_out(Vfo& v) { return (v.chan_ntaps > 0 && v.i_chan >= 0) ? v.st[(size_t)v.i_chan] : chan_feed(v); }
// What a read-out call names with `which` (sdrpp_vfo_read_many / _read_pcm / _read_compressed); nullptr: the VFO has no such stream.
//   0: what the VFO delivers — the demodulator's output; a RAW VFO's IF stream, behind an active IF chain the chain's output
//   1: the IF stream in front of the IF chain      2: the AF chain's output      3: the IF chain's output (a chain with a block switched on)
Stream* delivered(Vfo& v, int which) {
    Stream* ifc = (v.ifc.active() && v.i_ifc >= 0 && v.st[(size_t)v.i_ifc].base) ? &v.st[(size_t)v.i_ifc] : nullptr;
    switch (which) {
    case 0: return (v.d.demod != SDRPP_DEMOD_RAW) ? &v.st[(size_t)v.i_out] : (ifc ? ifc : &v.st[(size_t)v.i_if]);
    case 1: return &v.st[(size_t)v.i_if];
    case 2: return (v.af.on && v.af.i_last >= 0) ? &v.st[(size_t)v.af.i_last] : nullptr;
    case 3: return ifc;
    default: return nullptr;
    }
}
// The stream the demodulator reads: the IF chain's output while a chain is active, else RxVFO::out.
Stream& demod_feed(Vfo& v) { return delivered(v, 3) ? *delivered(v, 3) : rx_out(v); }
// How much of its input the demodulator remembers: the fused discriminator + audio FIR re-reads the IF history.
// (and the RDS branch's fused first stage recomputes its delay line from it: the stage's K0 - 1 samples and the one in front of them)
int demod_if_need(const Vfo& v) {
    const int fm = (v.d.demod == SDRPP_DEMOD_WFM || v.d.demod == SDRPP_DEMOD_NFM) ? std::max(v.audio_ntaps, 1) + 1 : 1;
    const int rds = (v.rds.attached && !v.rds.exact) ? std::max(fm, v.rds.rate.ntaps(0)) : fm;
    return v.stereo.attached ? std::max(rds, v.stereo.K) : rds;  // (the stereo branch's pilot job recomputes its window of discriminator values from it)
}

// ---- delay-line hand-overs ----------------------------------------------------------------------------------------------------------
// the newest min(both histories, max_samples) samples of `from`'s history become the newest of `to`'s
int hist_tail_copy(sdrpp_ctx* c, Stream& to, const Stream& from, int max_samples) {
    if (!to.hist[to.cur] || !from.hist[from.cur] || to.width != from.width) { return SDRPP_OK; }
    const int H = std::min(std::min(from.hist_len, to.hist_len), max_samples);
    if (H <= 0) { return SDRPP_OK; }
    const size_t w = (size_t)to.width;
    HIPCHK(c, hipMemcpy(to.hist[to.cur] + (size_t)(to.hist_len - H) * w, from.hist[from.cur] + (size_t)(from.hist_len - H) * w, (size_t)H * w * sizeof(float), hipMemcpyDeviceToDevice));
    return SDRPP_OK;
}
// The delay line of a FIR of `ntaps` taps that reads stream `s`: exactly the newest ntaps - 1 samples it was fed, whatever the stream's longer history holds
// in front of them (a one-tap filter has no delay line: nothing; a stream without history yet: zeros, which is what FIR's cleared buffer holds, fir.h:24-26).
int fir_line_save(sdrpp_ctx* c, const Stream& s, int ntaps, std::vector<float>& line) {
    const size_t w = (size_t)s.width;
    line.assign((size_t)std::max(ntaps - 1, 0) * w, 0.0f);
    if (ntaps > 1 && s.hist[s.cur] && s.hist_len >= ntaps - 1) {
        HIPCHK(c, hipMemcpy(line.data(), s.hist[s.cur] + (size_t)(s.hist_len - (ntaps - 1)) * w, line.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    return SDRPP_OK;
}
// FIR::setTaps (dsp/filter/fir.h:31-52) on a filter that held `line` and has `ntaps` taps from now on: the newest min(old, new) - 1 samples stay,
// zeros in front of them (all zeros for a filter that never ran).
int fir_line_restore(sdrpp_ctx* c, Stream& s, int ntaps, const std::vector<float>& line) {
    if (!s.hist[s.cur]) { return SDRPP_OK; }
    const size_t w = (size_t)s.width;
    HIPCHK(c, hipMemset(s.hist[s.cur], 0, (size_t)s.hist_len * w * sizeof(float)));
    const int have = (int)(line.size() / w), m = std::min(have, std::min(ntaps - 1, s.hist_len));
    if (m > 0) { HIPCHK(c, hipMemcpy(s.hist[s.cur] + (size_t)(s.hist_len - m) * w, line.data() + (size_t)(have - m) * w, (size_t)m * w * sizeof(float), hipMemcpyHostToDevice)); }
    return SDRPP_OK;
}

// ---- building a VFO -----------------------------------------------------------------------------------------------------------------
// sdrpp_vfo_add behind its argument check and flush: validates the description, builds the VFO and hands it to the context
int vfo_build(sdrpp_ctx* c, const sdrpp_vfo_desc* d, int* id) {
    const RateDesc rd = rate_desc(*d);
    if (int rc = rate_check_stages(c, rd, "")) { return rc; }
    if (d->n_stages > 0) {  // the fused translation + FIR kernel uses the linear-phase pairing (all reference plans are symmetric)
        const float* h = d->stage_taps[0];
        for (int k = 0; k < d->stage_ntaps[0] / 2; k++) {
            if (h[k] != h[d->stage_ntaps[0] - 1 - k]) { return fail(c, SDRPP_ERR_UNSUPPORTED, "first decimation stage must have symmetric (linear-phase) taps"); }
        }
    }
    if (int rc = rate_check_poly(c, rd, "")) { return rc; }
    if (d->chan_ntaps < 0 || d->chan_ntaps > kChanMaxTaps) { return fail(c, SDRPP_ERR_UNSUPPORTED, "channel filter of %d taps (max %d)", d->chan_ntaps, kChanMaxTaps); }
    if (d->demod < SDRPP_DEMOD_RAW || d->demod > SDRPP_DEMOD_CW) { return fail(c, SDRPP_ERR_INVALID, "demod %d", d->demod); }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // every early return below gives the device allocations made so far back (vfo_free); only a fully built VFO is handed to the context
    struct VfoFreer {
        void operator()(Vfo* p) const {
            if (p) {
                vfo_free(*p);
                delete p;
            }
        }
    };
    std::unique_ptr<Vfo, VfoFreer> v(new Vfo);
    v->id = c->next_id++;
    v->d = *d;
    for (int s = 0; s < SDRPP_MAX_DECIM_STAGES; s++) { v->d.stage_taps[s] = nullptr; }  // (the caller's arrays: `rate` has its own copies)
    v->d.resamp_taps = nullptr;
    RateChain& R = v->rate;
    rate_describe(R, rd);
    if (d->nco_mode < 0 || d->nco_mode > 2) { return fail(c, SDRPP_ERR_INVALID, "nco_mode %d: 0 (context), 1 (closed form) or 2 (reference rotator)", d->nco_mode); }
    v->nco_exact = d->nco_mode == 0 ? (c->nco_exact != 0) : (d->nco_mode == 2);
    int rc;
    // capacities
    size_t cap = (size_t)c->max_push;
    auto add_stream = [&](int width, int hist, size_t capn) -> int {
        v->st.emplace_back();
        int r = stream_alloc(c, v->st.back(), width, hist, capn);
        return r ? -1 : (int)v->st.size() - 1;
    };
    const bool fm = (d->demod == SDRPP_DEMOD_WFM || d->demod == SDRPP_DEMOD_NFM);
    if (fm || d->demod == SDRPP_DEMOD_AM) { v->audio_ntaps = std::max(d->audio_ntaps, 1); }  // fm.h:165-168 loadDummyTaps: a single unit tap when the low-pass is off
    const int if_hist = demod_if_need(*v);
    const int chan_hist = ((std::max(std::max(d->chan_ntaps - 1, 1), if_hist) + 63) / 64) * 64;  // grown on demand by sdrpp_vfo_set_channel_taps
    // what consumes the decimator / rotator output: the polyphase stage, else the channel filter or the discriminator
    if (R.n_stages == 0) {
        if (add_stream(2, R.need(0, chan_hist), cap) < 0) { return SDRPP_ERR_NOMEM; }
    }
    // every stage in blocks (and, below, in natural order for the fused front kernel); stage 0 runs as a plain FIR only behind the reference rotator
    RateForm form;
    form.matrix = v->nco_exact ? ~0u : ~1u;
    std::vector<float> bank;
    if ((rc = rate_build(c, R, form, v->st, cap, chan_hist, &bank))) { return rc; }
    if (R.has_poly()) { v->i_poly = (int)v->st.size() - 1; }
    for (int s = 0; s < R.n_stages; s++) {
        if ((rc = upload(c, &v->d_staps_nat[s], R.staps[s].data(), R.staps[s].size()))) { return rc; }
    }
    v->i_first = 0;
    {   // the front end as one filter: fusion decision (geometry only), tap identity, composite taps for the retune hand-over
        unsigned long long hsh = 1469598103934665603ull;  // FNV-1a over the taps of stages 0 and 1
        for (int s = 0; s < std::min(R.n_stages, 2); s++) {
            for (float t : R.staps[s]) {
                unsigned u;
                memcpy(&u, &t, 4);
                hsh = (hsh ^ u) * 1099511628211ull;
            }
        }
        v->tap_hash = hsh;
        if (R.n_stages >= 2) {  // the composite forms pair taps k and K-1-k: stage 1 must be linear phase as well
            const std::vector<float>& h2 = R.staps[1];
            for (size_t k = 0; k < h2.size() / 2; k++) { v->no_fuse = v->no_fuse || (h2[k] != h2[h2.size() - 1 - k]); }
        }
        v->fused_front = !v->nco_exact && !v->no_fuse && R.n_stages >= 2 && front2_t2(R.ntaps(0), R.decim_s[0], R.ntaps(1), R.decim_s[1], 8) > 0;
        if (R.n_stages >= 1 && !v->nco_exact) {
            const int K0 = R.ntaps(0), D1 = R.decim_s[0], K2 = v->fused_front ? R.ntaps(1) : 1;
            const int K = K0 + (K2 - 1) * D1;
            std::vector<double> h12((size_t)K, 0.0);
            for (int k2 = 0; k2 < K2; k2++) {
                const double w2 = v->fused_front ? (double)R.staps[1][(size_t)k2] : 1.0;
                for (int k1 = 0; k1 < K0; k1++) { h12[(size_t)k2 * D1 + k1] += w2 * (double)R.staps[0][(size_t)k1]; }
            }
            std::vector<float> hf(h12.begin(), h12.end());
            rc = upload(c, &v->d_h12, hf.data(), hf.size());
            if (rc) { return rc; }
            v->h12_K = K;
            v->h12_lgD = ilog2(D1) + (v->fused_front ? ilog2(R.decim_s[1]) : 0);
        }
        if (v->nco_exact && R.n_stages >= 1) {  // reference-rotator mode: the rotated full-rate stream feeds stage 0
            // (behind the chain's streams on purpose: rate_build appends the stages' and the resampler's in one go, and i_rot is only ever an index)
            v->i_rot = add_stream(2, R.ntaps(0) - 1, (size_t)c->max_push);
            if (v->i_rot < 0) { return SDRPP_ERR_NOMEM; }
        }
    }
    if (R.has_poly() && R.interp <= 8) {  // register-blocked kernel: per carried phase, taps of one full phase cycle
        const int L = R.interp, M = R.decim, tpp = R.tpp, lmax = (L <= 4) ? 4 : 8, rows = tpp + M;
        std::vector<float> cyc((size_t)L * rows * lmax, 0.0f);
        for (int ph0 = 0; ph0 < L; ph0++) {
            for (int r = 0; r < L; r++) {
                const int A = ph0 + r * M, ph = A % L, o = A / L;
                for (int k = 0; k < tpp; k++) { cyc[((size_t)ph0 * rows + (size_t)(k + o)) * lmax + r] = bank[(size_t)ph * tpp + k]; }
            }
        }
        rc = upload(c, &v->d_cyc, cyc.data(), cyc.size());
        if (rc) { return rc; }
        v->cyc_rows = rows;
        v->cyc_lmax = lmax;
    }
    // channel-filter output stream always exists (taps may be enabled later); its consumer is the demodulator
    v->i_chan = add_stream(2, if_hist, cap);
    if (v->i_chan < 0) { return SDRPP_ERR_NOMEM; }
    if (d->chan_ntaps > 0) {
        if (!d->chan_taps) { return fail(c, SDRPP_ERR_INVALID, "chan_taps null"); }
        v->ctaps_chan.assign(d->chan_taps, d->chan_taps + d->chan_ntaps);
        rc = upload_blocked(c, &v->d_chan, v->ctaps_chan.data(), (int)v->ctaps_chan.size(), 1, &v->chan_kp);
        if (rc) { return rc; }
        rc = toep_build_fir(c, v->tp_chan, v->ctaps_chan.data(), (int)v->ctaps_chan.size(), 1);
        if (rc) { return rc; }
        v->chan_ntaps = d->chan_ntaps;
    }
    v->d.chan_taps = nullptr;
    // the IF chain's output (sdrpp_vfo_set_if, sdrpp_vfo_set_fmnr) and the stream between its blanker / squelch and FMIF: only the slots — their
    // buffers come with the first chain that needs them, a VFO without one pays nothing
    v->st.emplace_back();
    v->i_ifc = (int)v->st.size() - 1;
    v->st.emplace_back();
    v->i_fmi = (int)v->st.size() - 1;
    if (d->demod != SDRPP_DEMOD_RAW) {
        if (fm || d->demod == SDRPP_DEMOD_AM) {
            static const float unit = 1.0f;
            const float* at = d->audio_ntaps > 0 ? d->audio_taps : &unit;
            const int an = v->audio_ntaps;
            if (d->audio_ntaps > 0 && !d->audio_taps) { return fail(c, SDRPP_ERR_INVALID, "audio_taps null"); }
            v->ataps.assign(at, at + an);
            rc = upload_blocked(c, &v->d_audio, v->ataps.data(), (int)v->ataps.size(), 1, &v->audio_kp);
            if (rc) { return rc; }
            rc = toep_build_fir(c, v->tp_audio, v->ataps.data(), (int)v->ataps.size(), 1);
            if (rc) { return rc; }
            if (!fm) {  // AM: the sequential envelope/AGC kernel writes a real stream for the low-pass; FM demodulates inside the FIR kernel
                v->i_dem = add_stream(1, std::max(an - 1, 1), cap);
                if (v->i_dem < 0) { return SDRPP_ERR_NOMEM; }
            }
        }
        if (d->demod >= SDRPP_DEMOD_USB) {  // SSB family (CW is SSB with the tone as its translation): real scratch between the parallel translation and the sequential AGC
            v->i_dem = add_stream(1, 0, cap);
            if (v->i_dem < 0) { return SDRPP_ERR_NOMEM; }
        }
        v->i_out = add_stream(2, 0, cap);
        if (v->i_out < 0) { return SDRPP_ERR_NOMEM; }
    }
    v->d.audio_taps = nullptr;
    rc = dev_alloc(c, &v->d_state, 2 * sizeof(AgcState) + sizeof(float));
    if (rc) { return rc; }
    rc = dev_alloc(c, &v->d_rot, 2);
    if (rc) { return rc; }
    v->theta = sdrpp_host::turnsPerSample(d->phase_delta_re, d->phase_delta_im);
    v->theta2 = sdrpp_host::turnsPerSample(d->ssb_phase_delta_re, d->ssb_phase_delta_im);
    if (d->demod < SDRPP_DEMOD_USB) { v->theta2 = 0.0; }
    v->modtaps_dirty = true;
    rc = vfo_reset_state(c, *v);
    if (rc) { return rc; }
    const int vid = v->id;  // (the right-hand side of the assignment below is evaluated first)
    *id = vid;
    c->vfos[vid] = std::unique_ptr<Vfo>(v.release());
    vfo_list_rebuild(c);
    return SDRPP_OK;
}

// ---- radio IF chain -----------------------------------------------------------------------------------------------------------------
// FMIF's delay line (fm_if.h: `buffer`, bins - 1 samples; kept here as the newest kFmifTile - 1, the matrix has zero columns for the rest) is the
// history of the stream FMIF reads: the blanker / squelch output st[i_fmi] while one of them runs, else RxVFO::out.  Which stream that is changes
// with every switch of the chain, and an unplugged FMIF keeps what it held (the reference only takes the block out of the chain).  So every call
// that changes the chain saves the line under the old configuration (fmif_line_save) and puts it back under the new one (fmif_line_restore);
// in between, and while FMIF is off, Vfo::Ifc::fm_line holds it.
Stream& fmif_feed(Vfo& v) { return (v.ifc.nbsq() && v.i_fmi >= 0) ? v.st[(size_t)v.i_fmi] : rx_out(v); }
int fmif_line_save(sdrpp_ctx* c, Vfo& v) {
    Vfo::Ifc& f = v.ifc;
    if (f.fm_line.empty()) { f.fm_line.assign((size_t)(kFmifTile - 1) * 2, 0.0f); }
    if (!f.fm_on) { return SDRPP_OK; }
    const Stream& s = fmif_feed(v);
    const int H = std::min(s.hist_len, kFmifTile - 1);
    std::fill(f.fm_line.begin(), f.fm_line.end(), 0.0f);
    if (H > 0 && s.hist[s.cur] && s.width == 2) {
        HIPCHK(c, hipMemcpy(f.fm_line.data() + (size_t)(kFmifTile - 1 - H) * 2, s.hist[s.cur] + (size_t)(s.hist_len - H) * 2, (size_t)H * 2 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return SDRPP_OK;
}
int fmif_line_restore(sdrpp_ctx* c, Vfo& v) {
    Vfo::Ifc& f = v.ifc;
    if (!f.fm_on) { return SDRPP_OK; }
    if (f.fm_line.empty()) { f.fm_line.assign((size_t)(kFmifTile - 1) * 2, 0.0f); }
    Stream& s = fmif_feed(v);
    int rc;
    if (!s.base) {  // (st[i_fmi], first use)
        if ((rc = stream_alloc(c, s, 2, kFmifTile - 1, v.st[(size_t)v.i_chan].cap))) { return rc; }
    }
    if ((rc = stream_grow_hist(c, s, kFmifTile - 1))) { return rc; }
    HIPCHK(c, hipMemcpy(s.hist[s.cur] + (size_t)(s.hist_len - (kFmifTile - 1)) * 2, f.fm_line.data(), f.fm_line.size() * sizeof(float), hipMemcpyHostToDevice));
    return SDRPP_OK;
}
// the IF chain's output stream, allocated with the first chain
int ifc_out_ensure(sdrpp_ctx* c, Vfo& v) {
    Stream& fs = v.st[(size_t)v.i_ifc];
    if (fs.base) { return SDRPP_OK; }
    const Stream& like = v.st[(size_t)v.i_chan];  // what the demodulator reads today: same capacity, same history
    return stream_alloc(c, fs, 2, like.hist_len, like.cap);
}
// sdrpp_vfo_set_if on a VFO the caller has looked up (the stream is idle).  What the demodulator remembers of its input (the discriminator's
// previous sample, the audio low-pass's delay line) moves with the switch: it was fed the IF until a chain becomes active and the chain's
// output from then on, or the other way round.
int ifc_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_if_desc* d) {
    Vfo::Ifc& f = v.ifc;
    if (v.i_ifc < 0) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no IF chain slot", v.id); }
    Stream& fs = v.st[(size_t)v.i_ifc];
    if (d) {  // (checked before anything changes)
        if (d->nb_enabled && !(d->nb_rate > 0.0f && d->nb_rate <= 1.0f && d->nb_level == d->nb_level)) { return fail(c, SDRPP_ERR_INVALID, "noise blanker: rate %g (0 < rate <= 1), level %g", d->nb_rate, d->nb_level); }
        if (d->squelch_enabled && d->squelch_level != d->squelch_level) { return fail(c, SDRPP_ERR_INVALID, "squelch level is not a number"); }
    }
    if (int rc = fmif_line_save(c, v)) { return rc; }  // FMIF is left alone: its delay line moves to whatever stream it reads from now on
    const bool was_active = f.active() && fs.base, was_nb = f.on && f.nb_on;
    if (d) {
        if (int rc = ifc_out_ensure(c, v)) { return rc; }
        if (!f.d_amp) {
            int rc = dev_alloc(c, &f.d_amp, 1);
            if (rc) { return rc; }
        }
        if (d->nb_enabled && !was_nb) {  // a blanker that starts: amp = 1 (noise_blanker.h:75); one that runs keeps it through setRate / setLevel
            const float one = 1.0f;
            HIPCHK(c, hipMemcpy(f.d_amp, &one, sizeof(float), hipMemcpyHostToDevice));
        }
        f.on = true;
        f.nb_on = d->nb_enabled != 0;
        f.nb_rate = d->nb_rate;
        f.nb_level = d->nb_level;
        f.sq_on = d->squelch_enabled != 0;
        f.sq_level = d->squelch_level;
    }
    else {
        f.on = false;
        f.nb_on = 0;
        f.sq_on = 0;
    }
    const bool now_active = f.active();
    if (was_active != now_active && fs.base) {
        Stream& feed = rx_out(v);
        const int if_need = demod_if_need(v);
        int rc = now_active ? hist_tail_copy(c, fs, feed, if_need) : hist_tail_copy(c, feed, fs, if_need);
        if (rc) { return rc; }
    }
    if (!now_active) { fs.n = 0; }
    return fmif_line_restore(c, v);
}

// sdrpp_vfo_set_fmnr on a VFO the caller has looked up (the stream is idle): FMIF::setBins clears the delay line (fm_if.h:26-34), unplugging the
// block keeps it, and what the demodulator remembers of its input moves when the chain as a whole starts or stops, as in ifc_apply.
int fmnr_apply(sdrpp_ctx* c, Vfo& v, bool enabled, int bins) {
    Vfo::Ifc& f = v.ifc;
    if (v.i_ifc < 0 || v.i_fmi < 0) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no IF chain slot", v.id); }
    Stream& fs = v.st[(size_t)v.i_ifc];
    int rc;
    if ((rc = fmif_line_save(c, v))) { return rc; }
    if (enabled) {
        if ((rc = ifc_out_ensure(c, v))) { return rc; }
        if (c->fmif_tabs.find(bins) == c->fmif_tabs.end()) {
            std::vector<float> tab((size_t)2 * 32 * 32);
            sdrpp_host::fmifMatrix(bins, tab.data());
            float* d_tab = nullptr;
            if ((rc = upload(c, &d_tab, tab.data(), tab.size()))) { return rc; }
            c->fmif_tabs[bins] = d_tab;
        }
    }
    const bool was_active = f.active() && fs.base;
    if (bins != f.fm_bins) { std::fill(f.fm_line.begin(), f.fm_line.end(), 0.0f); }
    f.fm_bins = bins;
    f.fm_on = enabled;
    const bool now_active = f.active();
    if (was_active != now_active && fs.base) {
        Stream& feed = rx_out(v);
        if ((rc = now_active ? hist_tail_copy(c, fs, feed, demod_if_need(v)) : hist_tail_copy(c, feed, fs, demod_if_need(v)))) { return rc; }
    }
    if (!now_active) { fs.n = 0; }
    return fmif_line_restore(c, v);
}

// ---- sdrpp_vfo_replace: what of the old VFO lives on in the new one -----------------------------------------------------------------
// RxVFO::setInSamplerate / setOutSamplerate (rx_vfo.h:35-58): the channeliser is re-planned, but not everything starts over.  The reference keeps
//   * the translation's phase (FrequencyXlator::setOffset only swaps phaseDelta, frequency_xlator.h:24-30) and
//   * the channel filter's delay line (setOutSamplerate: FIR::setTaps moves it under the new tap count, fir.h:31-52; setInSamplerate does not touch the
//     filter at all; a filter that is bypassed under the new settings keeps what it held, one that wakes up continues from that)          -> keep bit 0
// while its decimator stages are new objects and the polyphase resampler is reset (power_decimator.h:91-108, polyphase_resampler.h:38-67), and
//   * the demodulator behind it is a separate block that setInSamplerate leaves alone: discriminator / audio low-pass history, AGC and DC-blocker
//     states, SSB's second translation                                                                                                     -> keep bit 1
// (a demodulator SWITCH deletes and creates it, radio_module.h:419-563: bit 1 off).  The AF chain is re-attached by the caller and starts cleared.
int rds_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n);  // (the RDS branch: below, with the rest of it)
int stereo_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n, bool* cleared);  // (the stereo branch: likewise)
int sym_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n);  // (the symbol branch: likewise)
int rdsd_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n, size_t old_cap);  // (the RDS demodulator: likewise)
size_t rdsd_in_cap(const Vfo& v, int source);
int qpsk_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n);  // (the QPSK demodulator: likewise)
int vfo_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n, int keep) {
    Stream& of = chan_feed(o);
    Stream& nf = chan_feed(n);
    int rc;
    const size_t rdsd_cap = (o.rdsd.attached && (o.rdsd.source == 1 || o.rds.attached)) ? rdsd_in_cap(o, o.rdsd.source) : 0;  // (before the RDS branch moves)
    if (keep & 1) {
        if (o.nco_exact == n.nco_exact) {
            n.phi = o.phi;
            if (o.d_rot && n.d_rot) { HIPCHK(c, hipMemcpy(n.d_rot, o.d_rot, sizeof(float2), hipMemcpyDeviceToDevice)); }
        }
        // the channel filter's delay line as the reference's FIR object holds it now: the newest old_taps - 1 samples it was fed, or what it held
        // when it was last bypassed
        std::vector<float> line = o.chan_stale;
        if (o.chan_ntaps > 0 && (rc = fir_line_save(c, of, o.chan_ntaps, line))) { return rc; }
        if (n.chan_ntaps > 0 && nf.width == of.width) {
            if ((rc = fir_line_restore(c, nf, n.chan_ntaps, line))) { return rc; }
        }
        else if (n.chan_ntaps == 0) { n.chan_stale = line; }  // bypassed under the new settings: the filter object keeps what it held
    }
    if ((keep & 2) && o.d.demod == n.d.demod) {
        // the demodulator's view of the IF stream: the discriminator's previous sample and the audio low-pass's delay line are its newest samples
        // (behind an IF chain that is what the CHAIN delivered).  The stereo branch moves first: it decides how much of that view the new handle keeps
        bool st_cleared = false;
        if (n.d.demod == SDRPP_DEMOD_WFM && (rc = stereo_hand_over(c, o, n, &st_cleared))) { return rc; }
        if (!st_cleared) {
            rc = hist_tail_copy(c, demod_feed(n), demod_feed(o), demod_if_need(n));  // (the new VFO has no chain yet: its RxVFO::out)
            if (rc) { return rc; }
        }
        if (o.i_dem >= 0 && n.i_dem >= 0) {
            rc = hist_tail_copy(c, n.st[(size_t)n.i_dem], o.st[(size_t)o.i_dem], 1 << 30);
            if (rc) { return rc; }
        }
        if (o.d_state && n.d_state) {
            // the loops' states live on; their attack / decay are the NEW description's (AGC::setAttack / setDecay swap the coefficients only, agc.h:31-43)
            char blob[2 * sizeof(AgcState) + sizeof(float)];
            HIPCHK(c, hipMemcpy(blob, o.d_state, sizeof(blob), hipMemcpyDeviceToHost));
            AgcState st[2];
            memcpy(st, blob, sizeof(st));
            for (int i = 0; i < 2; i++) {
                st[i].attack = n.d.agc_attack;
                st[i].inv_attack = 1.0f - n.d.agc_attack;
                st[i].decay = n.d.agc_decay;
                st[i].inv_decay = 1.0f - n.d.agc_decay;
            }
            memcpy(blob, st, sizeof(st));
            HIPCHK(c, hipMemcpy(n.d_state, blob, sizeof(blob), hipMemcpyHostToDevice));
        }
        n.phi2 = o.phi2;
        if (o.d_rot && n.d_rot) { HIPCHK(c, hipMemcpy(n.d_rot + 1, o.d_rot + 1, sizeof(float2), hipMemcpyDeviceToDevice)); }
    }
    if ((keep & 4) && o.ifc.on) {
        // the radio's IF chain objects are not the demodulator's: they live through a demodulator switch (radio_module.h:84-96, 419-563), the
        // blanker with its amplitude estimate.  Attaching copies the demodulator's view of the IF (set above) into the chain's history.
        const sdrpp_if_desc fd{ o.ifc.nb_on, o.ifc.nb_rate, o.ifc.nb_level, o.ifc.sq_on, o.ifc.sq_level };
        rc = ifc_apply(c, n, &fd);
        if (rc) { return rc; }
        if (o.ifc.nb_on && o.ifc.d_amp && n.ifc.d_amp) { HIPCHK(c, hipMemcpy(n.ifc.d_amp, o.ifc.d_amp, sizeof(float), hipMemcpyDeviceToDevice)); }
    }
    if ((keep & 2) && o.d.demod == n.d.demod && n.d.demod == SDRPP_DEMOD_WFM) {
        if ((rc = rds_hand_over(c, o, n))) { return rc; }
    }
    if ((keep & 2) && o.d.demod == n.d.demod && n.d.demod == SDRPP_DEMOD_RAW) {
        if ((rc = sym_hand_over(c, o, n))) { return rc; }
    }
    if ((keep & 2) && o.d.demod == n.d.demod) {
        if ((rc = rdsd_hand_over(c, o, n, rdsd_cap))) { return rc; }
    }
    if ((keep & 2) && o.d.demod == n.d.demod && n.d.demod == SDRPP_DEMOD_RAW) {
        if ((rc = qpsk_hand_over(c, o, n))) { return rc; }
    }
    if (keep & 4) {  // ... and FMIF with them: its bin count, whether it is plugged in, and its delay line
        if ((rc = fmif_line_save(c, o))) { return rc; }
        n.ifc.fm_bins = o.ifc.fm_bins;
        n.ifc.fm_line = o.ifc.fm_line;
        if ((rc = fmnr_apply(c, n, o.ifc.fm_on, o.ifc.fm_bins))) { return rc; }
    }
    return SDRPP_OK;
}

// ---- sdrpp_vfo_set_channel_taps -----------------------------------------------------------------------------------------------------
int vfo_set_chan_taps(sdrpp_ctx* c, Vfo& v, const float* taps, int n) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = fmif_line_save(c, v)) { return rc; }  // (FMIF reads RxVFO::out, which changes its identity with the filter's bypass)
    Stream& fs = chan_feed(v);  // must remember n - 1 samples
    const int old_n = v.chan_ntaps, w = fs.width;
    const bool was_on = old_n > 0, now_on = n > 0;
    // ---- the filter's BYPASS switched (bandwidth == IF rate exactly, rx_vfo.h:60-70 / :89-100) ----
    // (a) The consumers behind the filter read "the IF stream" with memory (the demodulator's audio low-pass): their delay line holds the last
    //     samples they were FED — the filter's outputs until now, its input from now on, or the other way round.  The IF stream changes its
    //     identity here (st[i_chan] <-> the filter's input stream), so the newest history goes with it.
    // (b) The reference does not touch a bypassed filter: its delay line keeps what it held when it last ran, and a filter switched on again
    //     continues from that stale content (FIR::setTaps moves it like any other change of the tap count, fir.h:31-52).  The stream's side
    //     buffer here keeps being refreshed for consumer (a), so the filter's own last history is set aside when it goes to sleep and put
    //     back — under the new tap count — when it wakes up.
    if (was_on != now_on && v.i_chan >= 0) {
        Stream& cs = v.st[(size_t)v.i_chan];
        if (was_on) {  // going to sleep: (b) first, (a) overwrites the buffer
            if (int rc = fir_line_save(c, fs, old_n, v.chan_stale)) { return rc; }
        }
        if (now_on) {  // waking up: the buffer must be long enough for the new filter before anything is put into it
            int rc = stream_grow_hist(c, fs, n - 1);
            if (rc) { return rc; }
        }
        if (int rc = was_on ? hist_tail_copy(c, fs, cs, 1 << 30) : hist_tail_copy(c, cs, fs, 1 << 30)) { return rc; }  // (a)
        if (now_on) {  // (b): what the filter held when it last ran, under the new tap count
            if (int rc = fir_line_restore(c, fs, n, v.chan_stale)) { return rc; }
        }
    }
    else {
        int rc = stream_grow_hist(c, fs, n - 1);
        if (rc) { return rc; }
        // FIR::setTaps (dsp/filter/fir.h:31-52): a LONGER filter starts with zeros in front of the old delay line — its old_n - 1 samples are
        // all the reference kept, whatever the stream held before them.  The side buffer here holds the stream's true tail (newest last):
        // everything older than the old filter's reach is cleared.
        const int keep = std::max(old_n - 1, 0);
        if (n > old_n && fs.hist_len > keep && fs.hist[fs.cur]) {
            HIPCHK(c, hipMemset(fs.hist[fs.cur], 0, (size_t)(fs.hist_len - keep) * (size_t)w * sizeof(float)));
        }
    }
    v.ctaps_chan.assign(taps, taps + n);
    v.chan_ntaps = n;
    v.d.chan_ntaps = n;
    if (n > 0) {
        int rc = upload_blocked(c, &v.d_chan, v.ctaps_chan.data(), n, 1, &v.chan_kp);
        if (rc) { return rc; }
        rc = toep_build_fir(c, v.tp_chan, v.ctaps_chan.data(), n, 1);
        if (rc) { return rc; }
    }
    return fmif_line_restore(c, v);
}

// ---- radio AF chain -----------------------------------------------------------------------------------------------------------------
// sdrpp_vfo_set_af on a VFO the caller has looked up: the old chain goes, `af` (if any) is built behind st[i_out]
int af_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_af_desc* af) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    af_detach(v);
    if (!af) { return SDRPP_OK; }
    if (v.d.demod == SDRPP_DEMOD_RAW || v.i_out < 0) { return fail(c, SDRPP_ERR_UNSUPPORTED, "the AF chain needs a demodulating VFO"); }
    const RateDesc rd = rate_desc(*af);
    if (int rc = rate_check_stages(c, rd, "af ")) { return rc; }
    if (int rc = rate_check_poly(c, rd, "af ")) { return rc; }
    if (af->hpf_ntaps < 0 || (af->hpf_ntaps > 0 && !af->hpf_taps)) { return fail(c, SDRPP_ERR_INVALID, "bad af high-pass description"); }
    // (the high-pass's input stream gets its history from the tap count below, and a
    // filter too long for the matrix form and for an LDS tile of the register-blocked one runs untiled — highPass(300, 100) has 7 296 taps at 192 kHz)
    if (af->hpf_ntaps > kAfHpfMaxTaps) { return fail(c, SDRPP_ERR_UNSUPPORTED, "af high-pass of %d taps (max %d)", af->hpf_ntaps, kAfHpfMaxTaps); }
    Vfo::Af& a = v.af;
    RateChain& R = a.rate;
    rate_describe(R, rd);
    a.base = (int)v.st.size();
    a.alpha = af->deemph_alpha;
    int rc;
    const int tail = std::max(af->hpf_ntaps - 1, 0);  // behind the resampler: the high-pass (the de-emphasis needs no history)
    rc = stream_grow_hist(c, v.st[(size_t)v.i_out], R.need(0, tail));
    if (rc) { return rc; }
    size_t cap = v.st[(size_t)v.i_out].cap;
    auto add_stream = [&](int hist, size_t capn) -> int {
        v.st.emplace_back();
        int r = stream_alloc(c, v.st.back(), 2, hist, capn);
        return r ? -1 : (int)v.st.size() - 1;
    };
    if ((rc = rate_build(c, R, RateForm{}, v.st, cap, tail))) { return rc; }
    if (R.n_stages > 0) { a.i_stage0 = a.base; }
    if (R.has_poly()) { a.i_poly = a.base + R.n_stages; }
    if (af->hpf_ntaps > 0) {
        a.htaps.assign(af->hpf_taps, af->hpf_taps + af->hpf_ntaps);
        rc = upload_blocked(c, &a.d_hpf, a.htaps.data(), (int)a.htaps.size(), 1, &a.hpf_kp);
        if (rc) { return rc; }
        rc = toep_build_fir(c, a.tp_hpf, a.htaps.data(), (int)a.htaps.size(), 1);
        if (rc) { return rc; }
        a.i_hpf = add_stream(0, cap);
        if (a.i_hpf < 0) { return SDRPP_ERR_NOMEM; }
    }
    if (a.alpha != 0.0f) {
        rc = dev_alloc(c, &a.d_last, 2);
        if (rc) { return rc; }
        HIPCHK(c, hipMemset(a.d_last, 0, 2 * sizeof(float2)));
        a.state_cur = 0;
        a.seg_cap = (int)(cap / SDRPP_DEEMP_SEG) + 2;
        rc = dev_alloc(c, &a.d_seg, 2 * ((size_t)a.seg_cap + 1));
        if (rc) { return rc; }
        a.i_deemp = add_stream(0, cap);
        if (a.i_deemp < 0) { return SDRPP_ERR_NOMEM; }
    }
    a.i_last = v.i_out;
    a.on = true;
    return SDRPP_OK;
}

// ---- RDS branch of the WFM demodulator ----------------------------------------------------------------------------------------------
// FNV-1a over what makes a polyphase bank: identical descriptions share ONE device copy per context (5000 x 119 floats at 250 kS/s: 2.4 MB)
unsigned long long rds_bank_hash(int interp, int decim, const float* taps, int n) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](unsigned u) { h = (h ^ u) * 1099511628211ull; };
    mix((unsigned)interp);
    mix((unsigned)decim);
    mix((unsigned)n);
    for (int i = 0; i < n; i++) {
        unsigned u;
        memcpy(&u, &taps[i], 4);
        mix(u);
    }
    return h ? h : 1ull;
}
void rdsd_detach(sdrpp_ctx* c, Vfo& v);
void rds_detach(sdrpp_ctx* c, Vfo& v) {
    Vfo::Rds& r = v.rds;
    if (v.rdsd.attached && v.rdsd.source == 0) { rdsd_detach(c, v); }  // (a demodulator behind the branch goes with it)
    if (r.bank_key) {
        auto it = c->rds_banks.find(r.bank_key);
        if (it != c->rds_banks.end() && --it->second.refs <= 0) {
            dev_free(it->second.d_bank);
            c->rds_banks.erase(it);
        }
    }
    rds_free_own(r);
    r = Vfo::Rds{};
}
// The first decimator's delay line leaves the feed's history (the branch is switched off, or the history is about to be cleared or to move on without the
// branch): the discriminator values of its newest K0 samples are set aside (the oldest of them, which would need a sample more, lies outside the filter's reach),
// and the branch reads them in place of the history until it has been fed K0 samples in a row again.  A line that is in force already IS what the branch was
// fed last (short blocks are spliced onto it as they come): it stays, and only the count of samples fed in a row starts over.
int rds_freeze(sdrpp_ctx* c, Vfo& v) {
    Vfo::Rds& r = v.rds;
    if (!r.attached || !r.on || r.exact) { return SDRPP_OK; }
    r.line_fed = 0;
    if (r.frozen) { return SDRPP_OK; }
    const Stream& s = demod_feed(v);
    const int K0 = r.rate.ntaps(0);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float* line = r.d_line[r.line_cur];
    if (s.hist_len >= K0 && s.hist[s.cur]) {
        const float2* tail = reinterpret_cast<const float2*>(s.hist[s.cur]) + (s.hist_len - K0);
        hipLaunchKernelGGL(vfo_rds_line_kernel, dim3(1), dim3(64), 0, c->stream, RdsLineJob{ tail, tail, line, line, K0, K0, v.d.inv_deviation });
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    else { HIPCHK(c, hipMemset(line, 0, (size_t)K0 * sizeof(float))); }  // (never: rds_apply grows every stream the demodulator may read)
    r.frozen = true;
    return SDRPP_OK;
}
// The context's shared polyphase bank for a described chain (keyed by rds_bank_hash, one reference per branch): uploaded with its first user
int rds_bank_acquire(sdrpp_ctx* c, Vfo::Rds& r) {
    const RateChain& R = r.rate;
    const unsigned long long key = rds_bank_hash(R.interp, R.decim, R.rtaps.data(), (int)R.rtaps.size());
    auto it = c->rds_banks.find(key);
    if (it != c->rds_banks.end() && (it->second.interp != R.interp || it->second.tpp != R.tpp || it->second.taps != R.rtaps)) {
        return fail(c, SDRPP_ERR_UNSUPPORTED, "rds polyphase bank: two different descriptions under one key");  // (a 64-bit collision: never seen)
    }
    if (it == c->rds_banks.end()) {
        sdrpp_ctx::RdsBank B;
        const std::vector<float> bank = polyphase_bank(R.rtaps.data(), (int)R.rtaps.size(), R.interp, R.tpp);
        if (int rc = upload(c, &B.d_bank, bank.data(), bank.size())) { return rc; }
        B.interp = R.interp;
        B.tpp = R.tpp;
        B.taps = R.rtaps;
        it = c->rds_banks.emplace(key, std::move(B)).first;
    }
    it->second.refs++;
    r.bank_key = key;
    return SDRPP_OK;
}
// sdrpp_vfo_set_rds on a VFO the caller has looked up (the stream is idle); d == nullptr: the branch goes.  The NCO increment (pd_re, pd_im) travels beside
// the view and is part of the branch's identity: "the same branch" below means the same chain (rate_same) with the same increment in the same NCO mode.
int rds_apply(sdrpp_ctx* c, Vfo& v, const RateDesc* d, float pd_re, float pd_im, bool enabled) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d) {
        rds_detach(c, v);
        return SDRPP_OK;
    }
    if (v.d.demod != SDRPP_DEMOD_WFM) { return fail(c, SDRPP_ERR_UNSUPPORTED, "the RDS branch needs a WFM VFO"); }
    if (int rc = rate_check_stages(c, *d, "rds ")) { return rc; }
    if (int rc = rate_check_poly(c, *d, "rds ")) { return rc; }
    if (d->n_stages < 1 || d->stage_decim[0] < 2) { return fail(c, SDRPP_ERR_UNSUPPORTED, "the RDS branch's first stage must decimate"); }
    int tile = 0, pitch = 0;
    if (!v.nco_exact && !rds_tile_geometry(d->stage_ntaps[0], d->stage_decim[0], &tile, &pitch)) {
        return fail(c, SDRPP_ERR_UNSUPPORTED, "rds first stage (decimation %d, %d taps): no tile of its window fits the kernel's LDS", d->stage_decim[0], d->stage_ntaps[0]);
    }
    Vfo::Rds& r = v.rds;
    if (r.attached && r.exact == v.nco_exact && r.pd_re == pd_re && r.pd_im == pd_im && rate_same(r.rate, *d)) {  // the same branch: only the switch
        if (r.on && !enabled) {
            if (int rc = rds_freeze(c, v)) { return rc; }
            for (auto& s : r.st) { s.n = 0; }
        }
        r.on = enabled;
        r.ran = r.ran && enabled;
        return SDRPP_OK;
    }
    rds_detach(c, v);
    // every early return below gives back what was built so far
    struct Undo {
        sdrpp_ctx* c; Vfo& v; bool armed = true;
        ~Undo() { if (armed) { rds_detach(c, v); } }
    } undo{ c, v };
    int rc;
    RateChain& R = r.rate;
    rate_describe(R, *d);
    r.exact = v.nco_exact;
    r.pd_re = pd_re;
    r.pd_im = pd_im;
    r.theta = sdrpp_host::turnsPerSample(pd_re, pd_im);
    r.tile = tile;
    r.pitch = pitch;
    size_t cap = v.st[(size_t)v.i_chan].cap;
    r.st.reserve(SDRPP_MAX_DECIM_STAGES + 2);
    if (r.exact) {
        r.st.emplace_back();
        if (stream_alloc(c, r.st.back(), 2, R.need(0, 0), cap)) { return SDRPP_ERR_NOMEM; }
        if ((rc = dev_alloc(c, &r.d_rot, 1))) { return rc; }
        const float2 unit = make_float2(1.0f, 0.0f);  // frequency_xlator.h:21
        HIPCHK(c, hipMemcpy(r.d_rot, &unit, sizeof(unit), hipMemcpyHostToDevice));
    }
    r.i_stage0 = (int)r.st.size();
    RateForm form;  // stage 0 in closed form: the fused stage reads its taps in natural order; the bank is the context's, and 5000 phases have no matrix form
    form.natural = r.exact ? 0u : 1u;
    form.matrix = r.exact ? ~0u : ~1u;
    form.poly_matrix = false;
    if (R.has_poly()) {
        if ((rc = rds_bank_acquire(c, r))) { return rc; }
        form.bank = c->rds_banks[r.bank_key].d_bank;
    }
    if ((rc = rate_build(c, R, form, r.st, cap, 0))) { return rc; }
    if (R.has_poly()) { r.i_poly = (int)r.st.size() - 1; }
    r.i_last = (int)r.st.size() - 1;
    if (!r.exact) {
        // the streams the demodulator may read must remember the first stage's reach; the branch starts from a cleared delay line
        const int K0 = R.ntaps(0);
        if ((rc = stream_grow_hist(c, v.st[(size_t)v.i_chan], K0))) { return rc; }
        if ((rc = stream_grow_hist(c, chan_feed(v), K0))) { return rc; }
        if (v.i_ifc >= 0 && v.st[(size_t)v.i_ifc].base && (rc = stream_grow_hist(c, v.st[(size_t)v.i_ifc], K0))) { return rc; }
        for (int i = 0; i < 2; i++) {
            if ((rc = dev_alloc(c, &r.d_line[i], (size_t)K0))) { return rc; }
            HIPCHK(c, hipMemset(r.d_line[i], 0, (size_t)K0 * sizeof(float)));
        }
        r.frozen = true;
        r.line_cur = 0;
        r.line_fed = 0;
    }
    r.attached = true;
    r.on = enabled;
    undo.armed = false;
    return SDRPP_OK;
}
// sdrpp_vfo_replace with keep & 2 between two WFM VFOs: the branch — parameters, streams, state — belongs to the demodulator object and moves with it
int rds_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n) {
    if (!o.rds.attached) { return SDRPP_OK; }
    if (o.rds.exact != n.nco_exact) {  // the other NCO mode keeps its state in another form: the same description, attached to the new handle from cleared state
        const RateDesc d = rate_desc(o.rds.rate);
        return rds_apply(c, n, &d, o.rds.pd_re, o.rds.pd_im, o.rds.on);
    }
    if (int rc = rds_freeze(c, o)) { return rc; }
    n.rds = std::move(o.rds);
    o.rds = Vfo::Rds{};
    n.rds.ran = false;
    for (auto& s : n.rds.st) { s.n = 0; }
    if (!n.rds.exact) {
        const int K0 = n.rds.rate.ntaps(0);
        int rc;
        if ((rc = stream_grow_hist(c, n.st[(size_t)n.i_chan], K0))) { return rc; }
        if ((rc = stream_grow_hist(c, chan_feed(n), K0))) { return rc; }
        if (n.i_ifc >= 0 && n.st[(size_t)n.i_ifc].base && (rc = stream_grow_hist(c, n.st[(size_t)n.i_ifc], K0))) { return rc; }
    }
    return SDRPP_OK;
}
// ---- stereo branch of the WFM demodulator ---------------------------------------------------------------------------------------------
// BroadcastFM::reset as far as it concerns what the demodulator reads and the RDS branch does not own: the stream the demodulator reads forgets what it
// has seen (previous phase 0, cleared pilot / audio lines: atan2f(0, 0) = 0 makes a zeroed history exactly that) and the branch starts over (stereo_clear).
// The RDS branch's first decimator keeps its line (rds_freeze), as xlator / rdsResamp are left alone by reset().
int stereo_reset_demod(sdrpp_ctx* c, Vfo& v) {
    if (int rc = rds_freeze(c, v)) { return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Stream& f = demod_feed(v);
    for (int i = 0; i < 2; i++) {
        if (f.hist[i]) { HIPCHK(c, hipMemset(f.hist[i], 0, (size_t)std::max(f.hist_len, 1) * f.width * sizeof(float))); }
    }
    return stereo_clear(c, v);
}
bool stereo_same_desc(const Vfo::Stereo& s, const sdrpp_stereo_desc* d) {
    return s.K == d->pilot_ntaps && s.delay == d->delay && s.alpha == d->alpha && s.beta == d->beta && s.init_freq == d->init_freq && s.min_freq == d->min_freq &&
           s.max_freq == d->max_freq && memcmp(s.ptaps.data(), d->pilot_taps, s.ptaps.size() * sizeof(float)) == 0;
}
// every stream the demodulator may read remembers the pilot filter's reach
int stereo_grow_feeds(sdrpp_ctx* c, Vfo& v, int K) {
    int rc;
    if ((rc = stream_grow_hist(c, v.st[(size_t)v.i_chan], K))) { return rc; }
    if ((rc = stream_grow_hist(c, chan_feed(v), K))) { return rc; }
    if (v.i_ifc >= 0 && v.st[(size_t)v.i_ifc].base && (rc = stream_grow_hist(c, v.st[(size_t)v.i_ifc], K))) { return rc; }
    return SDRPP_OK;
}
// sdrpp_vfo_set_stereo on a VFO the caller has looked up (the stream is idle); d == nullptr: the branch goes
int stereo_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_stereo_desc* d) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Vfo::Stereo& s = v.stereo;
    if (!d) {
        if (s.attached && s.on) {
            if (int rc = stereo_reset_demod(c, v)) { return rc; }
        }
        stereo_free(s);
        return SDRPP_OK;
    }
    if (v.d.demod != SDRPP_DEMOD_WFM) { return fail(c, SDRPP_ERR_UNSUPPORTED, "the stereo branch needs a WFM VFO"); }
    if (d->pilot_ntaps <= 0 || !(d->pilot_ntaps & 1) || !d->pilot_taps) { return fail(c, SDRPP_ERR_INVALID, "stereo pilot filter: %d taps (an odd count, with taps)", d->pilot_ntaps); }
    if (d->pilot_ntaps > SDRPP_ST_PILOT_MAX_TAPS) { return fail(c, SDRPP_ERR_UNSUPPORTED, "stereo pilot filter of %d taps (max %d)", d->pilot_ntaps, SDRPP_ST_PILOT_MAX_TAPS); }
    if (d->delay <= 0 || d->delay > 65536) { return fail(c, SDRPP_ERR_INVALID, "stereo delay %d", d->delay); }
    // The loop's wrap subtracts 2 pi until the phase is back inside +-pi: every step may carry it at most kStereoMaxStep beyond, so that it ends after two
    // rounds for every description that is taken (the reference's own: 0.48 + 0.25 pi)
    const float kPi = 3.14159265f, kStereoMaxStep = 4.0f * kPi;
    const bool finite = std::isfinite(d->alpha) && std::isfinite(d->beta) && std::isfinite(d->init_freq) && std::isfinite(d->min_freq) && std::isfinite(d->max_freq);
    if (!finite || !(d->max_freq > d->min_freq) || fabsf(d->min_freq) > kPi || fabsf(d->max_freq) > kPi || fabsf(d->init_freq) > kPi ||
        !(fabsf(d->alpha) * kPi + std::max(fabsf(d->min_freq), fabsf(d->max_freq)) <= kStereoMaxStep)) {
        return fail(c, SDRPP_ERR_INVALID, "stereo loop: frequency limits %g .. %g (an interval within +-pi), initial frequency %g, alpha %g (|alpha| pi + the largest limit <= 4 pi), beta %g: all finite",
                    d->min_freq, d->max_freq, d->init_freq, d->alpha, d->beta);
    }
    if (v.audio_ntaps > SDRPP_ST_AUDIO_MAX_TAPS) { return fail(c, SDRPP_ERR_UNSUPPORTED, "stereo branch behind an audio low-pass of %d taps (max %d)", v.audio_ntaps, SDRPP_ST_AUDIO_MAX_TAPS); }
    const bool enabled = d->enabled != 0;
    if (s.attached && stereo_same_desc(s, d)) {  // the same branch: only the switch, which is BroadcastFM::setStereo
        if (s.on == enabled) { return SDRPP_OK; }
        s.on = enabled;
        s.ran = false;
        return stereo_reset_demod(c, v);
    }
    const bool was_on = s.attached && s.on;
    stereo_free(s);
    // every early return below gives back what was built so far — and, where an enabled branch has gone with it, makes the demodulator start over as
    // every other way of switching it off does
    struct Undo {
        sdrpp_ctx* c; Vfo& v; bool was_on; bool armed = true;
        ~Undo() {
            if (!armed) { return; }
            stereo_free(v.stereo);
            if (was_on) { (void)stereo_reset_demod(c, v); }
        }
    } undo{ c, v, was_on };
    int rc;
    s.K = d->pilot_ntaps;
    s.delay = d->delay;
    s.alpha = d->alpha;
    s.beta = d->beta;
    s.init_freq = d->init_freq;
    s.min_freq = d->min_freq;
    s.max_freq = d->max_freq;
    s.ptaps.assign(d->pilot_taps, d->pilot_taps + 2 * (size_t)d->pilot_ntaps);
    if ((rc = upload(c, &s.d_ptaps, s.ptaps.data(), s.ptaps.size()))) { return rc; }
    if ((rc = dev_alloc(c, &s.d_state, 1))) { return rc; }
    const size_t cap = v.st[(size_t)v.i_chan].cap;
    const int hist[3] = { s.delay + v.audio_ntaps - 1, 0, std::max(v.audio_ntaps - 1, 0) };
    s.st.resize(3);
    for (int i = 0; i < 3; i++) {
        if (stream_alloc(c, s.st[(size_t)i], 1, hist[i], cap)) { return SDRPP_ERR_NOMEM; }
    }
    if ((rc = stereo_grow_feeds(c, v, s.K))) { return rc; }
    s.attached = true;
    s.on = enabled;
    undo.armed = false;
    if (enabled || was_on) { return stereo_reset_demod(c, v); }  // (a switch: the demodulator starts over)
    return stereo_clear(c, v);
}
// sdrpp_vfo_replace with keep & 2 between two WFM VFOs: the branch belongs to the demodulator object and moves with it, parameters and state.  Its streams are
// sized for the IF stream's capacity and the audio filter's length: a new handle that differs in either gets the description attached afresh, and an enabled
// branch then starts, with the whole demodulator, from the reset() state (*cleared: the caller leaves the new handle's view of the IF stream zero too — a live
// pilot window in front of zeroed delay and audio lines would be neither the moved state nor a reset one).
int stereo_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n, bool* cleared) {
    Vfo::Stereo& s = o.stereo;
    *cleared = false;
    if (!s.attached) { return SDRPP_OK; }
    if (o.st[(size_t)o.i_chan].cap != n.st[(size_t)n.i_chan].cap || o.audio_ntaps != n.audio_ntaps) {
        const std::vector<float> taps = s.ptaps;
        const sdrpp_stereo_desc d{ taps.data(), s.K, s.delay, s.alpha, s.beta, s.init_freq, s.min_freq, s.max_freq, s.on ? 1 : 0 };
        *cleared = s.on;
        return stereo_apply(c, n, &d);
    }
    n.stereo = std::move(o.stereo);
    o.stereo = Vfo::Stereo{};
    n.stereo.ran = false;
    for (auto& q : n.stereo.st) { q.n = 0; }
    return stereo_grow_feeds(c, n, n.stereo.K);
}
// ---- framer behind the symbol branch (M17Slice4FSK, M17FrameDemux) --------------------------------------------------------------------------
void frame_detach(sdrpp_ctx* c, Vfo& v) {
    Vfo::Frame& f = v.frame;
    if (f.tab_key) {
        auto it = c->frame_tabs.find(f.tab_key);
        if (it != c->frame_tabs.end() && --it->second.refs <= 0) {
            dev_free(it->second.d_table);
            c->frame_tabs.erase(it);
        }
    }
    frame_free_own(f);
    f = Vfo::Frame{};
}
int frame_record_stride(int frame_bits) { return (2 + frame_bits / 8 + 3) & ~3; }
// the kernel's table: interleave[k] in the low half of word k, scramble[k] in bit 16
std::vector<uint32_t> frame_words(const sdrpp_frame_desc* d) {
    std::vector<uint32_t> w((size_t)d->frame_bits);
    for (int k = 0; k < d->frame_bits; k++) { w[(size_t)k] = (uint32_t)d->interleave[k] | ((uint32_t)(d->scramble[k] & 1) << 16); }
    return w;
}
// The context's shared table (keyed by a hash over its words, one reference per framer): uploaded with its first user
int frame_tab_acquire(sdrpp_ctx* c, Vfo::Frame& f, const std::vector<uint32_t>& words) {
    unsigned long long h = 1469598103934665603ull;
    for (uint32_t u : words) { h = (h ^ u) * 1099511628211ull; }
    const unsigned long long key = h ? h : 1ull;
    auto it = c->frame_tabs.find(key);
    if (it != c->frame_tabs.end() && it->second.words != words) { return fail(c, SDRPP_ERR_UNSUPPORTED, "framer tables: two different pairs under one key"); }  // (a 64-bit collision: never seen)
    if (it == c->frame_tabs.end()) {
        sdrpp_ctx::FrameTab T;
        T.words = words;
        if (int rc = upload(c, &T.d_table, T.words.data(), T.words.size())) { return rc; }
        it = c->frame_tabs.emplace(key, std::move(T)).first;
    }
    it->second.refs++;
    f.tab_key = key;
    f.d_table = it->second.d_table;
    return SDRPP_OK;
}
// a fresh M17FrameDemux: delay 0, searching
int frame_clear(sdrpp_ctx* c, Vfo& v) {
    Vfo::Frame& f = v.frame;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemset(f.d_state, 0, (size_t)(SDRPP_FRAME_STATE_HEAD + SDRPP_FRAME_MAX_BITS / 4) * sizeof(uint32_t)));
    f.ran = false;
    for (auto& q : f.st) { q.n = 0; }
    return SDRPP_OK;
}
bool frame_same_desc(const Vfo::Frame& f, const sdrpp_frame_desc* d, const sdrpp_ctx* c) {
    if (f.high_cut != d->high_cut || f.n_sync != d->n_sync || f.frame_bits != d->frame_bits || memcmp(f.sync, d->sync, (size_t)d->n_sync * sizeof(uint16_t)) != 0) { return false; }
    auto it = c->frame_tabs.find(f.tab_key);
    return it != c->frame_tabs.end() && it->second.words == frame_words(d);
}
// sdrpp_vfo_set_framer on a VFO the caller has looked up (the stream is idle); d == nullptr: the framer goes
int frame_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_frame_desc* d, bool enabled) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d) {
        frame_detach(c, v);
        return SDRPP_OK;
    }
    if (!v.sym.attached || v.sym.st.size() != 4) { return fail(c, SDRPP_ERR_INVALID, "framer: VFO %d carries no symbol branch", v.id); }
    if (!std::isfinite(d->high_cut)) { return fail(c, SDRPP_ERR_INVALID, "framer: second threshold %g: finite", d->high_cut); }
    if (d->n_sync < 1 || d->n_sync > SDRPP_FRAME_MAX_SYNC) { return fail(c, SDRPP_ERR_INVALID, "framer: %d sync words (1 .. %d)", d->n_sync, SDRPP_FRAME_MAX_SYNC); }
    if (d->frame_bits < 8 || d->frame_bits > SDRPP_FRAME_MAX_BITS || d->frame_bits % 8 != 0) { return fail(c, SDRPP_ERR_INVALID, "framer: frames of %d bits (a multiple of 8, 8 .. %d)", d->frame_bits, SDRPP_FRAME_MAX_BITS); }
    if (!d->scramble || !d->interleave) { return fail(c, SDRPP_ERR_INVALID, "framer: a table is missing"); }
    {
        std::vector<char> seen((size_t)d->frame_bits, 0);
        for (int k = 0; k < d->frame_bits; k++) {
            if (d->scramble[k] > 1) { return fail(c, SDRPP_ERR_INVALID, "framer: scramble[%d] = %d (0 or 1)", k, (int)d->scramble[k]); }
            if ((int)d->interleave[k] >= d->frame_bits || seen[(size_t)d->interleave[k]]) { return fail(c, SDRPP_ERR_INVALID, "framer: interleave[%d] = %d: the table is no permutation of 0 .. %d", k, (int)d->interleave[k], d->frame_bits - 1); }
            seen[(size_t)d->interleave[k]] = 1;
        }
    }
    Vfo::Frame& f = v.frame;
    if (f.attached && frame_same_desc(f, d, c)) {  // the same framer: only the switch — everything it holds stays as it is
        if (f.on && !enabled) {
            for (auto& q : f.st) { q.n = 0; }
        }
        f.on = enabled;
        f.ran = f.ran && enabled;
        return SDRPP_OK;
    }
    frame_detach(c, v);
    // every early return below gives back what was built so far
    struct Undo {
        sdrpp_ctx* c; Vfo& v; bool armed = true;
        ~Undo() { if (armed) { frame_detach(c, v); } }
    } undo{ c, v };
    int rc;
    f.high_cut = d->high_cut;
    f.n_sync = d->n_sync;
    for (int s = 0; s < d->n_sync; s++) { f.sync[s] = d->sync[s]; }
    f.frame_bits = d->frame_bits;
    f.stride = frame_record_stride(d->frame_bits);
    if ((rc = frame_tab_acquire(c, f, frame_words(d)))) { return rc; }
    if ((rc = dev_alloc(c, &f.d_state, (size_t)(SDRPP_FRAME_STATE_HEAD + SDRPP_FRAME_MAX_BITS / 4)))) { return rc; }
    // per-block buffers: the records a block of the branch's symbol capacity can complete (bytes, four to a float) and the per-push counts
    const size_t rcap = (size_t)f.cap_of((int)v.sym.st[1].cap);
    const size_t caps[2] = { (rcap * (size_t)f.stride + 3) / 4, (size_t)kGroupMax };
    f.st.resize(2);
    for (int i = 0; i < 2; i++) {
        if (stream_alloc(c, f.st[(size_t)i], 1, 0, caps[i])) { return SDRPP_ERR_NOMEM; }
    }
    if ((rc = frame_clear(c, v))) { return rc; }
    f.attached = true;
    f.on = enabled;
    undo.armed = false;
    return SDRPP_OK;
}
// sdrpp_vfo_replace with keep & 2, behind sym_hand_over: where the branch moved as it is the framer moves with everything it holds; where the branch was attached
// afresh (another stream capacity) so is the framer, cleared
int frame_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n, bool moved) {
    Vfo::Frame& f = o.frame;
    if (!f.attached) { return SDRPP_OK; }
    if (!moved) {
        const std::vector<uint32_t> words = c->frame_tabs[f.tab_key].words;
        std::vector<uint8_t> scr(words.size());
        std::vector<uint16_t> il(words.size());
        for (size_t k = 0; k < words.size(); k++) {
            scr[k] = (uint8_t)((words[k] >> 16) & 1u);
            il[k] = (uint16_t)(words[k] & 0xFFFFu);
        }
        sdrpp_frame_desc d{};
        d.high_cut = f.high_cut;
        d.n_sync = f.n_sync;
        for (int s = 0; s < f.n_sync; s++) { d.sync[s] = f.sync[s]; }
        d.frame_bits = f.frame_bits;
        d.scramble = scr.data();
        d.interleave = il.data();
        return frame_apply(c, n, &d, f.on);
    }
    n.frame = std::move(o.frame);
    o.frame = Vfo::Frame{};
    n.frame.ran = false;
    for (auto& q : n.frame.st) { q.n = 0; }
    return SDRPP_OK;
}
int frame_reset(sdrpp_ctx* c, Vfo& v) {
    if (!v.frame.attached) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no framer", v.id); }
    return frame_clear(c, v);
}
// The frames of the most recent block: the job's own counts, read from the device (the host waits for the stream)
int frame_count(sdrpp_ctx* c, Vfo& v) {
    Vfo::Frame& f = v.frame;
    if (!f.attached) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no framer", v.id); }
    if (!f.on || !f.ran || f.npush <= 0) { return 0; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int cnt[kGroupMax] = {};
    HIPCHK(c, hipMemcpy(cnt, f.st[1].data, (size_t)std::min(f.npush, kGroupMax) * sizeof(int), hipMemcpyDeviceToHost));
    int total = 0;
    for (int j = 0; j < std::min(f.npush, kGroupMax); j++) { total += std::max(cnt[j], 0); }
    return std::min(total, f.cap);
}
// ---- symbol branch of a RAW VFO -------------------------------------------------------------------------------------------------------
void sym_detach(sdrpp_ctx* c, Vfo& v) {
    frame_detach(c, v);  // (the framer reads the branch's outputs: it goes with it)
    Vfo::Sym& y = v.sym;
    if (y.bank_key) {
        auto it = c->sym_banks.find(y.bank_key);
        if (it != c->sym_banks.end() && --it->second.refs <= 0) {
            dev_free(it->second.d_bank);
            c->sym_banks.erase(it);
        }
    }
    sym_free_own(y);
    y = Vfo::Sym{};
}
// The context's shared interpolator bank (keyed by rds_bank_hash over its shape and its floats, one reference per branch): uploaded with its first user
int sym_bank_acquire(sdrpp_ctx* c, Vfo::Sym& y, const float* bank) {
    const int n = y.phases * y.T;
    const unsigned long long key = rds_bank_hash(y.phases, y.T, bank, n);
    auto it = c->sym_banks.find(key);
    if (it != c->sym_banks.end() && (it->second.phases != y.phases || it->second.T != y.T || memcmp(it->second.taps.data(), bank, (size_t)n * sizeof(float)) != 0)) {
        return fail(c, SDRPP_ERR_UNSUPPORTED, "interpolator bank: two different banks under one key");  // (a 64-bit collision: never seen)
    }
    if (it == c->sym_banks.end()) {
        sdrpp_ctx::SymBank B;
        B.taps.assign(bank, bank + n);
        if (int rc = upload(c, &B.d_bank, B.taps.data(), B.taps.size())) { return rc; }
        B.phases = y.phases;
        B.T = y.T;
        it = c->sym_banks.emplace(key, std::move(B)).first;
    }
    it->second.refs++;
    y.bank_key = key;
    y.d_bank = it->second.d_bank;
    return SDRPP_OK;
}
// a fresh POCSAGDSP: previous phase 0, cleared lines, phase 0, freq = omega, lastOut 0, offset 0
int sym_clear(sdrpp_ctx* c, Vfo& v) {
    Vfo::Sym& y = v.sym;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemset(y.d_lines, 0, (size_t)2 * (size_t)(y.K + y.T) * sizeof(float)));
    const int zero = 0;
    float st[4] = { 0.0f, y.omega, 0.0f, 0.0f };
    memcpy(&st[3], &zero, sizeof(int));
    HIPCHK(c, hipMemcpy(y.d_state, st, sizeof(st), hipMemcpyHostToDevice));
    y.cur = 0;
    y.ran = false;
    for (auto& q : y.st) { q.n = 0; }
    return SDRPP_OK;
}
bool sym_same_desc(const Vfo::Sym& y, const sdrpp_sym_desc* d, const sdrpp_ctx* c) {
    if (y.inv_deviation != d->inv_deviation || y.K != d->shape_ntaps || y.omega != d->omega || y.mu_gain != d->mu_gain || y.omega_gain != d->omega_gain || y.min_omega != d->min_omega ||
        y.max_omega != d->max_omega || y.phases != d->interp_phases || y.T != d->interp_ntaps || memcmp(y.taps.data(), d->shape_taps, y.taps.size() * sizeof(float)) != 0) {
        return false;
    }
    auto it = c->sym_banks.find(y.bank_key);
    return it != c->sym_banks.end() && memcmp(it->second.taps.data(), d->interp_bank, it->second.taps.size() * sizeof(float)) == 0;
}
// sdrpp_vfo_set_symbols on a VFO the caller has looked up (the stream is idle); d == nullptr: the branch goes
int sym_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_sym_desc* d, bool enabled) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d) {
        sym_detach(c, v);
        return SDRPP_OK;
    }
    if (v.d.demod != SDRPP_DEMOD_RAW) { return fail(c, SDRPP_ERR_UNSUPPORTED, "the symbol branch needs a RAW VFO"); }
    if (d->shape_ntaps < 1 || d->shape_ntaps > SDRPP_SYM_MAX_SHAPE_TAPS || !d->shape_taps) { return fail(c, SDRPP_ERR_INVALID, "symbol branch: shaping filter of %d taps (1 .. %d, with taps)", d->shape_ntaps, SDRPP_SYM_MAX_SHAPE_TAPS); }
    if (d->interp_ntaps < 1 || d->interp_ntaps > SDRPP_SYM_MAX_INTERP_TAPS || d->interp_phases < 1 || d->interp_phases > SDRPP_SYM_MAX_PHASES || !d->interp_bank) {
        return fail(c, SDRPP_ERR_INVALID, "symbol branch: interpolator of %d phases x %d taps (1 .. %d x 1 .. %d, with a bank)", d->interp_phases, d->interp_ntaps, SDRPP_SYM_MAX_PHASES, SDRPP_SYM_MAX_INTERP_TAPS);
    }
    const bool finite = std::isfinite(d->inv_deviation) && std::isfinite(d->omega) && std::isfinite(d->mu_gain) && std::isfinite(d->omega_gain) && std::isfinite(d->min_omega) && std::isfinite(d->max_omega);
    // every step floorf(phase + freq + mu_gain * error), phase in [0, 1), |error| <= 1, advances at least one sample and at most SDRPP_SYM_MAX_STEP + 1
    if (!finite || !(d->min_omega < d->max_omega) || !(d->min_omega - fabsf(d->mu_gain) >= 1.0f) || !(d->max_omega + fabsf(d->mu_gain) <= (float)SDRPP_SYM_MAX_STEP)) {
        return fail(c, SDRPP_ERR_INVALID, "symbol loop: omega limits %g .. %g, omega %g, mu gain %g, omega gain %g, 1 / deviation %g: all finite, min < max, min - |mu gain| >= 1, max + |mu gain| <= %d",
                    d->min_omega, d->max_omega, d->omega, d->mu_gain, d->omega_gain, d->inv_deviation, SDRPP_SYM_MAX_STEP);
    }
    const size_t cap = v.st[(size_t)v.i_chan].cap;
    if (cap + 16 >= ((size_t)1 << 24) - (size_t)(SDRPP_SYM_MAX_STEP + 1)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "symbol branch on a stream of up to %zu samples per push (offsets are exact below 2^24)", cap); }
    Vfo::Sym& y = v.sym;
    if (y.attached && sym_same_desc(y, d, c)) {  // the same branch: only the switch — everything it holds stays as it is
        if (y.on && !enabled) {
            for (auto& q : y.st) { q.n = 0; }
        }
        y.on = enabled;
        y.ran = y.ran && enabled;
        return SDRPP_OK;
    }
    sym_detach(c, v);
    // every early return below gives back what was built so far
    struct Undo {
        sdrpp_ctx* c; Vfo& v; bool armed = true;
        ~Undo() { if (armed) { sym_detach(c, v); } }
    } undo{ c, v };
    int rc;
    y.inv_deviation = d->inv_deviation;
    y.K = d->shape_ntaps;
    y.omega = d->omega;
    y.mu_gain = d->mu_gain;
    y.omega_gain = d->omega_gain;
    y.min_omega = d->min_omega;
    y.max_omega = d->max_omega;
    y.phases = d->interp_phases;
    y.T = d->interp_ntaps;
    y.min_step = std::max(1, (int)floorf(d->min_omega - fabsf(d->mu_gain)));
    y.taps.assign(d->shape_taps, d->shape_taps + d->shape_ntaps);
    if ((rc = upload(c, &y.d_taps, y.taps.data(), y.taps.size()))) { return rc; }
    if ((rc = sym_bank_acquire(c, y, d->interp_bank))) { return rc; }
    if ((rc = dev_alloc(c, &y.d_state, 4))) { return rc; }
    if ((rc = dev_alloc(c, &y.d_lines, (size_t)2 * (size_t)(y.K + y.T)))) { return rc; }
    // per-block buffers: the front's [T - 1][n] (stream_alloc leaves 16 samples of room behind `cap`: T - 1 <= 15), the symbols a block of `cap` samples can
    // start, their bits (bytes, four to a float) and the per-push counts
    const size_t scap = (size_t)y.cap_of((int)cap);
    const size_t caps[4] = { cap, scap, (scap + 3) / 4, (size_t)kGroupMax };
    y.st.resize(4);
    for (int i = 0; i < 4; i++) {
        if (stream_alloc(c, y.st[(size_t)i], 1, 0, caps[i])) { return SDRPP_ERR_NOMEM; }
    }
    if ((rc = sym_clear(c, v))) { return rc; }
    y.attached = true;
    y.on = enabled;
    undo.armed = false;
    return SDRPP_OK;
}
// sdrpp_vfo_replace with keep & 2 between two RAW VFOs: the branch moves with everything it holds; a new handle with another stream capacity gets the
// description attached afresh (its buffers are sized for the capacity) and starts cleared
int sym_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n) {
    Vfo::Sym& y = o.sym;
    if (!y.attached) { return SDRPP_OK; }
    if (o.st[(size_t)o.i_chan].cap != n.st[(size_t)n.i_chan].cap) {
        const std::vector<float> taps = y.taps, bank = c->sym_banks[y.bank_key].taps;
        const sdrpp_sym_desc d{ y.inv_deviation, y.K, taps.data(), y.omega, y.mu_gain, y.omega_gain, y.min_omega, y.max_omega, y.phases, y.T, bank.data() };
        if (int rc = sym_apply(c, n, &d, y.on)) { return rc; }
        return frame_hand_over(c, o, n, false);
    }
    n.sym = std::move(o.sym);
    o.sym = Vfo::Sym{};
    n.sym.ran = false;
    for (auto& q : n.sym.st) { q.n = 0; }
    return frame_hand_over(c, o, n, true);
}
// sdrpp_vfo_reset: the IF history it clears is the discriminator's "previous phase 0" (as for the RDS branch); everything else the branch holds stays
int sym_reset_prev(sdrpp_ctx* c, Vfo& v) {
    Vfo::Sym& y = v.sym;
    if (!y.attached) { return SDRPP_OK; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemset(y.d_lines + (size_t)y.cur * (size_t)(y.K + y.T) + (y.K - 1), 0, sizeof(float)));
    return SDRPP_OK;
}
// The symbols of the most recent block: the loop's own counts, read from the device (the host waits for the stream)
const char* const kNoSym = "VFO %d has no symbol branch";
int sym_count(sdrpp_ctx* c, Vfo& v) {
    Vfo::Sym& y = v.sym;
    if (!y.attached) { return fail(c, SDRPP_ERR_INVALID, kNoSym, v.id); }
    if (!y.on || !y.ran || y.npush <= 0) { return 0; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int cnt[kGroupMax] = {};
    HIPCHK(c, hipMemcpy(cnt, y.st[3].data, (size_t)std::min(y.npush, kGroupMax) * sizeof(int), hipMemcpyDeviceToHost));
    int total = 0;
    for (int j = 0; j < std::min(y.npush, kGroupMax); j++) { total += cnt[j]; }
    return std::min(total, y.cap);
}

// ---- RDS demodulator behind the RDS branch (source 0) or on a RAW VFO (source 1) ------------------------------------------------------------------
void rdsd_detach(sdrpp_ctx* c, Vfo& v) {
    Vfo::Rdsd& y = v.rdsd;
    if (y.bank_key) {
        auto it = c->rdsd_banks.find(y.bank_key);
        if (it != c->rdsd_banks.end() && --it->second.refs <= 0) {
            dev_free(it->second.d_taps);
            dev_free(it->second.d_bank);
            c->rdsd_banks.erase(it);
        }
    }
    rdsd_free_own(y);
    y = Vfo::Rdsd{};
}
// The context's shared tap table and interpolator bank (keyed by rds_bank_hash over both, one reference per demodulator): uploaded with their first user
int rdsd_bank_acquire(sdrpp_ctx* c, Vfo::Rdsd& y, const float* taps, const float* bank) {
    std::vector<float> all(taps, taps + 2 * (size_t)y.K);
    all.insert(all.end(), bank, bank + (size_t)y.phases * (size_t)y.T);
    const unsigned long long key = rds_bank_hash(y.K, y.phases * 32 + y.T, all.data(), (int)all.size());
    auto it = c->rdsd_banks.find(key);
    if (it != c->rdsd_banks.end() && (it->second.K != y.K || it->second.phases != y.phases || it->second.T != y.T || memcmp(it->second.taps.data(), taps, 2 * (size_t)y.K * sizeof(float)) != 0 ||
                                     memcmp(it->second.bank.data(), bank, (size_t)y.phases * (size_t)y.T * sizeof(float)) != 0)) {
        return fail(c, SDRPP_ERR_UNSUPPORTED, "rds demodulator tables: two different descriptions under one key");  // (a 64-bit collision: never seen)
    }
    if (it == c->rdsd_banks.end()) {
        sdrpp_ctx::RdsdBank B;
        B.taps.assign(taps, taps + 2 * (size_t)y.K);
        B.bank.assign(bank, bank + (size_t)y.phases * (size_t)y.T);
        if (int rc = upload(c, &B.d_taps, B.taps.data(), B.taps.size())) { return rc; }
        if (int rc = upload(c, &B.d_bank, B.bank.data(), B.bank.size())) {
            dev_free(B.d_taps);
            return rc;
        }
        B.K = y.K;
        B.phases = y.phases;
        B.T = y.T;
        it = c->rdsd_banks.emplace(key, std::move(B)).first;
    }
    it->second.refs++;
    y.bank_key = key;
    y.d_taps = it->second.d_taps;
    y.d_bank = it->second.d_bank;
    return SDRPP_OK;
}
// RDSDemod::reset() (rds_demod.h:51-62); `fresh`: RDSDemod::init — MM's delay samples cleared as well (a new object's buffer)
int rdsd_clear(sdrpp_ctx* c, Vfo& v, bool fresh) {
    Vfo::Rdsd& y = v.rdsd;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int zero = 0;
    float st[SDRPP_RDSD_STATE_HEAD] = {};
    st[0] = y.agc[3];
    st[1] = y.loop[0][2]; st[2] = y.loop[0][3];
    st[3] = y.loop[1][2]; st[4] = y.loop[1][3];
    st[5] = 0.0f; st[6] = y.omega; st[7] = 0.0f;
    memcpy(&st[8], &zero, sizeof(int));
    memcpy(&st[9], &zero, sizeof(int));
    HIPCHK(c, hipMemcpy(y.d_state, st, sizeof(st), hipMemcpyHostToDevice));
    const size_t line = 2 * (size_t)(y.K - 1) + (fresh ? (size_t)(y.T - 1) : 0);
    if (line > 0) { HIPCHK(c, hipMemset(y.d_state + SDRPP_RDSD_STATE_HEAD, 0, line * sizeof(float))); }
    y.ran = false;
    for (auto& q : y.st) { q.n = 0; }
    return SDRPP_OK;
}
bool rdsd_same_desc(const Vfo::Rdsd& y, const sdrpp_rdsd_desc* d, const sdrpp_ctx* c) {
    const sdrpp_rdsd_loop* lp[2] = { &d->loop1, &d->loop2 };
    for (int i = 0; i < 2; i++) {
        const float f[6] = { lp[i]->alpha, lp[i]->beta, lp[i]->init_phase, lp[i]->init_freq, lp[i]->min_freq, lp[i]->max_freq };
        if (memcmp(f, y.loop[i], sizeof(f)) != 0) { return false; }
    }
    const float agc[4] = { d->agc_set_point, d->agc_max_gain, d->agc_rate, d->agc_init_gain };
    if (y.source != d->source || memcmp(agc, y.agc, sizeof(agc)) != 0 || y.K != d->n_taps || y.omega != d->omega || y.mu_gain != d->mu_gain || y.omega_gain != d->omega_gain ||
        y.min_omega != d->min_omega || y.max_omega != d->max_omega || y.phases != d->interp_phases || y.T != d->interp_ntaps) {
        return false;
    }
    auto it = c->rdsd_banks.find(y.bank_key);
    return it != c->rdsd_banks.end() && memcmp(it->second.taps.data(), d->taps, it->second.taps.size() * sizeof(float)) == 0 &&
           memcmp(it->second.bank.data(), d->interp_bank, it->second.bank.size() * sizeof(float)) == 0;
}
// the stream the demodulator reads: the RDS branch's last stage (source 0) or the VFO's channel stream (source 1: what a demodulator would read)
size_t rdsd_in_cap(const Vfo& v, int source) { return source == 0 ? v.rds.st[(size_t)v.rds.i_last].cap : v.st[(size_t)v.i_chan].cap; }
// sdrpp_vfo_set_rds_demod on a VFO the caller has looked up (the stream is idle); d == nullptr: the demodulator goes
int rdsd_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_rdsd_desc* d, bool enabled) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d) {
        rdsd_detach(c, v);
        return SDRPP_OK;
    }
    if (d->source != 0 && d->source != 1) { return fail(c, SDRPP_ERR_INVALID, "rds demodulator: source %d (0: the RDS branch, 1: the stream a demodulator would read)", d->source); }
    if (d->source == 0 && !v.rds.attached) { return fail(c, SDRPP_ERR_INVALID, "rds demodulator, source 0: VFO %d has no RDS branch (sdrpp_vfo_set_rds first)", v.id); }
    if (d->source == 1 && v.d.demod != SDRPP_DEMOD_RAW) { return fail(c, SDRPP_ERR_UNSUPPORTED, "rds demodulator, source 1: needs a RAW VFO"); }
    if (d->n_taps < 1 || d->n_taps > SDRPP_RDSD_MAX_TAPS || !d->taps) { return fail(c, SDRPP_ERR_INVALID, "rds demodulator: band-pass of %d complex taps (1 .. %d, with taps)", d->n_taps, SDRPP_RDSD_MAX_TAPS); }
    if (d->interp_ntaps < 1 || d->interp_ntaps > SDRPP_SYM_MAX_INTERP_TAPS || !d->interp_bank) {
        return fail(c, SDRPP_ERR_INVALID, "rds demodulator: interpolator of %d taps per phase (1 .. %d, with a bank)", d->interp_ntaps, SDRPP_SYM_MAX_INTERP_TAPS);
    }
    if (d->interp_phases < 1 || d->interp_phases > SDRPP_SYM_MAX_PHASES) { return fail(c, SDRPP_ERR_INVALID, "rds demodulator: interpolator of %d phases (1 .. %d)", d->interp_phases, SDRPP_SYM_MAX_PHASES); }
    if (!std::isfinite(d->agc_set_point) || !std::isfinite(d->agc_max_gain) || !std::isfinite(d->agc_rate) || !std::isfinite(d->agc_init_gain)) {
        return fail(c, SDRPP_ERR_INVALID, "rds demodulator: AGC set point %g, max gain %g, rate %g, initial gain %g: all finite", d->agc_set_point, d->agc_max_gain, d->agc_rate, d->agc_init_gain);
    }
    const sdrpp_rdsd_loop* lp[2] = { &d->loop1, &d->loop2 };
    for (int i = 0; i < 2; i++) {
        const sdrpp_rdsd_loop& l = *lp[i];
        if (!std::isfinite(l.alpha) || !std::isfinite(l.beta) || !std::isfinite(l.init_phase) || !std::isfinite(l.init_freq) || !std::isfinite(l.min_freq) || !std::isfinite(l.max_freq)) {
            return fail(c, SDRPP_ERR_INVALID, "rds demodulator: loop %d has a value that is not finite", i + 1);
        }
        if (!(l.min_freq < l.max_freq)) { return fail(c, SDRPP_ERR_INVALID, "rds demodulator: loop %d frequency limits %g .. %g: min < max", i + 1, l.min_freq, l.max_freq); }
        // the bounded-loop rule: a step of at most 2 pi from a phase inside +-pi is wrapped by ONE subtraction or addition (vfo_rdsd_kernels.h)
        if (!((double)std::max(fabsf(l.min_freq), fabsf(l.max_freq)) + (double)fabsf(l.alpha) <= 2.0 * 3.14159265358979323846) || !(fabsf(l.init_phase) <= 3.1415926535f)) {
            return fail(c, SDRPP_ERR_INVALID, "rds demodulator: loop %d with frequency limits %g .. %g, alpha %g, initial phase %g: max(|min|, |max|) + |alpha| <= 2 pi and |phase| <= pi, else the phase wrap is no single step",
                        i + 1, l.min_freq, l.max_freq, l.alpha, l.init_phase);
        }
    }
    if (!std::isfinite(d->omega) || !std::isfinite(d->mu_gain) || !std::isfinite(d->omega_gain) || !std::isfinite(d->min_omega) || !std::isfinite(d->max_omega)) {
        return fail(c, SDRPP_ERR_INVALID, "rds demodulator: clock recovery has a value that is not finite");
    }
    if (!(d->min_omega < d->max_omega) || !(d->min_omega - fabsf(d->mu_gain) >= 1.0f) || !(d->max_omega + fabsf(d->mu_gain) <= (float)SDRPP_SYM_MAX_STEP)) {
        return fail(c, SDRPP_ERR_INVALID, "rds demodulator: omega limits %g .. %g, mu gain %g: min < max, min - |mu gain| >= 1, max + |mu gain| <= %d", d->min_omega, d->max_omega, d->mu_gain, SDRPP_SYM_MAX_STEP);
    }
    const size_t cap = rdsd_in_cap(v, d->source);
    if (cap + 16 >= ((size_t)1 << 24) - (size_t)(SDRPP_SYM_MAX_STEP + 1)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "rds demodulator on a stream of up to %zu samples per push (offsets are exact below 2^24)", cap); }
    Vfo::Rdsd& y = v.rdsd;
    if (y.attached && rdsd_same_desc(y, d, c)) {  // the same demodulator: only the switch — everything it holds stays as it is
        if (y.on && !enabled) {
            for (auto& q : y.st) { q.n = 0; }
        }
        y.on = enabled;
        y.ran = y.ran && enabled;
        return SDRPP_OK;
    }
    rdsd_detach(c, v);
    // every early return below gives back what was built so far
    struct Undo {
        sdrpp_ctx* c; Vfo& v; bool armed = true;
        ~Undo() { if (armed) { rdsd_detach(c, v); } }
    } undo{ c, v };
    int rc;
    y.source = d->source;
    const float agc[4] = { d->agc_set_point, d->agc_max_gain, d->agc_rate, d->agc_init_gain };
    memcpy(y.agc, agc, sizeof(agc));
    for (int i = 0; i < 2; i++) {
        const float f[6] = { lp[i]->alpha, lp[i]->beta, lp[i]->init_phase, lp[i]->init_freq, lp[i]->min_freq, lp[i]->max_freq };
        memcpy(y.loop[i], f, sizeof(f));
    }
    y.K = d->n_taps;
    y.omega = d->omega;
    y.mu_gain = d->mu_gain;
    y.omega_gain = d->omega_gain;
    y.min_omega = d->min_omega;
    y.max_omega = d->max_omega;
    y.phases = d->interp_phases;
    y.T = d->interp_ntaps;
    y.min_step = std::max(1, (int)floorf(d->min_omega - fabsf(d->mu_gain)));
    if ((rc = rdsd_bank_acquire(c, y, d->taps, d->interp_bank))) { return rc; }
    if ((rc = dev_alloc(c, &y.d_state, (size_t)SDRPP_RDSD_STATE_HEAD + 2 * (size_t)(y.K - 1) + (size_t)(y.T - 1) + 1))) { return rc; }
    // per-block buffers: the symbols a block of `cap` samples can start, their bits (bytes, four to a float) and the per-push counts
    const size_t scap = (size_t)y.cap_of((int)cap);
    const size_t caps[3] = { scap, (scap + 3) / 4, (size_t)kGroupMax };
    y.st.resize(3);
    for (int i = 0; i < 3; i++) {
        if (stream_alloc(c, y.st[(size_t)i], 1, 0, caps[i])) { return SDRPP_ERR_NOMEM; }
    }
    if ((rc = rdsd_clear(c, v, true))) { return rc; }
    y.attached = true;
    y.on = enabled;
    undo.armed = false;
    return SDRPP_OK;
}
// the description a demodulator was attached with (the arrays are the context's copies: valid while the demodulator holds its reference)
sdrpp_rdsd_desc rdsd_desc_of(const sdrpp_ctx* c, const Vfo::Rdsd& y) {
    const sdrpp_ctx::RdsdBank& B = c->rdsd_banks.at(y.bank_key);
    sdrpp_rdsd_desc d{};
    d.source = y.source;
    d.agc_set_point = y.agc[0]; d.agc_max_gain = y.agc[1]; d.agc_rate = y.agc[2]; d.agc_init_gain = y.agc[3];
    sdrpp_rdsd_loop* lp[2] = { &d.loop1, &d.loop2 };
    for (int i = 0; i < 2; i++) { *lp[i] = sdrpp_rdsd_loop{ y.loop[i][0], y.loop[i][1], y.loop[i][2], y.loop[i][3], y.loop[i][4], y.loop[i][5] }; }
    d.n_taps = y.K;
    d.taps = B.taps.data();
    d.omega = y.omega; d.mu_gain = y.mu_gain; d.omega_gain = y.omega_gain; d.min_omega = y.min_omega; d.max_omega = y.max_omega;
    d.interp_phases = y.phases; d.interp_ntaps = y.T;
    d.interp_bank = B.bank.data();
    return d;
}
// sdrpp_vfo_replace with keep & 2 between two VFOs of the same demodulator kind, after the RDS / symbol branches have moved: the demodulator moves with
// everything it holds; a new handle whose input stream has another capacity gets the description attached afresh (its buffers are sized for it), cleared.
// A source-0 demodulator whose RDS branch did not arrive at the new handle stays behind and goes with the old handle.
int rdsd_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n, size_t old_cap) {
    Vfo::Rdsd& y = o.rdsd;
    if (!y.attached) { return SDRPP_OK; }
    if (y.source == 0 && !n.rds.attached) { return SDRPP_OK; }
    if (old_cap != rdsd_in_cap(n, y.source)) {
        const sdrpp_ctx::RdsdBank B = c->rdsd_banks.at(y.bank_key);  // (a copy: attaching may let go of the table's last reference)
        sdrpp_rdsd_desc d = rdsd_desc_of(c, y);
        d.taps = B.taps.data();
        d.interp_bank = B.bank.data();
        return rdsd_apply(c, n, &d, y.on);
    }
    n.rdsd = std::move(o.rdsd);
    o.rdsd = Vfo::Rdsd{};
    n.rdsd.ran = false;
    for (auto& q : n.rdsd.st) { q.n = 0; }
    return SDRPP_OK;
}
// The symbols of the most recent block: the job's own counts, read from the device (the host waits for the stream)
const char* const kNoRdsd = "VFO %d has no RDS demodulator";
int rdsd_count(sdrpp_ctx* c, Vfo& v) {
    Vfo::Rdsd& y = v.rdsd;
    if (!y.attached) { return fail(c, SDRPP_ERR_INVALID, kNoRdsd, v.id); }
    if (!y.on || !y.ran || y.npush <= 0) { return 0; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int cnt[kGroupMax] = {};
    HIPCHK(c, hipMemcpy(cnt, y.st[2].data, (size_t)std::min(y.npush, kGroupMax) * sizeof(int), hipMemcpyDeviceToHost));
    int total = 0;
    for (int j = 0; j < std::min(y.npush, kGroupMax); j++) { total += cnt[j]; }
    return std::min(total, y.cap);
}

// ---- Meteor QPSK demodulator on a RAW VFO -----------------------------------------------------------------------------------------------------
void qpsk_detach(sdrpp_ctx* c, Vfo& v) {
    Vfo::Qpsk& y = v.qpsk;
    if (y.bank_key) {
        auto it = c->qpsk_banks.find(y.bank_key);
        if (it != c->qpsk_banks.end() && --it->second.refs <= 0) {
            dev_free(it->second.d_taps);
            dev_free(it->second.d_bank);
            c->qpsk_banks.erase(it);
        }
    }
    qpsk_free_own(y);
    y = Vfo::Qpsk{};
}
// The context's shared real tap table and interpolator bank (keyed by rds_bank_hash over both, one reference per demodulator): uploaded with their first user
int qpsk_bank_acquire(sdrpp_ctx* c, Vfo::Qpsk& y, const float* taps, const float* bank) {
    std::vector<float> all(taps, taps + (size_t)y.K);
    all.insert(all.end(), bank, bank + (size_t)y.phases * (size_t)y.T);
    const unsigned long long key = rds_bank_hash(y.K, y.phases * 32 + y.T, all.data(), (int)all.size());
    auto it = c->qpsk_banks.find(key);
    if (it != c->qpsk_banks.end() && (it->second.K != y.K || it->second.phases != y.phases || it->second.T != y.T || memcmp(it->second.taps.data(), taps, (size_t)y.K * sizeof(float)) != 0 ||
                                     memcmp(it->second.bank.data(), bank, (size_t)y.phases * (size_t)y.T * sizeof(float)) != 0)) {
        return fail(c, SDRPP_ERR_UNSUPPORTED, "qpsk demodulator tables: two different descriptions under one key");  // (a 64-bit collision: never seen)
    }
    if (it == c->qpsk_banks.end()) {
        sdrpp_ctx::QpskBank B;
        B.taps.assign(taps, taps + (size_t)y.K);
        B.bank.assign(bank, bank + (size_t)y.phases * (size_t)y.T);
        if (int rc = upload(c, &B.d_taps, B.taps.data(), B.taps.size())) { return rc; }
        if (int rc = upload(c, &B.d_bank, B.bank.data(), B.bank.size())) {
            dev_free(B.d_taps);
            return rc;
        }
        B.K = y.K;
        B.phases = y.phases;
        B.T = y.T;
        it = c->qpsk_banks.emplace(key, std::move(B)).first;
    }
    it->second.refs++;
    y.bank_key = key;
    y.d_taps = it->second.d_taps;
    y.d_bank = it->second.d_bank;
    return SDRPP_OK;
}
// Meteor::reset() (meteor_demod.h:139-148): the filter line (fir.h:58), the gain, the loop (pll.h:55-62), MM's offset / phase / freq and six delay words
// (mm.h:87-98).  lastI and MM's T - 1 delay samples stay, as the reference leaves them; `fresh`: Meteor::init — those cleared as well (a new object)
int qpsk_clear(sdrpp_ctx* c, Vfo& v, bool fresh) {
    Vfo::Qpsk& y = v.qpsk;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float st[SDRPP_QPSK_STATE_HEAD] = {};
    if (!fresh) { HIPCHK(c, hipMemcpy(st, y.d_state, sizeof(st), hipMemcpyDeviceToHost)); }
    const float last_i = fresh ? 0.0f : st[3];
    memset(st, 0, sizeof(st));
    st[0] = y.agc[3];
    st[1] = y.loop[2]; st[2] = y.loop[3];
    st[3] = last_i;
    st[4] = 0.0f; st[5] = y.omega;
    HIPCHK(c, hipMemcpy(y.d_state, st, sizeof(st), hipMemcpyHostToDevice));
    if (fresh && y.T > 1) { HIPCHK(c, hipMemset(y.d_state + SDRPP_QPSK_STATE_HEAD, 0, 2 * (size_t)(y.T - 1) * sizeof(float))); }
    HIPCHK(c, hipMemset(y.d_lines, 0, 4 * (size_t)y.K * sizeof(float)));
    y.ran = false;
    for (auto& q : y.st) { q.n = 0; }
    return SDRPP_OK;
}
bool qpsk_same_desc(const Vfo::Qpsk& y, const sdrpp_qpsk_desc* d, const sdrpp_ctx* c) {
    const float f[6] = { d->loop.alpha, d->loop.beta, d->loop.init_phase, d->loop.init_freq, d->loop.min_freq, d->loop.max_freq };
    const float agc[4] = { d->agc_set_point, d->agc_max_gain, d->agc_rate, d->agc_init_gain };
    if (memcmp(f, y.loop, sizeof(f)) != 0 || memcmp(agc, y.agc, sizeof(agc)) != 0 || y.K != d->n_taps || y.omega != d->omega || y.mu_gain != d->mu_gain || y.omega_gain != d->omega_gain ||
        y.min_omega != d->min_omega || y.max_omega != d->max_omega || y.phases != d->interp_phases || y.T != d->interp_ntaps || y.soft_scale != d->soft_scale) {
        return false;
    }
    auto it = c->qpsk_banks.find(y.bank_key);
    return it != c->qpsk_banks.end() && memcmp(it->second.taps.data(), d->taps, it->second.taps.size() * sizeof(float)) == 0 &&
           memcmp(it->second.bank.data(), d->interp_bank, it->second.bank.size() * sizeof(float)) == 0;
}
// sdrpp_vfo_set_qpsk on a VFO the caller has looked up (the stream is idle); d == nullptr: the demodulator goes.  `broken` and `oqpsk` are modes, not a part of
// the description's identity: the same description with other modes sets them and keeps the state (sdrpp_vfo_qpsk_set_mode does only that).
int qpsk_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_qpsk_desc* d, bool enabled) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!d) {
        qpsk_detach(c, v);
        return SDRPP_OK;
    }
    if (v.d.demod != SDRPP_DEMOD_RAW) { return fail(c, SDRPP_ERR_UNSUPPORTED, "qpsk demodulator: needs a RAW VFO"); }
    if (d->n_taps < 1 || d->n_taps > SDRPP_QPSK_MAX_TAPS || !d->taps) { return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: shaping filter of %d real taps (1 .. %d, with taps)", d->n_taps, SDRPP_QPSK_MAX_TAPS); }
    if (d->interp_ntaps < 1 || d->interp_ntaps > SDRPP_SYM_MAX_INTERP_TAPS || !d->interp_bank) {
        return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: interpolator of %d taps per phase (1 .. %d, with a bank)", d->interp_ntaps, SDRPP_SYM_MAX_INTERP_TAPS);
    }
    if (d->interp_phases < 1 || d->interp_phases > SDRPP_SYM_MAX_PHASES) { return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: interpolator of %d phases (1 .. %d)", d->interp_phases, SDRPP_SYM_MAX_PHASES); }
    if (!std::isfinite(d->agc_set_point) || !std::isfinite(d->agc_max_gain) || !std::isfinite(d->agc_rate) || !std::isfinite(d->agc_init_gain)) {
        return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: AGC set point %g, max gain %g, rate %g, initial gain %g: all finite", d->agc_set_point, d->agc_max_gain, d->agc_rate, d->agc_init_gain);
    }
    const sdrpp_rdsd_loop& l = d->loop;
    if (!std::isfinite(l.alpha) || !std::isfinite(l.beta) || !std::isfinite(l.init_phase) || !std::isfinite(l.init_freq) || !std::isfinite(l.min_freq) || !std::isfinite(l.max_freq)) {
        return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: the loop has a value that is not finite");
    }
    if (!(l.min_freq < l.max_freq)) { return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: loop frequency limits %g .. %g: min < max", l.min_freq, l.max_freq); }
    // the bounded-loop rule: a step of at most 2 pi from a phase inside +-pi is wrapped by ONE subtraction or addition (vfo_rdsd_kernels.h)
    if (!((double)std::max(fabsf(l.min_freq), fabsf(l.max_freq)) + (double)fabsf(l.alpha) <= 2.0 * 3.14159265358979323846) || !(fabsf(l.init_phase) <= 3.1415926535f)) {
        return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: loop with frequency limits %g .. %g, alpha %g, initial phase %g: max(|min|, |max|) + |alpha| <= 2 pi and |phase| <= pi, else the phase wrap is no single step",
                    l.min_freq, l.max_freq, l.alpha, l.init_phase);
    }
    if (!std::isfinite(d->omega) || !std::isfinite(d->mu_gain) || !std::isfinite(d->omega_gain) || !std::isfinite(d->min_omega) || !std::isfinite(d->max_omega)) {
        return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: clock recovery has a value that is not finite");
    }
    if (!(d->min_omega < d->max_omega) || !(d->min_omega - fabsf(d->mu_gain) >= 1.0f) || !(d->max_omega + fabsf(d->mu_gain) <= (float)SDRPP_SYM_MAX_STEP)) {
        return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: omega limits %g .. %g, mu gain %g: min < max, min - |mu gain| >= 1, max + |mu gain| <= %d", d->min_omega, d->max_omega, d->mu_gain, SDRPP_SYM_MAX_STEP);
    }
    if (!std::isfinite(d->soft_scale)) { return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: soft scale %g: finite", d->soft_scale); }
    for (int k = 0; k < d->n_taps; k++) {
        if (!std::isfinite(d->taps[k])) { return fail(c, SDRPP_ERR_INVALID, "qpsk demodulator: tap %d is not finite", k); }
    }
    const size_t cap = v.st[(size_t)v.i_chan].cap;  // the stream a demodulator would read
    if (cap + 16 >= ((size_t)1 << 24) - (size_t)(SDRPP_SYM_MAX_STEP + 1)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "qpsk demodulator on a stream of up to %zu samples per push (offsets are exact below 2^24)", cap); }
    Vfo::Qpsk& y = v.qpsk;
    if (y.attached && y.st.size() == 4 && y.st[0].cap == cap && qpsk_same_desc(y, d, c)) {  // the same demodulator: only the switch and the modes — everything it holds stays as it is
        if (y.on && !enabled) {
            for (auto& q : y.st) { q.n = 0; }
        }
        y.on = enabled;
        y.ran = y.ran && enabled;
        y.broken = d->broken != 0;
        y.oqpsk = d->oqpsk != 0;
        return SDRPP_OK;
    }
    qpsk_detach(c, v);
    // every early return below gives back what was built so far
    struct Undo {
        sdrpp_ctx* c; Vfo& v; bool armed = true;
        ~Undo() { if (armed) { qpsk_detach(c, v); } }
    } undo{ c, v };
    int rc;
    const float agc[4] = { d->agc_set_point, d->agc_max_gain, d->agc_rate, d->agc_init_gain };
    memcpy(y.agc, agc, sizeof(agc));
    const float f[6] = { l.alpha, l.beta, l.init_phase, l.init_freq, l.min_freq, l.max_freq };
    memcpy(y.loop, f, sizeof(f));
    y.broken = d->broken != 0;
    y.oqpsk = d->oqpsk != 0;
    y.K = d->n_taps;
    y.omega = d->omega;
    y.mu_gain = d->mu_gain;
    y.omega_gain = d->omega_gain;
    y.min_omega = d->min_omega;
    y.max_omega = d->max_omega;
    y.soft_scale = d->soft_scale;
    y.phases = d->interp_phases;
    y.T = d->interp_ntaps;
    y.min_step = std::max(1, (int)floorf(d->min_omega - fabsf(d->mu_gain)));
    if ((rc = qpsk_bank_acquire(c, y, d->taps, d->interp_bank))) { return rc; }
    if ((rc = dev_alloc(c, &y.d_state, (size_t)SDRPP_QPSK_STATE_HEAD + 2 * (size_t)(y.T - 1) + 2))) { return rc; }
    if ((rc = dev_alloc(c, &y.d_lines, 4 * (size_t)y.K))) { return rc; }
    // per-block buffers: the filter's output, then the symbols a block of `cap` samples can start (float pairs, int8 pairs four to a float) and the per-push counts
    const size_t scap = (size_t)y.cap_of((int)cap);
    const int widths[4] = { 2, 2, 1, 1 };
    const size_t caps[4] = { cap, scap, (scap + 1) / 2, (size_t)kGroupMax };
    y.st.resize(4);
    for (int i = 0; i < 4; i++) {
        if (stream_alloc(c, y.st[(size_t)i], widths[i], 0, caps[i])) { return SDRPP_ERR_NOMEM; }
    }
    y.attached = true;  // (qpsk_clear reads nothing of it; set before so that Undo sees a whole object)
    if ((rc = qpsk_clear(c, v, true))) { return rc; }
    y.cur = 0;
    y.on = enabled;
    undo.armed = false;
    return SDRPP_OK;
}
// the description a demodulator was attached with (the arrays are the context's copies: valid while the demodulator holds its reference)
sdrpp_qpsk_desc qpsk_desc_of(const sdrpp_ctx* c, const Vfo::Qpsk& y) {
    const sdrpp_ctx::QpskBank& B = c->qpsk_banks.at(y.bank_key);
    sdrpp_qpsk_desc d{};
    d.n_taps = y.K;
    d.taps = B.taps.data();
    d.agc_set_point = y.agc[0]; d.agc_max_gain = y.agc[1]; d.agc_rate = y.agc[2]; d.agc_init_gain = y.agc[3];
    d.loop = sdrpp_rdsd_loop{ y.loop[0], y.loop[1], y.loop[2], y.loop[3], y.loop[4], y.loop[5] };
    d.broken = y.broken; d.oqpsk = y.oqpsk;
    d.omega = y.omega; d.mu_gain = y.mu_gain; d.omega_gain = y.omega_gain; d.min_omega = y.min_omega; d.max_omega = y.max_omega;
    d.interp_phases = y.phases; d.interp_ntaps = y.T;
    d.interp_bank = B.bank.data();
    d.soft_scale = y.soft_scale;
    return d;
}
// sdrpp_vfo_replace with keep & 2 between two RAW VFOs: the demodulator moves with everything it holds; a new handle whose stream has another capacity gets
// the description attached afresh (its buffers are sized for it), cleared.
int qpsk_hand_over(sdrpp_ctx* c, Vfo& o, Vfo& n) {
    Vfo::Qpsk& y = o.qpsk;
    if (!y.attached) { return SDRPP_OK; }
    if (y.st[0].cap != n.st[(size_t)n.i_chan].cap) {
        const sdrpp_ctx::QpskBank B = c->qpsk_banks.at(y.bank_key);  // (a copy: attaching may let go of the table's last reference)
        sdrpp_qpsk_desc d = qpsk_desc_of(c, y);
        d.taps = B.taps.data();
        d.interp_bank = B.bank.data();
        return qpsk_apply(c, n, &d, y.on);
    }
    qpsk_detach(c, n);
    n.qpsk = std::move(o.qpsk);
    o.qpsk = Vfo::Qpsk{};
    n.qpsk.ran = false;
    for (auto& q : n.qpsk.st) { q.n = 0; }
    return SDRPP_OK;
}
// The symbols of the most recent block: the job's own counts, read from the device (the host waits for the stream)
const char* const kNoQpsk = "VFO %d has no QPSK demodulator";
int qpsk_count(sdrpp_ctx* c, Vfo& v) {
    Vfo::Qpsk& y = v.qpsk;
    if (!y.attached) { return fail(c, SDRPP_ERR_INVALID, kNoQpsk, v.id); }
    if (!y.on || !y.ran || y.npush <= 0) { return 0; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int cnt[kGroupMax] = {};
    HIPCHK(c, hipMemcpy(cnt, y.st[3].data, (size_t)std::min(y.npush, kGroupMax) * sizeof(int), hipMemcpyDeviceToHost));
    int total = 0;
    for (int j = 0; j < std::min(y.npush, kGroupMax); j++) { total += cnt[j]; }
    return std::min(total, y.cap);
}

// ---- read-out -----------------------------------------------------------------------------------------------------------------------
// A pipelined back-end launch whose wavefronts gave up waiting for each other (never seen; a hang would be worse) counted that in THIS context's
// page-locked word.  Called wherever the host has just synchronised with the stream and is about to hand out results.
int pipe_timeouts_check(sdrpp_ctx* c) {
    if (!c->pipe_launched || !c->h_tick_flag) { return SDRPP_OK; }
    c->pipe_launched = false;
    const int n = *(const volatile int*)(c->h_tick_flag + 8);
    if (n != c->timeouts_seen) {
        const int d = n - c->timeouts_seen;
        c->timeouts_seen = n;
        return fail(c, SDRPP_ERR_HIP, "pipelined back end: %d wavefront waits timed out (results of the last pushes are invalid)", d);
    }
    return SDRPP_OK;
}

// What the last push left in one of the context's output buffers: a VFO's stream (delivered) or the pre-processing chain's output.  `ok` false: there is
// no such output, and the read-out call refuses with its family's own message (`missing`, a format for the id).
struct OutBuf { const float* data; int n; bool ok; };
OutBuf out_of(const Stream* s) { return s ? OutBuf{ s->data, s->n, true } : OutBuf{ nullptr, 0, false }; }
OutBuf out_of_preproc(const sdrpp_ctx* c) { return c->pre.on ? OutBuf{ c->pre.last, c->pre.last_n, true } : OutBuf{ nullptr, 0, false }; }
// the RDS branch's output of the most recent push (nothing while it is switched off)
const char* const kNoRds = "VFO %d has no RDS branch";
OutBuf out_of_rds(const Vfo& v) {
    const Vfo::Rds& r = v.rds;
    if (!r.attached) { return OutBuf{ nullptr, 0, false }; }
    const Stream& s = r.st[(size_t)r.i_last];
    return OutBuf{ s.data, (r.on && r.ran) ? s.n : 0, true };
}
const char* const kNoAf = "VFO %d has no AF chain";
const char* const kNoIfc = "VFO %d has no active IF chain";
const char* const kNoPreproc = "no pre-processing chain configured";  // (takes no id)
const char* const kNoOut = "VFO %d has no output stream";                 // (never seen: what a VFO delivers and its IF stream always exist)
int out_count(sdrpp_ctx* c, OutBuf o, const char* missing, int id) {
    if (!o.ok) { return fail(c, SDRPP_ERR_INVALID, missing, id); }
    return o.n;
}
// min(max, n) complex samples to the host.  pipe_check: off for the pre-processing chain's output, which the pipelined back end never writes.
int out_read(sdrpp_ctx* c, OutBuf o, const char* missing, int id, float* dst, int max, bool pipe_check) {
    if (!o.ok) { return fail(c, SDRPP_ERR_INVALID, missing, id); }
    const int n = std::min(max, o.n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = pipe_check ? pipe_timeouts_check(c) : SDRPP_OK) { return rc; }
    if (n > 0) { HIPCHK(c, hipMemcpy(dst, o.data, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost)); }
    return n;
}
int out_hand(sdrpp_ctx* c, OutBuf o, const char* missing, int id, const float** data, int* n) {
    if (!o.ok) { return fail(c, SDRPP_ERR_INVALID, missing, id); }
    if (data) { *data = o.data; }
    if (n) { *n = o.n; }
    return SDRPP_OK;
}

// ---- sink-side sample packing ----------------------------------------------------------------------------------
int pack_scratch(sdrpp_ctx* c, size_t bytes) {
    if (bytes <= c->pack_cap) { return SDRPP_OK; }
    dev_free(c->d_pack);
    c->pack_cap = 0;
    int rc = dev_alloc(c, &c->d_pack, bytes + 1024);
    if (rc) { return rc; }
    c->pack_cap = bytes + 1024;
    return SDRPP_OK;
}
// nv floats at `src` -> int16 (pcm_type 1) / int8 (0) at `dst`, on the context's stream
void pack_convert(sdrpp_ctx* c, const float* src, long long nv, float scale, int pcm_type, void* dst) {
    const dim3 grid((unsigned)std::min<long long>((nv + 255) / 256, 4096));
    if (pcm_type == 1) { hipLaunchKernelGGL(pack_convert_kernel<int16_t>, grid, dim3(256), 0, c->stream, src, scale, nv, (int16_t*)dst); }
    else { hipLaunchKernelGGL(pack_convert_kernel<int8_t>, grid, dim3(256), 0, c->stream, src, scale, nv, (int8_t*)dst); }
}
// the first min(max, count) complex samples at `src`, converted on the device so that the copy to the host carries 4 (2) bytes per sample
int pcm_read(sdrpp_ctx* c, const float* src, int count, int pcm_type, float scale, void* dst_host, int max) {
    const int n = std::min(max, count);
    if (n == 0) { return 0; }
    const long long nv = (long long)n * 2;
    const size_t esz = pcm_type == 1 ? 2 : 1;
    if (int rc = pack_scratch(c, (size_t)nv * esz)) { return rc; }
    pack_convert(c, src, nv, scale, pcm_type, c->d_pack);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = pipe_timeouts_check(c)) { return rc; }
    HIPCHK(c, hipMemcpy(dst_host, c->d_pack, (size_t)nv * esz, hipMemcpyDeviceToHost));
    return n;
}

// ---- recorder sink (misc_modules/recorder) ------------------------------------------------------------------------------------------
// sdrpp_vfo_set_rec on a VFO the caller has looked up: parameters only — the sink has no state and plans nothing by itself
int rec_apply(sdrpp_ctx* c, Vfo& v, const sdrpp_rec_desc* d) {
    if (!d) {
        v.rec = Vfo::Rec{};
        return SDRPP_OK;
    }
    if (v.d.demod == SDRPP_DEMOD_RAW || v.i_out < 0) { return fail(c, SDRPP_ERR_UNSUPPORTED, "the recorder sink needs a demodulating VFO"); }
    if (d->sample_type == SDRPP_REC_INT32) { return fail(c, SDRPP_ERR_UNSUPPORTED, "recorder sample type INT32: the reference's own conversion overflows where it clips"); }
    if (d->sample_type != SDRPP_REC_UINT8 && d->sample_type != SDRPP_REC_INT16 && d->sample_type != SDRPP_REC_FLOAT32) { return fail(c, SDRPP_ERR_INVALID, "recorder sample type %d", d->sample_type); }
    v.rec.on = true;
    v.rec.volume = d->volume;
    v.rec.gain = powf(d->volume, 2);  // audio/volume.h:14,22
    v.rec.mono = d->mono != 0;
    v.rec.type = d->sample_type;
    v.rec.ignore_silence = d->ignore_silence != 0;
    return SDRPP_OK;
}
// sdrpp_vfo_rec_read: the stream's most recent block through the sink, converted on the device so that the copy carries the file's bytes
int rec_read(sdrpp_ctx* c, Vfo& v, void* dst_host, int max_frames, sdrpp_rec_info* info) {
    if (!v.rec.on) { return fail(c, SDRPP_ERR_INVALID, "VFO %d has no recorder sink", v.id); }
    const Stream& s = result_stream(v);
    const size_t bpf = rec_frame_bytes(v.rec), info_off = ((size_t)s.n * bpf + 15) & ~(size_t)15;
    if (int rc = pack_scratch(c, info_off + kRecInfoStride)) { return rc; }
    const ResRec q{ s.data, s.n, 0, info_off, v.rec.gain, v.rec.mono, v.rec.type, v.rec.ignore_silence, 0 };
    hipLaunchKernelGGL(vfo_rec_kernel, dim3(1), dim3(256), 0, c->stream, rec_job(q, c->d_pack));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = pipe_timeouts_check(c)) { return rc; }
    const int n = std::min(max_frames, s.n);
    if (n > 0) { HIPCHK(c, hipMemcpy(dst_host, c->d_pack, (size_t)n * bpf, hipMemcpyDeviceToHost)); }
    if (info) { HIPCHK(c, hipMemcpy(info, c->d_pack + info_off, sizeof(sdrpp_rec_info), hipMemcpyDeviceToHost)); }
    return n;
}

}  // namespace
