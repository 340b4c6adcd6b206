// One ordinary pass: snapshot / restore of the streaming state (a block happens completely or not at all), reference-block bounds, push_common.
// Part of the one translation unit sdrpp_gpu.hip (included there, in order; not a stand-alone header).
#pragma once

namespace {

// ---- streaming state that planning a block changes, for roll-back: a block either happens completely or not at all ----------------------
struct PlanSnapshot {
    struct V { RateChain::Pos pos, af_pos, rds_pos; double phi, phi2; long long seen; int i_if, lvl_if, lvl_out, lvl_af, lvl_ifc; size_t nrecs;
               int af_last, af_state;
               int rds_lvl; double rds_phi; bool rds_frozen, rds_ran; int rds_line_cur, rds_line_fed; bool stereo_ran;
               bool sym_ran; int sym_cur, sym_lvl, sym_n_if, sym_npush, sym_cap;
               bool frame_ran; int frame_lvl, frame_npush, frame_cap;
               bool rdsd_ran; int rdsd_lvl, rdsd_n_in, rdsd_npush, rdsd_cap;
               bool qpsk_ran; int qpsk_cur, qpsk_lvl, qpsk_n_in, qpsk_npush, qpsk_cap; };
    std::vector<V> v;
    std::vector<int> nc;  // n and cur of every stream of every VFO (its own, then its RDS branch's, its stereo branch's, its symbol branch's, its RDS demodulator's, its QPSK demodulator's and its framer's), in the order of the walk
    int64_t fft_pos, fft_next;
    int n_lines, iq_cur, wf_cur, wf_lines;
    bool wf_have;
    RateChain::Pos pre_pos;
    int pre_state, pre_raw_cur, pre_cur[SDRPP_MAX_DECIM_STAGES];
};
// `rotate`: pipelined mode — every stream of the VFO moves on to its next ring buffer in the same walk (stream_rotate)
void plan_snapshot(sdrpp_ctx* c, PlanSnapshot& S, bool rotate = false) {
    S.v.resize(c->vfo_list.size());
    S.nc.clear();
    for (size_t i = 0; i < c->vfo_list.size(); i++) {
        Vfo& v = *c->vfo_list[i];
        PlanSnapshot::V& q = S.v[i];
        q.pos = v.rate.pos; q.af_pos = v.af.rate.pos; q.rds_pos = v.rds.rate.pos;
        q.phi = v.phi; q.phi2 = v.phi2; q.seen = v.seen; q.i_if = v.i_if; q.lvl_if = v.lvl_if; q.lvl_out = v.lvl_out; q.lvl_af = v.lvl_af; q.lvl_ifc = v.lvl_ifc;
        q.nrecs = v.recs.size();
        q.af_last = v.af.i_last; q.af_state = v.af.state_cur;
        q.rds_lvl = v.rds.lvl; q.rds_phi = v.rds.phi; q.rds_frozen = v.rds.frozen; q.rds_ran = v.rds.ran; q.rds_line_cur = v.rds.line_cur; q.rds_line_fed = v.rds.line_fed; q.stereo_ran = v.stereo.ran;
        q.frame_ran = v.frame.ran; q.frame_lvl = v.frame.lvl; q.frame_npush = v.frame.npush; q.frame_cap = v.frame.cap;
        q.sym_ran = v.sym.ran; q.sym_cur = v.sym.cur; q.sym_lvl = v.sym.lvl; q.sym_n_if = v.sym.n_if; q.sym_npush = v.sym.npush; q.sym_cap = v.sym.cap;
        q.rdsd_ran = v.rdsd.ran; q.rdsd_lvl = v.rdsd.lvl; q.rdsd_n_in = v.rdsd.n_in; q.rdsd_npush = v.rdsd.npush; q.rdsd_cap = v.rdsd.cap;
        q.qpsk_ran = v.qpsk.ran; q.qpsk_cur = v.qpsk.cur; q.qpsk_lvl = v.qpsk.lvl; q.qpsk_n_in = v.qpsk.n_in; q.qpsk_npush = v.qpsk.npush; q.qpsk_cap = v.qpsk.cap;
        for_each_stream(v, [&](Stream& st) {
            S.nc.push_back(st.n);
            S.nc.push_back(st.cur);
            if (rotate) { stream_rotate(st); }
        });
    }
    S.fft_pos = c->fft_pos; S.fft_next = c->fft_next; S.n_lines = c->n_lines; S.iq_cur = c->iq_cur;
    S.wf_cur = c->wf.cur; S.wf_lines = c->wf.lines; S.wf_have = c->wf.have_latest;
    S.pre_pos = c->pre.rate.pos;
    S.pre_state = c->pre.state_cur;
    S.pre_raw_cur = c->pre.raw.cur;
    for (size_t k = 0; k < c->pre.st.size() && k < SDRPP_MAX_DECIM_STAGES; k++) { S.pre_cur[k] = c->pre.st[k].cur; }
}
// (retune records a plan has dropped stay dropped: they were out of every window's reach)
void plan_restore(sdrpp_ctx* c, const PlanSnapshot& S) {
    const int* nc = S.nc.data();
    for (size_t i = 0; i < c->vfo_list.size(); i++) {
        Vfo& v = *c->vfo_list[i];
        const PlanSnapshot::V& q = S.v[i];
        v.rate.pos = q.pos; v.af.rate.pos = q.af_pos; v.rds.rate.pos = q.rds_pos;
        v.phi = q.phi; v.phi2 = q.phi2; v.seen = q.seen; v.i_if = q.i_if; v.lvl_if = q.lvl_if; v.lvl_out = q.lvl_out; v.lvl_af = q.lvl_af; v.lvl_ifc = q.lvl_ifc;
        v.af.i_last = q.af_last; v.af.state_cur = q.af_state;
        v.rds.lvl = q.rds_lvl; v.rds.phi = q.rds_phi; v.rds.frozen = q.rds_frozen; v.rds.ran = q.rds_ran; v.rds.line_cur = q.rds_line_cur; v.rds.line_fed = q.rds_line_fed; v.stereo.ran = q.stereo_ran;
        v.frame.ran = q.frame_ran; v.frame.lvl = q.frame_lvl; v.frame.npush = q.frame_npush; v.frame.cap = q.frame_cap;
        v.sym.ran = q.sym_ran; v.sym.cur = q.sym_cur; v.sym.lvl = q.sym_lvl; v.sym.n_if = q.sym_n_if; v.sym.npush = q.sym_npush; v.sym.cap = q.sym_cap;
        v.rdsd.ran = q.rdsd_ran; v.rdsd.lvl = q.rdsd_lvl; v.rdsd.n_in = q.rdsd_n_in; v.rdsd.npush = q.rdsd_npush; v.rdsd.cap = q.rdsd_cap;
        v.qpsk.ran = q.qpsk_ran; v.qpsk.cur = q.qpsk_cur; v.qpsk.lvl = q.qpsk_lvl; v.qpsk.n_in = q.qpsk_n_in; v.qpsk.npush = q.qpsk_npush; v.qpsk.cap = q.qpsk_cap;
        for_each_stream(v, [&](Stream& st) {
            st.n = *nc++;
            st.cur = *nc++;
        });
    }
    c->fft_pos = S.fft_pos; c->fft_next = S.fft_next; c->n_lines = S.n_lines; c->iq_cur = S.iq_cur;
    c->wf.cur = S.wf_cur; c->wf.lines = S.wf_lines; c->wf.have_latest = S.wf_have;
    c->meters.out_lines = 0;  // (the meters' output array may have been overwritten: it holds no push's lines now)
    c->pre.rate.pos = S.pre_pos;
    c->pre.state_cur = S.pre_state;
    c->pre.raw.cur = S.pre_raw_cur;
    for (size_t k = 0; k < c->pre.st.size() && k < SDRPP_MAX_DECIM_STAGES; k++) { c->pre.st[k].cur = S.pre_cur[k]; }
}

void block_bounds(sdrpp_ctx* c, int64_t count, const std::vector<int>* push_ends) {
    c->arena_begins++;
    c->arena_allocs = 0;
    // the reference's blocks inside this push (sdrpp_set_reference_block): ends as cumulative sample counts
    // every push is at least one block of its own; with a reference block size it is cut further
    std::vector<int>& B = c->vfo_bounds;
    B.clear();
    const std::vector<int> whole{ (int)count };
    int64_t lo = 0;
    for (int e : (push_ends ? *push_ends : whole)) {
        if (c->ref_block > 0) {
            for (int64_t q = lo + c->ref_block; q < e; q += c->ref_block) { B.push_back((int)q); }
        }
        if (e > lo || B.empty()) { B.push_back(e); }
        lo = e;
    }
}
int iq_hist_need(sdrpp_ctx* c) {
    int need_hist = 1;
    if (c->fft_on) { need_hist = std::max(need_hist, c->nz - 1); }
    for (auto& kv : c->vfos) {
        const RateChain& R = kv.second->rate;
        if (R.n_stages > 0) { need_hist = std::max(need_hist, R.ntaps(0) - 1); }
        if (R.n_stages > 1) { need_hist = std::max(need_hist, R.ntaps(0) - 1 + R.decim_s[0] * (R.ntaps(1) - 1)); }  // fused front
    }
    return need_hist;
}
// what the NEXT push can reach back to: the samples of the frame in progress and the deepest stage-1 (+ fused stage-2) window
CarryJob iq_carry_job(sdrpp_ctx* c, const float* d_iq, int64_t count) {
    int need = 1;
    if (c->fft_on) {
        const int64_t P = (int64_t)c->nz + c->skip;
        const int64_t partial = c->fft_pos - c->fft_next * P;  // do_fft already advanced both
        if (partial > 0) { need = std::max(need, (int)std::min<int64_t>(partial, c->nz - 1)); }
    }
    for (auto& kv : c->vfos) {
        const RateChain& R = kv.second->rate;
        if (R.n_stages > 0) { need = std::max(need, R.ntaps(0) - 1); }
        if (R.n_stages > 1) { need = std::max(need, R.ntaps(0) - 1 + R.decim_s[0] * (R.ntaps(1) - 1)); }
    }
    need = std::min(need, c->iq_hist_cap);
    return CarryJob{ d_iq, c->iq_hist[c->iq_cur], c->iq_hist[c->iq_cur ^ 1], c->iq_hist_cap, (int)count, 2, need };
}

// `push_ends`: cumulative ends of the pushes a deferred pass combines (nullptr: the pass is one push)
int push_common(sdrpp_ctx* c, const float* d_iq, int64_t count, const std::vector<int>* push_ends = nullptr) {
    if (count == 0) {  // an empty block produces nothing (and changes no state)
        c->n_lines = 0;
        for (auto& kv : c->vfos) {
            for_each_stream(*kv.second, [](Stream& s) { s.n = 0; });
        }
        return SDRPP_OK;
    }
    int rc0;
    {
        HostScope hs("arena_begin (backpressure)");
        rc0 = arena_begin(c);
    }
    if (rc0) { return rc0; }
    static thread_local PlanSnapshot snap;  // (re-used: a fresh one is two allocations per block, tens of KB with 128 VFOs; a nested pass starts only after the outer plan has been restored)
    plan_snapshot(c, snap);
    c->plan_lvl0 = 0;
    block_bounds(c, count, push_ends);
    if (c->pre.on) {
        rc0 = run_preproc(c, &d_iq, &count);
        if (rc0) {
            plan_restore(c, snap);
            return rc0;
        }
        if (count == 0) {  // the decimator swallowed the whole block (offset carried): nothing reaches the FFT / VFOs
            c->n_lines = 0;
            for (auto& kv : c->vfos) {
                for_each_stream(*kv.second, [](Stream& s) { s.n = 0; });
            }
            return arena_end(c);
        }
    }
    int rc = ensure_iq_hist(c, iq_hist_need(c));
    if (rc) {
        plan_restore(c, snap);
        return rc;
    }
    IqSrc src{ (const float2*)d_iq, (const float2*)c->iq_hist[c->iq_cur], c->iq_hist_cap, (long long)count };
    // fork: the FFT branch goes to its own stream and overlaps the VFO bank; both only read the IQ buffers
    // (a push that completes no frame launches nothing on the FFT branch: no fork / join either — each costs the main stream 5-9 us, and at
    // the reference's block size every fourth push of a 65 536-point waterfall is such a push)
    bool fft_work = false;
    if (c->fft_on) {
        const int64_t P = (int64_t)c->nz + c->skip;
        fft_work = (c->fft_pos + count) - c->nz - c->fft_next * P >= 0;
    }
    const bool fork = fft_work && !c->vfos.empty();
    if (fork) {
        HostScope hs("fork events");
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->fft_stream, c->ev_fork, 0));
        c->launch_stream = c->fft_stream;
    }
    {
        HostScope hs("do_fft");
        rc = do_fft(c, src, count);
    }
    c->launch_stream = c->stream;
    if (fork) { (void)hipEventRecord(c->ev_join, c->fft_stream); }
    if (!rc) {
        const CarryJob iqc = iq_carry_job(c, d_iq, count);
        if (c->vfos.empty()) {
            std::vector<CarryJob> carry{ iqc };
            CarryJob* d_carry = arena_push(c, carry);
            rc = arena_commit(c);
            if (!rc) {
                FamilyTimer t(c, F_MISC);
                const int iq_elems = carry[0].need * 2;
                launch(c, carry_kernel, dim3((unsigned)std::max(1, std::min((iq_elems + 8191) / 8192, 512)), 1), dim3(256), 0, (const CarryJob*)d_carry, 0);  // (carry_body: 8 192 floats per workgroup and round)
            }
        }
        else {
            HostScope hs("do_vfos");
            rc = do_vfos_plan(c, src, count, iqc);
        }
    }
    HostScope hs2("join + arena_end");
    if (fork) { (void)hipStreamWaitEvent(c->stream, c->ev_join, 0); }  // (also after a failure: the FFT branch's launches must not overtake what follows)
    if (rc) {
        // the block did not happen: the streaming state is what it was before the push (what the kernels launched so far wrote is never
        // looked at: counts, history sides and frame positions are the host's)
        plan_restore(c, snap);
        (void)arena_end(c);
        return rc;
    }
    c->iq_cur ^= 1;
    rc = arena_end(c);
    if (rc) { return rc; }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { return fail(c, SDRPP_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e)); }
    return SDRPP_OK;
}

}  // namespace
