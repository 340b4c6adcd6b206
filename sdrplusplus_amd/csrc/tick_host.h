// Pipelined execution, host side (tick_kernels.h): role queue, one launch per block, result slots, drain.
// Part of the one translation unit sdrpp_gpu.hip (included there, in order; not a stand-alone header).
#pragma once

namespace {

// =====================================================================================================================
// Pipelined execution (tick_kernels.h): queue, launch, drain
// =====================================================================================================================
void tick_wait_done(sdrpp_ctx* c, uint64_t nticks) {
    if (!c->h_tick_flag) { return; }
    // the flag holds the number of completed ticks modulo 2^32; at most kArenaSlots ticks are ever outstanding
    const volatile unsigned* f = c->h_tick_flag;
    long spins = 0;
    while ((int)((unsigned)nticks - *f) > 0) {
        if (++spins > 2000) { std::this_thread::yield(); }
        if (spins > 40000000) {  // ~minutes: the device is gone; let the next HIP call report it
            (void)hipStreamSynchronize(c->stream);
            if ((int)((unsigned)nticks - *f) > 0) { return; }
        }
    }
}
// An event behind everything launched so far (c->ticks), from the ring.  `pre`: only reserve the ring entry and return it — the caller hands
// the event to the launch itself (hipExtLaunchKernelGGL's stop event).
hipEvent_t tick_event_take(sdrpp_ctx* c, uint64_t behind_tick) {
    const int k = c->tick_ev_next;
    c->tick_ev_next = (k + 1) % sdrpp_ctx::kTickEvents;
    tick_ev_resolve(c, k);  // (the launch it timed is kTickEvents ticks old: long complete)
    if (!c->tick_ev[k] && hipEventCreate(&c->tick_ev[k]) != hipSuccess) { return nullptr; }
    c->tick_ev_tick[k] = behind_tick;
    c->tick_ev_last = behind_tick;
    return c->tick_ev[k];
}
// The results tick `nticks` wrote into page-locked host memory are visible to this thread: 1 yes, 0 not yet (wait = false), < 0 error.
// The flag first (cheap: a cached word the device writes once per tick), then the first event recorded at or behind that tick — a later
// tick's event orders the earlier tick's writes just as well; if there is none yet, one is recorded now behind everything launched.
int tick_results_visible(sdrpp_ctx* c, uint64_t nticks, bool wait) {
    if (nticks == 0) { return 1; }
    if (wait) { tick_wait_done(c, nticks); }
    else if (c->h_tick_flag && (int)((unsigned)nticks - *(const volatile unsigned*)c->h_tick_flag) > 0) { return 0; }
    int best = -1;
    for (int k = 0; k < sdrpp_ctx::kTickEvents; k++) {
        if (c->tick_ev[k] && c->tick_ev_tick[k] >= nticks && (best < 0 || c->tick_ev_tick[k] < c->tick_ev_tick[best])) { best = k; }
    }
    hipEvent_t ev = best >= 0 ? c->tick_ev[best] : nullptr;
    if (!ev) {
        ev = tick_event_take(c, c->ticks);
        if (!ev || hipEventRecord(ev, c->stream) != hipSuccess) { return fail(c, SDRPP_ERR_HIP, "hipEventRecord failed"); }
    }
    long spins = 0;
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) { return 1; }
        if (e != hipErrorNotReady) { return fail(c, SDRPP_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e)); }
        if (!wait) { return 0; }
        if (++spins > 200) { std::this_thread::yield(); }
    }
}
bool tick_is_done(const sdrpp_ctx* c, uint64_t nticks) { return !c->h_tick_flag || (int)((unsigned)nticks - *(const volatile unsigned*)c->h_tick_flag) <= 0; }

// One tick: level-0 work of the block that arrives with it (`land`: its landing copy, may be null; the arena slot the caller has filled
// with the block's job tables) + every queued role whose turn it is.  The role table of the NEXT tick is appended to the arena slot and
// travels with this tick's upload.
// expected lifetime of a workgroup of a role relative to the others (tools/tick_trace.py timelines), for the order inside a tick
inline int tick_role_weight(int role, bool crowded) {
    if (role == TR_ROTX16) { return 120; }  // the reference's rotator recursion over the whole block: milliseconds — it IS the tick, everything else runs in its shadow
    // result copies write page-locked host memory over the bus: few workgroups whose life is mostly that round trip — started last they are the
    // tail of the tick, started first they finish in its shadow
    if (role == TR_COPY) { return 110; }
    // FFT pass 1: since its workgroups walk their tiles and take the lean loader they live ~12 us at 10^6-sample blocks, shorter than the
    // Toeplitz roles' 17-33 us.  In a CROWDED tick (more workgroups than the GPU holds at once: they are handed out in index order) they go
    // behind the filters and pass 2, so that the tick ends on short workgroups: 18.6 -> 19.6 GS/s at 10^6-sample blocks; in a tick whose
    // workgroups are all resident from the start the order only decides who gets going first, and pass 1 early is worth 2 % at 200 000-sample
    // blocks (profiles/r03z_tick_p1_weight.log)
    if (role >= TR_FFT_P1_5 && role <= TR_FFT_P1_10) { return crowded ? 45 : 70; }
    // the long first stages (cfg 4): far more workgroups than the GPU holds, 58 us each — behind the sequential recursions (few, long), in front
    // of everything else: with four tile engines per workgroup they are 60 % of the tick's workgroup time, and started late they ARE its tail
    // (weight 72 against 58: 10^6-sample blocks 6.02 -> 6.13 GS/s, 307 200: 3.19 -> 3.78; behind the filters, 40 / 15: 5.77 / 5.64 and 3.11 / 3.07;
    // profiles/r04w_fcl_weight.log — with two engines per workgroup, round 3, the order hardly mattered: profiles/r03zj_*)
    switch (role) {
    case TR_FCL_0: case TR_FCL_PF: return 72;
    case TR_FCM_132_4: case TR_FCM_6: case TR_FCM_10: case TR_FCM_16: case TR_FCM16_132_4: case TR_S1_1: case TR_S1D_1: case TR_F2_1: return 90;
    case TR_SEQ: case TR_SSBX: case TR_IFC: return 85;  // (one wavefront per VFO walking its whole block: few and long)
    case TR_FIRB_C: case TR_FIRB_R: case TR_FIRB_S: case TR_FIRB_Q: return 70;
    case TR_POLYC: return 55;
    case TR_DEEMP_P1: case TR_DC_P1: return 52;
    case TR_DEEMP_P0: case TR_DC_P0: return 48;
    case TR_TOEP_Q: return 65;
    case TR_TOEP_C: case TR_TOEP_R: case TR_FFT_S10: case TR_FFT_S11: case TR_FFT_S12: return 60;
    case TR_FFT_P2_7: case TR_FFT_P2_8: case TR_FFT_P2_9: case TR_FFT_P2_10: case TR_FFT_P2ROW: return 50;
    case TR_FFT_TR: return 25;
    case TR_ROT: case TR_PRE: return 30;
    case TR_ZOOM_16: case TR_ZOOM_4: case TR_ZOOM_1: return 20;
    default: return 10;  // carry, copies
    }
}
int tick_launch(sdrpp_ctx* c, const CopyJob* land) {
    std::vector<sdrpp_ctx::RoleLaunch> now;
    if (!c->tickq.empty()) {
        now.swap(c->tickq.front());
        c->tickq.pop_front();
    }
    if ((int)now.size() != c->next_tab_n) { return fail(c, SDRPP_ERR_HIP, "internal: tick table out of step (%zu roles queued, %d uploaded)", now.size(), c->next_tab_n); }
    // the table of the tick after this one
    TickTable* tab_dev_next = nullptr;
    int tab_n_next = 0;
    if (!c->tickq.empty() && !c->tickq.front().empty()) {
        std::vector<sdrpp_ctx::RoleLaunch>& nx = c->tickq.front();
        // The roles of a tick are independent of each other, so their order is free — and the hardware hands out workgroups in index
        // order: longest workgroups first (front ends, FFT pass 1, the filters; zoom / carry / copies last), so that the tick ends on
        // short ones instead of on a front end that only got its turn when everything else was through (10^6-sample blocks: the front
        // end started 46 us into an 81 us tick).  The table is final here: later blocks only add to later ticks.
        long long wgs = 0;
        for (auto& r : nx) { wgs += (long long)r.e.gx * r.e.gy; }
        const bool crowded = wgs > 3ll * c->num_cus;  // (three workgroups of the tick kernel per CU)
        std::stable_sort(nx.begin(), nx.end(), [crowded](const sdrpp_ctx::RoleLaunch& a, const sdrpp_ctx::RoleLaunch& b) { return tick_role_weight(a.e.role, crowded) > tick_role_weight(b.e.role, crowded); });
        if (nx.size() > SDRPP_TICK_MAX_ENTRIES) { return fail(c, SDRPP_ERR_UNSUPPORTED, "internal: %zu roles in one tick", nx.size()); }
        const size_t off = (c->arena_off + 63) & ~(size_t)63;
        if (off + sizeof(TickTable) > kArenaBytes) { return fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }
        TickTable* T = reinterpret_cast<TickTable*>(c->arena_host[c->arena_slot] + off);
        T->n = (int)nx.size();
        int total = 0;
        for (size_t i = 0; i < nx.size(); i++) {
            total += nx[i].e.gx * nx[i].e.gy;
            T->block_end[i] = total;
            T->e[i] = nx[i].e;
        }
        c->arena_off = off + offsetof(TickTable, e) + nx.size() * sizeof(TickEntry);
        tab_dev_next = reinterpret_cast<TickTable*>(c->arena_dev + off);
        tab_n_next = (int)nx.size();
    }
    TickL0 l0{};
    if (land && land->bytes > 0) {
        l0.job[0] = *land;
        l0.blocks[0] = (int)std::max<long long>(1, std::min<long long>((land->bytes + 8191) / 8192, c->tick_land_blocks));
        // (a converting copy: a workgroup per 32 KB of SOURCE, rounded down — eight 16-byte loads per work-item, the unrolled loop's trip, from the first
        // block that has that much; the source is a quarter or half of what the verbatim copy fetches for the same samples)
        if ((land->kind & 0xff) == 4) { l0.blocks[0] = (int)std::max<long long>(1, std::min<long long>(land->bytes / 32768, c->tick_land_blocks)); }
    }
    if (c->arena_off > 0) {
        l0.job[1] = CopyJob{ c->arena_host_dev[c->arena_slot], c->arena_dev, (long long)((c->arena_off + 15) & ~(size_t)15), 0, 0 };
        l0.blocks[1] = (int)std::max<size_t>(1, std::min<size_t>((c->arena_off + 4095) / 4096, 16));  // one 16-byte load per work-item: a round trip over the bus each
    }
    int blocks = l0.blocks[0] + l0.blocks[1];
    size_t lds = 0;
    bool set1 = false;
    long long role_wgs = 0;
    bool to_host = false;
    for (auto& r : now) {
        to_host = to_host || r.to_host;
        blocks += r.e.gx * r.e.gy;
        role_wgs += (long long)r.e.gx * r.e.gy;
        lds = std::max(lds, r.lds);
        set1 = set1 || r.e.role == TR_FCL_PF || r.e.role == TR_FCM_6 || r.e.role == TR_FCM_10 || r.e.role == TR_FCM_16;  // (roles that exist in the 247-register build only: tick_kernels.h)
        if (r.e.role >= 0 && r.e.role < 64) { c->stat_role_wgs[r.e.role] += (int64_t)r.e.gx * r.e.gy; }
    }
    if (role_wgs > 3ll * c->num_cus) { c->stat_crowded++; }
    {   // where the stage-0 copies stand among the tick's workgroups (SDRPP_GPU_TICK_L0_AT: 0 = in front (default), -1 = behind all roles, n = behind
        // the first n role workgroups): a switch for the measurement DESIGN_HISTORY.md 4b names as the next step
        const int l0_at = c->tick_l0_at;
        const int role_blocks = blocks - l0.blocks[0] - l0.blocks[1];
        l0.first = l0_at < 0 ? role_blocks : std::min(l0_at, role_blocks);
    }
    if (blocks == 0) {  // nothing to do at all: a level of the queue without roles (an idle flush; a gap between a block's levels)
        c->next_tab = tab_dev_next;
        c->next_tab_n = tab_n_next;
        // No launch, so the tick counter the device publishes does not move — but every block still in the queue has just advanced by one level:
        // a block's completion tick was computed as "ticks now + its remaining levels", one COUNTED tick per level, and would lie one launch past
        // the end of the drain for every empty level (sdrpp_result_wait: "block cannot complete").  Its remaining levels are one fewer now.
        for (auto& R : c->res) {
            if (R.ticket != 0 && R.done_tick > c->ticks) { R.done_tick--; }
        }
        return SDRPP_OK;
    }
    c->tick_target += (unsigned)blocks;
    c->ticks++;
    TickDone done{ c->d_tick_counter, c->hd_tick_flag, c->tick_target, (unsigned)c->ticks };
    hipEvent_t stop_ev = nullptr;
    const TickTable* tab = c->next_tab_n > 0 ? c->next_tab : c->empty_tab;
    {
        // Completion events ride on the launch itself (hipExtLaunchKernelGGL's start / stop events: the dispatch packet's own signal, no packet
        // of their own in the queue): the stop event orders the tick's result writes for the host (host_ctx.h), start + stop time the launch.
        const bool timed = c->timing && ((c->timing_mask >> F_TICK) & 1u);
        c->fam_launch[F_TICK]++;
        hipEvent_t ea = nullptr;
        if (timed || to_host) {
            const int k = c->tick_ev_next;
            stop_ev = tick_event_take(c, c->ticks);
            if (!stop_ev) { return fail(c, SDRPP_ERR_HIP, "hipEventCreate failed"); }
            if (timed) {
                ea = get_event(c);
                c->tick_ev_start[k] = ea;
            }
        }
        HostScope hs("launch");
        if (stop_ev) {
            if (set1) { hipExtLaunchKernelGGL((tick_kernel<1>), dim3((unsigned)blocks), dim3(256), (unsigned)lds, c->stream, ea, stop_ev, 0, l0, tab, done); }
            else { hipExtLaunchKernelGGL((tick_kernel<0>), dim3((unsigned)blocks), dim3(256), (unsigned)lds, c->stream, ea, stop_ev, 0, l0, tab, done); }
        }
        else if (set1) { hipLaunchKernelGGL((tick_kernel<1>), dim3((unsigned)blocks), dim3(256), lds, c->stream, l0, tab, done); }
        else { hipLaunchKernelGGL((tick_kernel<0>), dim3((unsigned)blocks), dim3(256), lds, c->stream, l0, tab, done); }
    }
    c->arena_tick[c->arena_slot] = c->ticks;
    c->next_tab = tab_dev_next;
    c->next_tab_n = tab_n_next;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { return fail(c, SDRPP_ERR_HIP, "tick launch failed: %s", hipGetErrorString(e)); }
    return SDRPP_OK;
}
// run every queued role (no new input): what a caller that wants the results of the last blocks NOW pays for the skew
int tick_drain(sdrpp_ctx* c) {
    while (!c->tickq.empty()) {
        int rc = arena_begin(c);
        if (rc) { return rc; }
        rc = tick_launch(c, nullptr);
        if (rc) { return rc; }
    }
    return SDRPP_OK;
}

// Can this context's blocks run as ticks at all?  (What can only be seen while planning — a VFO group too small for the matrix front end,
// a filter without the matrix form, more frames than one scratch chunk — aborts the plan instead.)
bool tick_eligible(sdrpp_ctx* c) {
    if ((c->pre.on && c->pre.ref_order) || c->deferred) { return false; }  // (the reference-order arithmetic of the pre-processing chain has no roles)
    for (auto& kv : c->vfos) {
        const Vfo& v = *kv.second;
        // (reference-rotator VFOs have their roles since round 5 — TR_ROTX16 / TR_FIRD / TR_SSBX; its one-wavefront form has not)
        if ((v.nco_exact && c->rot_exact_single) || !v.recs.empty() || v.st.size() > 24) { return false; }
    }
    return true;
}

// ---- results of a block in page-locked host memory (sdrpp_set_pipelined's result flags): gather roles one level behind the producers ----
// What result flag 1 delivers per VFO: the end of its chain — the AF chain's output where one is attached (what the radio module's audio
// stream carries, radio_module.h:98-110), else the demodulator's, else (no demodulator) the IF stream — and the level it is written at.
const Stream& result_stream(const Vfo& v, int* level = nullptr) {
    if (v.af.on && v.af.i_last >= 0 && v.d.demod != SDRPP_DEMOD_RAW) {
        if (level) { *level = v.lvl_af; }
        return v.st[(size_t)v.af.i_last];
    }
    const bool raw = v.d.demod == SDRPP_DEMOD_RAW;
    if (raw && v.ifc.active() && v.i_ifc >= 0 && v.st[(size_t)v.i_ifc].base) {  // a RAW VFO behind an IF chain: the chain's output
        if (level) { *level = v.lvl_ifc; }
        return v.st[(size_t)v.i_ifc];
    }
    if (level) { *level = raw ? v.lvl_if : v.lvl_out; }
    return raw ? v.st[(size_t)v.i_if] : v.st[(size_t)v.i_out];
}
// the push ends of a launch group (Vfo::tk_if / tk_af) at the rate of the stream result_stream() names
const std::vector<int>& result_ends(const Vfo& v, const Stream& s) {
    return (&s == &v.st[(size_t)v.i_if] || (v.i_out >= 0 && &s == &v.st[(size_t)v.i_out]) || (v.i_ifc >= 0 && &s == &v.st[(size_t)v.i_ifc])) ? v.tk_if : v.tk_af;
}
constexpr size_t kRecInfoStride = 32;  // one sdrpp_rec_info per push in a result slot
static_assert(sizeof(sdrpp_rec_info) <= kRecInfoStride && sizeof(sdrpp_rec_info) == sizeof(RecInfo), "sdrpp_rec_info is what the recorder kernel writes");
inline size_t rec_frame_bytes(const Vfo::Rec& r) { return (size_t)(r.type == SDRPP_REC_UINT8 ? 1 : (r.type == SDRPP_REC_INT16 ? 2 : 4)) * (r.mono ? 1 : 2); }
size_t tick_results_need(sdrpp_ctx* c) {
    size_t need = 0;
    if (c->res_flags & 1) {
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            size_t cap = std::max(result_stream(v).cap, v.st[(size_t)v.i_if].cap);  // (which stream ends the chain can change with sdrpp_vfo_set_af: room for either)
            if (v.i_out >= 0) { cap = std::max(cap, v.st[(size_t)v.i_out].cap); }
            need += ((cap + 16) * 8 + 15) & ~(size_t)15;
        }
    }
    if (c->res_flags & 16) {  // recorder sinks: the converted block (at most 8 bytes per frame, whatever type the sink has when the block comes) + one record per push of a launch group
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            if (!v.rec.on || v.i_out < 0) { continue; }
            const size_t cap = std::max(result_stream(v).cap, v.st[(size_t)v.i_out].cap);
            need += (((cap + 16) * 8 + 15) & ~(size_t)15) + (size_t)kGroupMax * kRecInfoStride;
        }
    }
    if (c->res_flags & 32) {  // RDS branches: the 5 kS/s baseband of the block
        for (auto& kv : c->vfos) {
            const Vfo::Rds& r = kv.second->rds;
            if (r.attached && !r.st.empty()) { need += ((r.st.back().cap + 16) * 8 + 15) & ~(size_t)15; }
        }
    }
    if (c->res_flags & 64) {  // symbol branches: per-push counts, then the largest block's capacity of soft values and of bits
        for (auto& kv : c->vfos) {
            const Vfo::Sym& y = kv.second->sym;
            if (y.attached && y.st.size() == 4) { need += (size_t)kGroupMax * 4 + (((y.st[1].cap + 16) * 4 + 15) & ~(size_t)15) + ((y.st[1].cap + 16 + 15) & ~(size_t)15); }
        }
    }
    if (c->res_flags & 512) {  // framers: per-push frame counts, then the largest block's capacity of records
        for (auto& kv : c->vfos) {
            const Vfo::Frame& f = kv.second->frame;
            if (f.attached && f.st.size() == 2) { need += (size_t)kGroupMax * 4 + (((f.st[0].cap + 16) * 4 + 15) & ~(size_t)15); }
        }
    }
    if (c->res_flags & 128) {  // RDS demodulators: the symbol branch's layout
        for (auto& kv : c->vfos) {
            const Vfo::Rdsd& y = kv.second->rdsd;
            if (y.attached && y.st.size() == 3) { need += (size_t)kGroupMax * 4 + (((y.st[0].cap + 16) * 4 + 15) & ~(size_t)15) + ((y.st[0].cap + 16 + 15) & ~(size_t)15); }
        }
    }
    if (c->res_flags & 256) {  // QPSK demodulators: per-push counts, then the block's capacity of int8 pairs (2 bytes) and, where asked for, of float pairs (8 bytes)
        for (auto& kv : c->vfos) {
            const Vfo::Qpsk& y = kv.second->qpsk;
            if (y.attached && y.st.size() == 4) { need += (size_t)kGroupMax * 4 + (c->res_qpsk_soft ? (((y.st[1].cap + 16) * 8 + 15) & ~(size_t)15) : 0) + (((y.st[1].cap + 16) * 2 + 15) & ~(size_t)15); }
        }
    }
    if ((c->res_flags & 8) && c->pre.on) {
        size_t cap = c->pre.out.base ? c->pre.out.cap : 0;
        for (auto& st : c->pre.st) { cap = std::max(cap, st.cap); }
        need += ((cap + 16) * 8 + 15) & ~(size_t)15;
    }
    if (c->fft_on) {
        if ((c->res_flags & 2) && c->data_width > 0) { need += 2 * ((c->lines_cap * (size_t)c->data_width * 4 + 15) & ~(size_t)15); }
        if (c->res_flags & 4) { need += (c->lines_cap * (size_t)c->fft_size * 4 + 15) & ~(size_t)15; }
        need += (c->lines_cap * c->meters.offs.size() * 8 + 15) & ~(size_t)15;  // signal meters: no flag, every block carries them while a table is set
    }
    return need;
}
int tick_results_ensure(sdrpp_ctx* c) {
    const size_t need = tick_results_need(c);
    if (need <= c->res_cap && c->res_ring) { return SDRPP_OK; }
    // The ring grows (a VFO was added, a larger view / FFT configured) in the middle of a run: results that are complete or on their way
    // but not yet collected must survive — a host keeps tickets across such a change (IQFrontEnd: pendingTickets across tempStop / addVFO).
    // Everything queued runs to its end first, then the ring's content moves into the larger one at the same offsets; a ring of which the host
    // is holding blocks (handed out by sdrpp_result_wait) stays alive until they are released — the pointers the host was given stay valid.
    int rc = tick_drain(c);
    if (rc) { return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tick_wait_done(c, c->ticks);
    const size_t cap = need + need / 8 + 4096;
    const size_t bytes = (size_t)kResSlots * ((cap + 4095) & ~(size_t)4095);
    char* nh = nullptr;
    char* nd = nullptr;
    if (hipHostMalloc((void**)&nh, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess || hipHostGetDevicePointer((void**)&nd, nh, 0) != hipSuccess) {
        if (nh) { (void)hipHostFree(nh); }
        return fail(c, SDRPP_ERR_NOMEM, "page-locked result ring of %zu bytes", bytes);
    }
    if (c->res_ring) {
        int held = 0;
        for (auto& g : c->res_live) {
            memcpy(nh + g.off, c->res_ring + g.off, g.bytes);
            held += g.held;
        }
        for (auto& R : c->res) {  // blocks the host has not asked for yet follow their bytes into the new ring (held ones keep the address they were given)
            if (R.ticket != 0 && !R.held && R.epoch == c->res_epoch && R.base) {
                R.base = nh + (R.base - c->res_ring);
                R.epoch = c->res_epoch + 1;
            }
        }
        if (held > 0) { c->res_retired.push_back(sdrpp_ctx::ResRetired{ c->res_ring, c->res_epoch, held }); }
        else { (void)hipHostFree(c->res_ring); }
    }
    c->res_ring = nh;
    c->res_ring_dev = nd;
    c->res_ring_bytes = bytes;
    c->res_cap = cap;
    c->res_epoch++;
    return SDRPP_OK;
}
// a region of the result ring for launch group `gid`; regions the ring has come round to are taken back, oldest first (their blocks' results are
// gone: sdrpp_result_wait says so), unless the host still holds one — then nothing is touched and the push fails
int tick_results_alloc(sdrpp_ctx* c, uint64_t gid, size_t bytes, size_t* off_out) {
    const size_t need = (std::max<size_t>(bytes, 16) + 255) & ~(size_t)255;
    if (!c->res_ring || need > c->res_ring_bytes) { return fail(c, SDRPP_ERR_INVALID, "internal: results of %zu bytes, ring of %zu", need, c->res_ring_bytes); }
    size_t off = c->res_head;
    if (off + need > c->res_ring_bytes) { off = 0; }
    size_t npop = 0;
    for (size_t i = 0; i < c->res_live.size(); i++) {
        const sdrpp_ctx::ResRegion& g = c->res_live[i];
        if (g.off < off + need && off < g.off + g.bytes) { npop = i + 1; }
    }
    for (size_t i = 0; i < npop; i++) {
        if (c->res_live[i].held > 0) {
            return fail(c, SDRPP_ERR_INVALID, "results of launch group %llu are still held (%d blocks) and the result ring has come round to them: release results sooner", (unsigned long long)c->res_live[i].gid,
                        c->res_live[i].held);
        }
    }
    c->res_live.erase(c->res_live.begin(), c->res_live.begin() + (long)npop);
    c->res_live.push_back(sdrpp_ctx::ResRegion{ gid, off, need, 0 });
    c->res_head = off + need;
    *off_out = off;
    return SDRPP_OK;
}
sdrpp_ctx::ResRegion* tick_results_region(sdrpp_ctx* c, uint64_t gid) {
    for (auto it = c->res_live.rbegin(); it != c->res_live.rend(); ++it) {
        if (it->gid == gid) { return &*it; }
        if (it->gid < gid) { break; }
    }
    return nullptr;
}

// ---- what a block's results consist of: one push — or a launch group of k pushes (c->grp_ends: their cumulative ends), planned as ONE block ----
// Every VFO's output block of the group lies in the group's result slot in one piece; push j's share of it is the samples between the push ends
// carried down the VFO's chain (Vfo::tk_if / tk_af, plan_vfo.h), its lines the frames whose last sample arrived with it.
struct ResCopy { const void* src; size_t off; size_t bytes; int level; };
struct ResMeter { int n_lines = 0, n = 0; size_t off = 0; int level = 0; };  // the signal meters of the block's lines (n == 0: none)
struct ResRec { const float* src; int n; size_t off, info_off; float gain; int mono, type, ignore_silence; int level; };  // a recorder sink's share of a push (result flag 16)
inline RecJob rec_job(const ResRec& q, char* base) { return RecJob{ reinterpret_cast<const float2*>(q.src), base + q.off, base + q.info_off, q.n, q.gain, q.mono, q.type, q.ignore_silence, 0 }; }
int64_t tick_frames_by(const sdrpp_ctx* c, int64_t e) {  // lines complete once the first `e` samples of the block just planned are in (do_fft's own count)
    const int64_t P = (int64_t)c->nz + c->skip;
    const int64_t a = c->plan_fft_pos0 + e - c->nz - c->plan_fft_next0 * P;
    return a >= 0 ? a / P + 1 : 0;
}
int tick_results_describe(sdrpp_ctx* c, uint64_t first_ticket, int k, std::vector<ResCopy>& copies, std::vector<ResRec>& recs, ResMeter& meter, size_t* region_off) {
    copies.clear();
    recs.clear();
    meter = ResMeter{};
    *region_off = 0;
    if (!c->res_flags && !meters_active(c)) {
        for (int j = 0; j < k; j++) {
            sdrpp_ctx::Result& R0 = c->res[(first_ticket + (uint64_t)j) % kResMeta];
            if (!R0.held) { R0 = sdrpp_ctx::Result{}; }
        }
        return SDRPP_OK;
    }
    const bool split = k > 1;
    if (split && (int)c->grp_ends.size() != k) { return fail(c, SDRPP_ERR_INVALID, "internal: %d blocks, %zu push ends", k, c->grp_ends.size()); }
    sdrpp_ctx::Result* R[kGroupMax];
    for (int j = 0; j < k; j++) {
        R[j] = &c->res[(first_ticket + (uint64_t)j) % kResMeta];
        if (R[j]->held) { return fail(c, SDRPP_ERR_INVALID, "results of block %llu are still held %d pushes later: release results sooner", (unsigned long long)R[j]->ticket, kResMeta); }
    }
    for (int j = 0; j < k; j++) {
        *R[j] = sdrpp_ctx::Result{};
        R[j]->ticket = first_ticket + (uint64_t)j;
        R[j]->group = c->groups;
        R[j]->fft_size = c->fft_size;
        R[j]->data_width = c->data_width;
        R[j]->flags = c->res_flags;
    }
    size_t off = 0;
    if (c->res_flags & 1) {
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            int lvl = 1;
            const Stream& s = result_stream(v, &lvl);
            const std::vector<int>& tk = result_ends(v, s);
            if (split && ((int)tk.size() != k || tk[(size_t)k - 1] != s.n)) { return fail(c, SDRPP_ERR_INVALID, "internal: push ends of VFO %d do not add up (%zu ends, %d samples)", v.id, tk.size(), s.n); }
            for (int j = 0; j < k; j++) {
                const int lo = (split && j > 0) ? tk[(size_t)j - 1] : 0, hi = split ? tk[(size_t)j] : s.n;
                R[j]->ids.push_back(v.id);
                R[j]->offsets.push_back((int64_t)(off / 8) + lo);
                R[j]->counts.push_back(hi - lo);
            }
            const size_t bytes = (size_t)s.n * 8;
            if (bytes) { copies.push_back(ResCopy{ s.data, off, bytes, lvl + 1 }); }
            off += (bytes + 15) & ~(size_t)15;
        }
    }
    if ((c->res_flags & 8) && c->pre.on && c->pre.last_n > 0 && !split) {  // the pre-processed stream of the block (what streams bound with bindIQStream receive); groups never form behind a pre-processing chain
        const size_t bytes = (size_t)c->pre.last_n * 8;
        R[0]->off_iq = off;
        R[0]->n_iq = c->pre.last_n;
        copies.push_back(ResCopy{ c->pre.last, off, bytes, c->plan_lvl0 + 1 });
        off += (bytes + 15) & ~(size_t)15;
    }
    const int n_lines = c->fft_on ? c->n_lines : 0;
    int64_t lo_lines[kGroupMax + 1] = { 0 };
    for (int j = 0; j < k; j++) { lo_lines[j + 1] = (split && n_lines > 0) ? std::min<int64_t>(n_lines, tick_frames_by(c, c->grp_ends[(size_t)j])) : n_lines; }
    if (split && lo_lines[k] != n_lines) { return fail(c, SDRPP_ERR_INVALID, "internal: lines of the group do not add up (%lld of %d)", (long long)lo_lines[k], n_lines); }
    for (int j = 0; j < k; j++) { R[j]->n_lines = (int)(lo_lines[j + 1] - lo_lines[j]); }
    if (n_lines > 0) {
        const int lines_level = c->plan_lvl0 + (c->fft_lg <= 12 ? 1 : (c->fft_lg <= 16 ? 2 : 3));
        if ((c->res_flags & 2) && c->data_width > 0) {
            const size_t row = (size_t)c->data_width * 4, bytes = (size_t)n_lines * row;
            for (int j = 0; j < k; j++) { R[j]->off_zoomed = off + (size_t)lo_lines[j] * row; }
            copies.push_back(ResCopy{ c->d_zoomed, off, bytes, lines_level + 2 });
            off += (bytes + 15) & ~(size_t)15;
            for (int j = 0; j < k; j++) { R[j]->off_index = off + (size_t)lo_lines[j] * row; }
            copies.push_back(ResCopy{ c->d_index, off, bytes, lines_level + 2 });
            off += (bytes + 15) & ~(size_t)15;
        }
        if (c->res_flags & 4) {
            const size_t row = (size_t)c->fft_size * 4, bytes = (size_t)n_lines * row;
            for (int j = 0; j < k; j++) { R[j]->off_raw = off + (size_t)lo_lines[j] * row; }
            copies.push_back(ResCopy{ c->d_lines, off, bytes, lines_level + 1 });
            off += (bytes + 15) & ~(size_t)15;
        }
    }
    if (meters_active(c)) {  // one row of n (strength, snr) pairs per line, in line order: push j's share starts at its first line
        const size_t n = c->meters.offs.size(), row = n * 8;
        for (int j = 0; j < k; j++) {
            R[j]->n_meters = (int)n;
            R[j]->off_meters = off + (size_t)lo_lines[j] * row;
        }
        if (n_lines > 0) {
            meter = ResMeter{ n_lines, (int)n, off, c->plan_lvl0 + (c->fft_lg <= 12 ? 1 : (c->fft_lg <= 16 ? 2 : 3)) + 1 };
            off += ((size_t)n_lines * row + 15) & ~(size_t)15;
        }
    }
    if (c->res_flags & 16) {
        // every recorder sink: the group's converted block in one piece (push j's share: frames [tk[j - 1], tk[j]) of it), then one record per push
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            if (!v.rec.on || v.i_out < 0) { continue; }
            int lvl = 1;
            const Stream& s = result_stream(v, &lvl);
            const std::vector<int>& tk = result_ends(v, s);
            if (split && ((int)tk.size() != k || tk[(size_t)k - 1] != s.n)) { return fail(c, SDRPP_ERR_INVALID, "internal: push ends of VFO %d do not add up (%zu ends, %d samples)", v.id, tk.size(), s.n); }
            const size_t bpf = rec_frame_bytes(v.rec), info0 = off + (((size_t)s.n * bpf + 15) & ~(size_t)15);
            for (int j = 0; j < k; j++) {
                const int lo = (split && j > 0) ? tk[(size_t)j - 1] : 0, hi = split ? tk[(size_t)j] : s.n;
                R[j]->rec_ids.push_back(v.id);
                R[j]->rec_off.push_back(off + (size_t)lo * bpf);
                R[j]->rec_info_off.push_back(info0 + (size_t)j * kRecInfoStride);
                recs.push_back(ResRec{ s.data + (size_t)lo * 2, hi - lo, off + (size_t)lo * bpf, info0 + (size_t)j * kRecInfoStride, v.rec.gain, v.rec.mono, v.rec.type, v.rec.ignore_silence, lvl + 1 });
            }
            off = info0 + (size_t)k * kRecInfoStride;
        }
    }
    if (c->res_flags & 32) {
        // every RDS branch that ran in this block: the group's samples in one piece, push j's share between its push ends (Vfo::Rds::tk)
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            const Vfo::Rds& r = v.rds;
            if (!r.attached || !r.ran) { continue; }
            const Stream& s = r.st[(size_t)r.i_last];
            if (split && ((int)r.tk.size() != k || r.tk[(size_t)k - 1] != s.n)) { return fail(c, SDRPP_ERR_INVALID, "internal: push ends of VFO %d's RDS branch do not add up (%zu ends, %d samples)", v.id, r.tk.size(), s.n); }
            for (int j = 0; j < k; j++) {
                const int lo = (split && j > 0) ? r.tk[(size_t)j - 1] : 0, hi = split ? r.tk[(size_t)j] : s.n;
                R[j]->rds_ids.push_back(v.id);
                R[j]->rds_off.push_back(off + (size_t)lo * 8);
                R[j]->rds_counts.push_back(hi - lo);
            }
            const size_t bytes = (size_t)s.n * 8;
            if (bytes) { copies.push_back(ResCopy{ s.data, off, bytes, r.lvl + 1 }); }
            off += (bytes + 15) & ~(size_t)15;
        }
    }
    if (c->res_flags & 64) {
        // every symbol branch that ran in this block: the loop's per-push counts, then what its outputs have room for in this block (how many of them are symbols
        // is the loop's own result: the counts say, sdrpp_result_sym reads them once the block is complete)
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            const Vfo::Sym& y = v.sym;
            if (!y.attached || !y.ran) { continue; }
            if (y.npush != k) { return fail(c, SDRPP_ERR_INVALID, "internal: VFO %d's symbol branch planned %d pushes, the block has %d", v.id, y.npush, k); }
            const size_t cnt_off = off, soft_off = cnt_off + (((size_t)k * 4 + 15) & ~(size_t)15), bits_off = soft_off + (((size_t)y.cap * 4 + 15) & ~(size_t)15);
            for (int j = 0; j < k; j++) {
                R[j]->sym_ids.push_back(v.id);
                R[j]->sym_push.push_back(j);
                R[j]->sym_cnt_off.push_back(cnt_off);
                R[j]->sym_soft_off.push_back(soft_off);
                R[j]->sym_bits_off.push_back(bits_off);
            }
            copies.push_back(ResCopy{ y.st[3].data, cnt_off, (size_t)k * 4, y.lvl + 1 });
            copies.push_back(ResCopy{ y.st[1].data, soft_off, (size_t)y.cap * 4, y.lvl + 1 });
            copies.push_back(ResCopy{ y.st[2].data, bits_off, ((size_t)y.cap + 3) & ~(size_t)3, y.lvl + 1 });
            off = bits_off + (((size_t)y.cap + 15) & ~(size_t)15);
        }
    }
    if (c->res_flags & 128) {
        // every RDS demodulator that ran in this block: the job's per-push counts, then what its outputs have room for in this block (the symbol branch's layout)
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            const Vfo::Rdsd& y = v.rdsd;
            if (!y.attached || !y.ran) { continue; }
            if (y.npush != k) { return fail(c, SDRPP_ERR_INVALID, "internal: VFO %d's RDS demodulator planned %d pushes, the block has %d", v.id, y.npush, k); }
            const size_t cnt_off = off, soft_off = cnt_off + (((size_t)k * 4 + 15) & ~(size_t)15), bits_off = soft_off + (((size_t)y.cap * 4 + 15) & ~(size_t)15);
            for (int j = 0; j < k; j++) {
                R[j]->rdsd_ids.push_back(v.id);
                R[j]->rdsd_push.push_back(j);
                R[j]->rdsd_cnt_off.push_back(cnt_off);
                R[j]->rdsd_soft_off.push_back(soft_off);
                R[j]->rdsd_bits_off.push_back(bits_off);
            }
            copies.push_back(ResCopy{ y.st[2].data, cnt_off, (size_t)k * 4, y.lvl + 1 });
            copies.push_back(ResCopy{ y.st[0].data, soft_off, (size_t)y.cap * 4, y.lvl + 1 });
            copies.push_back(ResCopy{ y.st[1].data, bits_off, ((size_t)y.cap + 3) & ~(size_t)3, y.lvl + 1 });
            off = bits_off + (((size_t)y.cap + 15) & ~(size_t)15);
        }
    }
    if (c->res_flags & 256) {
        // every QPSK demodulator that ran in this block: the job's per-push counts, then [the float pairs] and the int8 pairs its outputs have room for in this block
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            const Vfo::Qpsk& y = v.qpsk;
            if (!y.attached || !y.ran) { continue; }
            if (y.npush != k) { return fail(c, SDRPP_ERR_INVALID, "internal: VFO %d's QPSK demodulator planned %d pushes, the block has %d", v.id, y.npush, k); }
            const size_t cnt_off = off, soft_off = cnt_off + (((size_t)k * 4 + 15) & ~(size_t)15), packed_off = soft_off + (c->res_qpsk_soft ? (((size_t)y.cap * 8 + 15) & ~(size_t)15) : 0);
            for (int j = 0; j < k; j++) {
                R[j]->qpsk_ids.push_back(v.id);
                R[j]->qpsk_push.push_back(j);
                R[j]->qpsk_cnt_off.push_back(cnt_off);
                R[j]->qpsk_soft_off.push_back(c->res_qpsk_soft ? soft_off : SIZE_MAX);
                R[j]->qpsk_packed_off.push_back(packed_off);
            }
            copies.push_back(ResCopy{ y.st[3].data, cnt_off, (size_t)k * 4, y.lvl + 1 });
            if (c->res_qpsk_soft) { copies.push_back(ResCopy{ y.st[1].data, soft_off, (size_t)y.cap * 8, y.lvl + 1 }); }
            copies.push_back(ResCopy{ y.st[2].data, packed_off, ((size_t)y.cap * 2 + 3) & ~(size_t)3, y.lvl + 1 });
            off = packed_off + (((size_t)y.cap * 2 + 15) & ~(size_t)15);
        }
    }
    if (c->res_flags & 512) {
        // every framer that ran in this block: the job's per-push frame counts, then what its records have room for in this block
        for (auto& kv : c->vfos) {
            const Vfo& v = *kv.second;
            const Vfo::Frame& f = v.frame;
            if (!f.attached || !f.ran) { continue; }
            if (f.npush != k) { return fail(c, SDRPP_ERR_INVALID, "internal: VFO %d's framer planned %d pushes, the block has %d", v.id, f.npush, k); }
            const size_t bytes = ((size_t)f.cap * (size_t)f.stride + 3) & ~(size_t)3;
            const size_t cnt_off = off, rec_off = cnt_off + (((size_t)k * 4 + 15) & ~(size_t)15);
            for (int j = 0; j < k; j++) {
                R[j]->frame_ids.push_back(v.id);
                R[j]->frame_push.push_back(j);
                R[j]->frame_stride.push_back(f.stride);
                R[j]->frame_cnt_off.push_back(cnt_off);
                R[j]->frame_rec_off.push_back(rec_off);
            }
            copies.push_back(ResCopy{ f.st[1].data, cnt_off, (size_t)k * 4, f.lvl + 1 });
            copies.push_back(ResCopy{ f.st[0].data, rec_off, bytes, f.lvl + 1 });
            off = rec_off + ((bytes + 15) & ~(size_t)15);
        }
    }
    if (off > c->res_cap) { return fail(c, SDRPP_ERR_INVALID, "internal: results of %zu bytes exceed what a launch may deliver (%zu)", off, c->res_cap); }
    int rc = tick_results_alloc(c, c->groups, off, region_off);
    if (rc) {
        for (int j = 0; j < k; j++) { R[j]->ticket = 0; }
        return rc;
    }
    for (int j = 0; j < k; j++) {
        R[j]->base = c->res_ring + *region_off;
        R[j]->epoch = c->res_epoch;
    }
    return SDRPP_OK;
}
// gather roles of the block just planned -> c->emits (one level behind the producers); fills the result entries of its pushes
int tick_results_plan(sdrpp_ctx* c, uint64_t first_ticket, int k) {
    static thread_local std::vector<ResCopy> copies;
    static thread_local std::vector<ResRec> recs;
    ResMeter meter;
    size_t region = 0;
    int rc = tick_results_describe(c, first_ticket, k, copies, recs, meter, &region);
    if (rc || (copies.empty() && recs.empty() && meter.n == 0)) { return rc; }
    char* base = c->res_ring_dev + region;
    if (meter.n > 0) {  // the signal meters: TR_WF_RING's second form at the level that role reads the raw lines at (and the raw-line gather), straight into the slot; the table travels with the block
        const WfMeterOffs* d_offs = arena_push(c, c->meters.offs);
        if (!d_offs) { return fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }
        emit_meter(c, meter.level, meter.n_lines, d_offs, meters_per_wg(meter.n_lines, meter.n), c->d_lines, c->fft_size, meter.n, reinterpret_cast<float*>(base + meter.off), true);
        c->plan_top = std::max(c->plan_top, meter.level + 1);
    }
    if (!recs.empty()) {  // the recorder sinks: jobs of the copy role (kind 3), one workgroup each, at the level the float gather of the same stream stands at
        Lev<RecJob> rj;
        Lev<CopyJob> cj;
        for (auto& q : recs) { rj.add(q.level, rec_job(q, base)); }
        if (!arena_push_lev(c, rj)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }
        for (int l = 0; l < rj.top; l++) {
            for (size_t i = 0; i < rj.at[l].size(); i++) { cj.add(l, CopyJob{ rj.dev[l] + i, nullptr, 0, 3 | 0x100, 0 }); }
        }
        if (!arena_push_lev(c, cj)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }
        for (int l = 0; l < cj.top; l++) {
            if (cj.at[l].empty()) { continue; }
            emit(c, l, F_MISC, TR_COPY, 1, (int)cj.at[l].size(), 12 * sizeof(float), cj.dev[l]);
            if (!c->emits.empty()) { c->emits.back().to_host = true; }
            c->plan_top = std::max(c->plan_top, l + 1);
        }
    }
    if (copies.empty()) { return SDRPP_OK; }
    Lev<CopyJob> jobs;
    for (auto& q : copies) { jobs.add(q.level, CopyJob{ q.src, base + q.off, (long long)q.bytes, 0x100, 0 }); }
    if (!arena_push_lev(c, jobs)) { return fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }
    for (int l = 0; l < jobs.top; l++) {
        if (jobs.at[l].empty()) { continue; }
        long long mx = 0;
        for (auto& j : jobs.at[l]) { mx = std::max(mx, j.bytes); }
        emit(c, l, F_MISC, TR_COPY, (int)std::max<long long>(1, std::min<long long>((mx + 32767) / 32768, 16)), (int)jobs.at[l].size(), 0, jobs.dev[l]);
        if (!c->emits.empty()) { c->emits.back().to_host = true; }
        c->plan_top = std::max(c->plan_top, l + 1);
    }
    return SDRPP_OK;
}

// results of a block that ran as an ORDINARY pass inside a pipelined run (something the device cannot pipeline: a pre-processing chain, a
// VFO group without the matrix front end, a retune hand-over ...): the same slot layout, filled by plain copies behind the pass and waited
// for here — the slow path, but sdrpp_result_wait / _release then work for EVERY block of a pipelined run, whichever way it was processed
int tick_results_direct(sdrpp_ctx* c, uint64_t first_ticket, int k) {
    int rc = tick_results_ensure(c);
    if (rc) { return rc; }
    static thread_local std::vector<ResCopy> copies;
    static thread_local std::vector<ResRec> recs;
    ResMeter meter;
    size_t region = 0;
    rc = tick_results_describe(c, first_ticket, k, copies, recs, meter, &region);
    if (rc) { return rc; }
    char* base = c->res_ring + region;
    if (meter.n > 0) {  // (the pass has left them in the context's own array: run_meters)
        if (c->meters.out_lines != meter.n_lines || c->meters.out_n != meter.n) { return fail(c, SDRPP_ERR_INVALID, "internal: meters of %d lines x %d, results of %d x %d", c->meters.out_lines, c->meters.out_n, meter.n_lines, meter.n); }
        HIPCHK(c, hipMemcpyAsync(base + meter.off, c->meters.d_out, (size_t)meter.n_lines * meter.n * 8, hipMemcpyDeviceToHost, c->stream));
    }
    for (auto& q : copies) { HIPCHK(c, hipMemcpyAsync(base + q.off, q.src, q.bytes, hipMemcpyDeviceToHost, c->stream)); }
    for (auto& q : recs) {
        hipLaunchKernelGGL(vfo_rec_kernel, dim3(1), dim3(256), 0, c->stream, rec_job(q, c->res_ring_dev + region));
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int j = 0; j < k; j++) {
        sdrpp_ctx::Result& R = c->res[(first_ticket + (uint64_t)j) % kResMeta];
        if (R.ticket == first_ticket + (uint64_t)j) { R.done_tick = c->ticks; }  // nothing queued is left: complete as it stands
    }
    return SDRPP_OK;
}

// sdrpp_push_staged_when: the host is still filling the staging slot with other threads while this thread plans the block; nothing that
// reads the slot may be launched before they are through (the word counts their unfinished parts).
int stage_pending_wait(sdrpp_ctx* c) {
    if (c->stage_pend.empty()) { return SDRPP_OK; }
    std::vector<const volatile uint32_t*> words;
    words.swap(c->stage_pend);
    HostScope hs("staging wait");
    const auto t0 = std::chrono::steady_clock::now();
    for (const volatile uint32_t* w : words) {
        for (unsigned spins = 0; *w != 0u; spins++) {
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
            if ((spins & 0xfffu) == 0xfffu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_staged_when: the staging slot was not completed within 5 s"); }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return SDRPP_OK;
}

// One block in pipelined mode — one push, or a launch group of k pushes (`ends`: their cumulative ends, `count` samples in all; tickets
// first_ticket .. first_ticket + k - 1, already counted in c->pushes: the caller takes them back if this fails).  `d_iq`: where the samples are
// (caller's device buffer) or will be once `land` has run (landing ring).
int tick_push(sdrpp_ctx* c, const float* d_iq, int64_t count, const CopyJob* land, const std::vector<int>* ends, uint64_t first_ticket) {
    if (count == 0) { return SDRPP_OK; }
    const int k = (ends && ends->size() > 1) ? (int)ends->size() : 1;
    struct GroupScope {  // the push ends are visible to the planners (plan_vfo.h: chain) for the duration of this block only
        sdrpp_ctx* c;
        GroupScope(sdrpp_ctx* c_, const std::vector<int>* e, int k_) : c(c_) { if (k_ > 1) { c->grp_ends = *e; } else { c->grp_ends.clear(); } }
        ~GroupScope() { c->grp_ends.clear(); }
    } group_scope(c, ends, k);
    const float* const d_iq_raw = d_iq;  // (planning a pre-processing chain moves d_iq / count on to the pre-processed stream)
    const int64_t count_raw = count;
    c->plan_block_from_host = land != nullptr && land->bytes > 0;
    bool as_tick = tick_eligible(c);
    if (as_tick) {  // rings of the per-block buffers, result slots (allocated on first use / after a change of the configuration)
        for (auto& kv : c->vfos) {
            int rc = SDRPP_OK;
            for_each_stream(*kv.second, [&](Stream& st) {
                if (!rc && st.n_extra < kRing - 1 && st.base) { rc = stream_ring_ensure(c, st); }
            });
            if (rc) { return rc; }
        }
        if (c->pre.on) {  // the pre-processing chain's stage outputs are per-block buffers too
            for (auto& st : c->pre.st) {
                if (st.n_extra < kRing - 1 && st.base) {
                    int rc = stream_ring_ensure(c, st);
                    if (rc) { return rc; }
                }
            }
            if (c->pre.out.base && c->pre.out.n_extra < kRing - 1) {
                int rc = stream_ring_ensure(c, c->pre.out);
                if (rc) { return rc; }
            }
        }
        int rc = fft_ring_ensure(c);
        if (!rc && (c->res_flags || meters_active(c))) { rc = tick_results_ensure(c); }
        if (rc) { return rc; }
    }
    c->groups++;
    const bool have_slot = as_tick;
    static thread_local PlanSnapshot snap;  // (re-used: a fresh one is two allocations per block, tens of KB with 128 VFOs; a nested pass starts only after the outer plan has been restored)
    int rc = SDRPP_OK;
    if (as_tick) {
        HostScope hs("tick plan");
        rc = arena_begin(c);
        if (rc) {
            c->groups--;
            return rc;
        }
        {
            HostScope hs2("tick: snapshot + rotate");
            plan_snapshot(c, snap, true);  // (and every VFO stream on to its next ring buffer, in the same walk)
        }
        fft_ring_rotate(c);
        if (c->pre.on) {
            for (auto& st : c->pre.st) { stream_rotate(st); }
            stream_rotate(c->pre.out);
        }
        c->tick_planning = true;
        c->tick_abort = false;
        c->emits.clear();
        c->plan_top = 2;
        c->plan_lvl0 = 0;
        block_bounds(c, count, k > 1 ? ends : nullptr);
        if (c->pre.on) {  // levels 1 .. plan_lvl0 of the block: from here on `d_iq` / `count` are the pre-processed stream
            rc = run_preproc(c, &d_iq, &count);
            if (!rc && count == 0) { c->tick_abort = true; }  // (the decimator swallowed the whole block: an ordinary pass sorts that out)
        }
        if (!rc && !c->tick_abort) { rc = ensure_iq_hist(c, iq_hist_need(c)); }
        if (!rc && !c->tick_abort) {
            IqSrc src{ (const float2*)d_iq, (const float2*)c->iq_hist[c->iq_cur], c->iq_hist_cap, (long long)count };
            rc = do_fft(c, src, count);
            if (!rc && !c->tick_abort) {
                const CarryJob iqc = iq_carry_job(c, d_iq, count);
                if (c->vfos.empty()) {
                    std::vector<CarryJob> carry{ iqc };
                    CarryJob* d_carry = arena_push(c, carry);
                    if (!d_carry) { rc = fail(c, SDRPP_ERR_UNSUPPORTED, "job arena exhausted"); }
                    else { emit(c, 1 + c->plan_lvl0, F_MISC, TR_CARRY, std::max(1, std::min((iqc.need * 2 + 8191) / 8192, 512)), 1, 0, d_carry); }
                }
                else { rc = do_vfos_plan(c, src, count, iqc); }
            }
            if (!rc && !c->tick_abort) {
                HostScope hs2("tick: results plan");
                rc = tick_results_plan(c, first_ticket, k);
            }
        }
        c->tick_planning = false;
        // the block's depth is where its last ROLE stands, not where the planners reserved room (a bank whose outputs stay on the device has
        // nothing behind its last filter: one tick less until the block is complete, one tick less to drain)
        if (!rc && !c->tick_abort) {
            int top = 2;
            for (auto& r : c->emits) { top = std::max(top, r.level + 1); }
            c->plan_top = std::min(c->plan_top, top);
        }
        if (!rc && !c->tick_abort && c->plan_top > kTickDepth + 1) { c->tick_abort = true; }
        if (rc || c->tick_abort) {
            plan_restore(c, snap);
            c->emits.clear();
            for (int j = 0; j < k; j++) {
                sdrpp_ctx::Result& R = c->res[(first_ticket + (uint64_t)j) % kResMeta];
                if (!R.held) { R.ticket = 0; }
            }
            as_tick = false;
            if (rc) {
                c->groups--;
                return rc;
            }
            c->arena_off = 0;  // (the slot stays this tick's: only the next role table goes in)
        }
    }
    if (!as_tick) {
        c->stat_pass_blocks += k;
        // this block runs as an ordinary pass: everything queued first (the first of those ticks carries the landing copy), then the pass
        // behind them on the same stream
        if (!have_slot) {
            rc = arena_begin(c);
            if (rc) {
                c->groups--;
                return rc;
            }
        }
        rc = stage_pending_wait(c);
        if (!rc) { rc = tick_launch(c, land); }
        if (!rc) { rc = tick_drain(c); }
        if (land) { c->land_tick = c->ticks; }
        if (!rc) { rc = push_common(c, d_iq_raw, count_raw, k > 1 ? ends : nullptr); }
        // its results are where an ordinary pass leaves them (device buffers, readable after a synchronisation) and — with result flags —
        // also in the block's result slot like every other block's
        if (!rc && (c->res_flags || meters_active(c))) { rc = tick_results_direct(c, first_ticket, k); }
        else {
            for (int j = 0; j < k; j++) {
                sdrpp_ctx::Result& R = c->res[(first_ticket + (uint64_t)j) % kResMeta];
                if (!R.held) { R = sdrpp_ctx::Result{}; }
            }
        }
        if (rc) { c->groups--; }
        return rc;
    }
    // queue the roles level by level and launch this block's tick
    HostScope hs3("tick: queue + launch");
    c->stat_tick_blocks += k;
    c->stat_last_depth = c->plan_top;
    c->stat_last_table_bytes = (int64_t)c->arena_off;  // job tables of this block (the next tick's role table is added at the launch)
    if ((int)c->tickq.size() < c->plan_top) { c->tickq.resize((size_t)c->plan_top); }
    for (auto& r : c->emits) { c->tickq[(size_t)r.level].push_back(r); }
    c->emits.clear();
    c->iq_cur ^= 1;
    // tickq[0] is this very tick: it holds only what earlier blocks queued (a block's own roles start at level 1)
    rc = stage_pending_wait(c);
    if (!rc) {
        HostScope hs("tick launch");
        rc = tick_launch(c, land);
    }
    if (land) { c->land_tick = c->ticks; }
    for (int j = 0; j < k; j++) {
        sdrpp_ctx::Result& R = c->res[(first_ticket + (uint64_t)j) % kResMeta];
        if (R.ticket == first_ticket + (uint64_t)j) { R.done_tick = c->ticks + (uint64_t)(c->plan_top - 1); }
    }
    return rc;
}

// bytes per complex sample of a wire format (sdrpp_iq_format::type)
inline size_t iq_format_bytes(int type) { return type == SDRPP_IQ_I16 ? 4 : 2; }

// ---- several blocks per launch (sdrpp_set_pipeline_group) ---------------------------------------------------------------------------------
// May pushes share a launch at all right now?  Not behind a pre-processing chain (its decimator changes the rate the push ends live at), not while a
// block cannot run as a tick, and not with a VFO that only rotates (no decimation plan: its NCO is anchored at the start of a launch, the results
// would differ from block-by-block processing in the last bit).
bool group_eligible(sdrpp_ctx* c) {
    if (c->group_max <= 1 || c->pre.on || !tick_eligible(c)) { return false; }
    for (Vfo* v : c->vfo_list) {
        if (!v->nco_exact && v->rate.n_stages == 0) { return false; }
    }
    return true;
}
// Whatever is held goes out as ONE block of the tick queue (nothing held: nothing happens).  On failure the held pushes did not happen: their
// tickets are taken back.
int tick_group_launch(sdrpp_ctx* c) {
    if (c->held.kind < 0 || c->held.ends.empty()) { return SDRPP_OK; }  // (a staging slot handed out by sdrpp_push_stage and not yet pushed stays open)
    sdrpp_ctx::Held H;
    std::swap(H, c->held);
    const int k = (int)H.ends.size();
    const uint64_t first_ticket = c->pushes - (uint64_t)k + 1;
    int rc = SDRPP_OK;
    if (H.kind == 0) { rc = tick_push(c, reinterpret_cast<const float*>(H.base), H.total, nullptr, &H.ends, first_ticket); }  // read in place, one tick from now at the earliest
    else {
        const int li = (int)((c->groups + 1) % 3);
        if (!c->tick_land[li]) { rc = dev_alloc(c, &c->tick_land[li], (size_t)SDRPP_LAND_TABLE + (size_t)c->max_push * 2 + 32); }
        void* d = nullptr;
        if (!rc && (hipHostGetDevicePointer(&d, H.kind == 3 ? (void*)H.base : (void*)c->stage_host[H.stage_slot], 0) != hipSuccess || !d)) { rc = fail(c, SDRPP_ERR_HIP, "hipHostGetDevicePointer(staging) failed"); }
        float* const land_iq = c->tick_land[li] ? c->tick_land[li] + SDRPP_LAND_TABLE : nullptr;
        if (!rc && H.kind == 2 && H.fmt_type == SDRPP_IQ_U8 && c->tick_land_tab[li] != H.fmt_table) {
            // The landing copy runs in the very tick that uploads the block's job tables, so the table cannot travel in the arena: it goes in front of
            // the landing buffer, on the stream, ahead of the launch that reads it (1 KB, and only when this buffer last saw another table).
            if (hipMemcpyAsync(c->tick_land[li], H.fmt_table.data(), (size_t)SDRPP_LAND_TABLE * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(c, SDRPP_ERR_HIP, "upload of the U8 table failed"); }
            else { c->tick_land_tab[li] = H.fmt_table; }
        }
        if (!rc) {
            CopyJob land{ d, land_iq, (long long)((size_t)H.total * 8), 0, 0 };
            if (H.kind == 2) {
                const float inv = H.fmt_type == SDRPP_IQ_U8 ? 0.0f : 1.0f / H.fmt_scalar;
                int inv_bits;
                memcpy(&inv_bits, &inv, sizeof(inv_bits));
                land = CopyJob{ d, land_iq, (long long)((size_t)H.total * iq_format_bytes(H.fmt_type)), 4 | (H.fmt_type << 16), inv_bits };
            }
            rc = tick_push(c, land_iq, H.total, &land, &H.ends, first_ticket);
            if (H.kind != 3) { c->stage_tick[H.stage_slot] = c->ticks; }
        }
    }
    c->stage_pend.clear();
    if (rc) { c->pushes -= (uint64_t)k; }
    else if (k > 1) {
        c->stat_groups++;
        c->stat_group_blocks += k;
        c->stat_group_max = std::max<int64_t>(c->stat_group_max, k);
    }
    return rc;
}
// One push of a pipelined run: joins the held group, or — the group full, the push of another kind or not contiguous with it, grouping off — sends
// what is held on its way first.  kind 0: `p` = device address (read in place); 1 / 2: float / raw (`fmt`) samples in host memory, copied into the
// group's page-locked staging slot (p == nullptr: the host has filled the slot itself, sdrpp_push_stage); 3: the caller's page-locked memory.
// A raw push is "of another kind" than the held ones unless its format is theirs: type, the scalar's bits, for U8 the table's contents — the landing
// copy of a launch converts with ONE format.
int tick_hold(sdrpp_ctx* c, int kind, const void* p, int64_t count, const volatile uint32_t* pending, const sdrpp_iq_format* fmt = nullptr) {
    if (count == 0) { return SDRPP_OK; }
    sdrpp_ctx::Held& H = c->held;
    const bool groupable = group_eligible(c);
    const size_t bps = kind == 2 ? iq_format_bytes(fmt->type) : 8;
    if (H.kind >= 0) {
        bool fits = groupable && H.kind == kind && (int)H.ends.size() < c->group_max && H.total + count <= c->max_push;
        if (fits && kind == 2) {
            fits = H.fmt_type == fmt->type && (fmt->type == SDRPP_IQ_U8 ? memcmp(H.fmt_table.data(), fmt->table, 256 * sizeof(float)) == 0 : memcmp(&H.fmt_scalar, &fmt->scalar, sizeof(float)) == 0);
        }
        if (fits && (kind == 0 || kind == 3)) { fits = reinterpret_cast<const char*>(p) == H.base + (size_t)8 * (size_t)H.total; }
        if (H.ends.empty() && H.kind == kind && kind == 1 && H.total == 0) { fits = true; }  // (a slot opened by sdrpp_push_stage, nothing in it yet)
        if (!fits) {
            if ((kind == 1 || kind == 2) && !p) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_staged: %lld samples do not fit the open staging slot", (long long)count); }
            int rc = tick_group_launch(c);
            if (rc) { return rc; }
            c->held = sdrpp_ctx::Held{};
        }
    }
    if (H.kind < 0) {
        if ((kind == 1 || kind == 2) && !p) { return fail(c, SDRPP_ERR_INVALID, "sdrpp_push_staged without an open staging slot (sdrpp_push_stage)"); }
        H.kind = kind;
        H.base = reinterpret_cast<const char*>(p);
        H.total = 0;
        H.ends.clear();
        if (kind == 2) {
            H.fmt_type = fmt->type;
            H.fmt_scalar = fmt->scalar;
            if (fmt->type == SDRPP_IQ_U8) { H.fmt_table.assign(fmt->table, fmt->table + 256); }
        }
        if (kind == 1 || kind == 2) {
            const int si = c->stage_cur;
            c->stage_cur = (c->stage_cur + 1) % kStageSlots;
            if (!c->stage_host[si]) {
                if (hipHostMalloc((void**)&c->stage_host[si], (size_t)c->max_push * 8 + 64, hipHostMallocMapped) != hipSuccess) {
                    H.kind = -1;
                    return fail(c, SDRPP_ERR_NOMEM, "page-locked staging buffer");
                }
            }
            if (c->stage_tick[si]) { tick_wait_done(c, c->stage_tick[si]); }  // its last landing copy has run
            H.stage_slot = si;
        }
    }
    if ((kind == 1 || kind == 2) && p) { memcpy(reinterpret_cast<char*>(c->stage_host[H.stage_slot]) + (size_t)H.total * bps, p, (size_t)count * bps); }
    H.total += count;
    H.ends.push_back((int)H.total);
    c->pushes++;
    bool go = !groupable || (int)H.ends.size() >= c->group_max;
    if (!go && c->group_adaptive && c->h_tick_flag) { go = (int)((unsigned)c->ticks - *(const volatile unsigned*)c->h_tick_flag) < 2; }  // the device would run dry: do not wait for more
    if (pending) {
        // sdrpp_push_staged_when: the word belongs to the caller and is only promised to live for the call.  The push that sends the group on its
        // way is planned while its copy threads are still at work (the wait comes just before the launch, stage_pending_wait); one that is merely
        // held has nothing to overlap with: it waits here — unless the caller has promised (sdrpp_set_pipeline_group flag 2) that its words live until
        // the launch: then the hold returns at once and the copy runs on under whatever the caller does next; the launch of the group waits for all of them.
        c->stage_pend.push_back(pending);
        if (!go && !c->stage_pend_stable) {
            int rc = stage_pending_wait(c);
            if (rc) {  // the block did not arrive: it is not part of the group
                H.ends.pop_back();
                H.total -= count;
                c->pushes--;
                return rc;
            }
        }
    }
    return go ? tick_group_launch(c) : SDRPP_OK;
}

}  // namespace
