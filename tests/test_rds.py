"""The WFM demodulator's RDS branch on the device (sdrpp_vfo_set_rds): discriminator -> translation by -57 kHz -> RationalResampler<complex_t>(250 kS/s ->
5 kS/s), the `_rdsOut` path of dsp::demod::BroadcastFM (core/src/dsp/demod/broadcast_fm.h:144-215).

YARDSTICK: pieces the oracle already has, each pinned to the reference by tests/test_oracle_vs_reference.py — orc_demod (WFM, low-pass off: column 0 is the
discriminator), orc_xlator(-57000, 250000) (orc_xlator_set_ideal for the closed-form comparison; fed reference block by reference block for the rotator
comparison) and orc_resampler(plans, 250000, 5000, 2) — always applied to the IF stream the device itself delivered (vfo_read_if, or vfo_ifc_read behind an IF chain).

BOUNDS: 1e-5 of the yardstick's RMS over a run (BASELINE.json), 1e-6 between push cuts in closed form (per-push anchoring), bit for bit wherever two paths of the
device compute the same thing.

PER SAMPLE: tests/test_rds_rows.py — every output against a float64 restatement, at every tile, pitch, window, line and rotator-block edge; every value test
here runs ONE description (first stage 44 taps decimating by 8: tile 29, pitch 34, a window of 268 samples) and sees a run's RMS only."""
import ctypes as C
import os

import numpy as np
import pytest

import support as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rds_ref.npz")
SR, IF_RATE, BW, F0 = 1e6, 250e3, 150e3, 200e3  # one WFM VFO at +200 kHz: plan {2 x 12, 2 x 69}, IF 250 k
B = 5000                                         # one push = one reference block = 1 250 IF samples = 25 or 26 outputs
NOT_FOUND, INVALID, UNSUPPORTED = -6, -2, -5


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Yardstick:
    """orc_demod (discriminator) -> orc_xlator -> orc_resampler; the three objects live as long as the reference's BroadcastFM keeps them."""

    def __init__(self, ideal, if_rate=IF_RATE, bw=BW):
        self.O = S.oracle()
        self.if_rate, self.bw = if_rate, bw
        self.dem = None
        self.fresh_demod()
        self.xl = self.O.orc_xlator_create(-57000.0, if_rate)
        self.O.orc_xlator_set_ideal(self.xl, int(bool(ideal)))
        self.rs = self.O.orc_resampler_create(S.plans_handle(), if_rate, 5000.0, 2)

    def fresh_demod(self):
        """BroadcastFM::reset / RxVFO::reset: the discriminator starts over, xlator and rdsResamp stay"""
        if self.dem:
            self.O.orc_demod_destroy(self.dem)
        self.dem = self.O.orc_demod_create(S.MODES["WFM"], self.bw, self.if_rate, 0, 50.0, 5.0, 0)

    def discriminate(self, ifs):
        ifs = S.c64(ifs)
        a = np.empty((len(ifs) + 1, 2), np.float32)
        n = self.O.orc_demod_process(self.dem, len(ifs), S._fp(ifs.view(np.float32)), S._fp(a)) if len(ifs) else 0
        d = np.zeros(n, np.complex64)
        d.real = a[:n, 0]
        return d

    def branch(self, d, cut=None):
        """xlator (called once per entry of `cut`, the reference's blocks at the IF rate) and resampler over discriminator values"""
        out, pos = [], 0
        for n in (cut if cut is not None else [len(d)]):
            if n == 0:
                continue
            x = np.ascontiguousarray(d[pos:pos + n])
            c = np.empty(n, np.complex64)
            self.O.orc_xlator_process(self.xl, n, S._fp(x.view(np.float32)), S._fp(c.view(np.float32)))
            y = np.empty(n + 16, np.complex64)
            m = self.O.orc_resampler_process(self.rs, n, S._fp(c.view(np.float32)), S._fp(y.view(np.float32)))
            out.append(y[:m].copy())
            pos += n
        assert pos == len(d)
        return np.concatenate(out) if out else np.zeros(0, np.complex64)

    def process(self, ifs, cut=None, feed=True):
        """feed = False: rdsOut is off — the discriminator runs (it is the audio path's), the branch sees nothing"""
        d = self.discriminate(ifs)
        return self.branch(d, cut) if feed else np.zeros(0, np.complex64)

    def close(self):
        self.O.orc_demod_destroy(self.dem)
        self.O.orc_xlator_destroy(self.xl)
        self.O.orc_resampler_destroy(self.rs)
        self.dem = None


def broadcast(n, seed, sr=SR, f0=F0, bits=None, rds_dev=3000.0, noise=0.002):
    """An FM carrier at f0, 75 kHz deviation: 1 kHz audio, the 19 kHz pilot, a biphase-modulated 57 kHz subcarrier (phase 0 at sample 0) of ~3 kHz deviation, noise."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / sr
    if bits is None:
        bits = r.integers(0, 2, int(n / sr * 1187.5) + 2)
    bb = biphase(bits, n, sr)
    msg = 0.45 * np.sin(2 * np.pi * 1000.0 * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t) + (rds_dev / 75e3) * bb * np.cos(2 * np.pi * 57000.0 * t)
    ph = 2 * np.pi * np.cumsum(75e3 * msg) / sr
    x = 0.5 * np.exp(1j * (2 * np.pi * f0 * t + ph)) + noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return x.astype(np.complex64)


def biphase(bits, n, sr):
    """differentially encoded biphase symbols at 1187.5 bit/s: +1 / -1 over the first half of a symbol, the opposite over the second"""
    enc = np.cumsum(np.asarray(bits)) & 1  # differential encoding
    t = np.arange(n) / sr * 1187.5
    k = np.minimum(t.astype(np.int64), len(enc) - 1)
    half = (t - np.floor(t)) < 0.5
    return np.where(enc[k] == 1, 1.0, -1.0) * np.where(half, 1.0, -1.0)


def make_ctx(max_push=200000, ref_block=B):
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max_push)
    ctx.set_reference_block(ref_block)
    return ctx


def add_wfm(ctx, f0=F0, nco_mode=0, rds=True, enabled=True):
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(SR, IF_RATE, BW, f0, "WFM", nco_mode=nco_mode)
    vid = ctx.vfo_add(d, keep)
    if rds:
        rd, rkeep = radio.rds_desc(IF_RATE)
        ctx.vfo_set_rds(vid, rd, enabled, rkeep)
    return vid


def run_cut(ctx, vid, x, size):
    """push x in pushes of `size`; -> (outputs per push, IF per push)"""
    outs, ifs = [], []
    for lo in range(0, len(x), size):
        ctx.push(x[lo:lo + size])
        outs.append(ctx.vfo_rds_read(vid))
        ifs.append(ctx.vfo_read_if(vid))
    return outs, ifs


@pytest.fixture(scope="module")
def stream():
    return broadcast(200000, seed=7)


# ---- 1. the yardstick against the reference's recorded outputs ---------------------------------------------------------------------------
def test_yardstick_reproduces_the_reference_fixture():
    """The composed yardstick (oracle's own rotator), fed the fixture's IF inputs with its block schedule, gives the fixture's `rdsout` and per-block counts bit
    for bit — the state frozen across setRDSOut(false) and kept through reset() included (case toggle_reset)."""
    z = np.load(GOLDEN)
    for name in z["names"]:
        x = (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
        cut, on, reset_at = z[name + "_cut"], z[name + "_on"], z[name + "_reset"]
        y = Yardstick(ideal=False)
        pos, outs, counts = 0, [], []
        for b, n in enumerate(cut):
            if b in reset_at:
                y.fresh_demod()
            o = y.process(x[pos:pos + n], feed=bool(on[b]))
            outs.append(o)
            counts.append(len(o))
            pos += int(n)
        y.close()
        assert np.array_equal(np.asarray(counts), z[name + "_counts"]), (name, counts, z[name + "_counts"])
        assert bits_equal(np.concatenate(outs), z[name + "_rds"].view(np.complex64).reshape(-1)), name
        assert sum(counts) > 100


def test_the_references_click_on_setrdsout_is_the_documented_deviation():
    """The fixture's audio around the two setRDSOut calls of case toggle_reset (blocks 2 .. 5): the oracle's WFM demodulator (low-pass on) reproduces it bit
    for bit only if it is replaced by a fresh one in front of blocks 3 and 5 — BroadcastFM::setRDSOut clears the discriminator and the audio filter.  Run
    through, as this project's layer runs the audio path whatever the branch does (the documented deviation; test_the_branch_changes_no_other_output), the
    audio differs right behind the switch: the reference's click."""
    z, O = np.load(GOLDEN), S.oracle()
    x = (z["toggle_reset_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
    want = z["toggle_reset_audio"]
    assert len(want) == 4 * 1250

    def audio(fresh_at):
        dem, out = O.orc_demod_create(S.MODES["WFM"], BW, IF_RATE, 1, 50.0, 5.0, 0), []
        for b in range(6):
            if b in fresh_at:
                O.orc_demod_destroy(dem)
                dem = O.orc_demod_create(S.MODES["WFM"], BW, IF_RATE, 1, 50.0, 5.0, 0)
            blk = np.ascontiguousarray(x[b * 1250:(b + 1) * 1250])
            a = np.empty((1251, 2), np.float32)
            O.orc_demod_process(dem, 1250, S._fp(blk.view(np.float32)), S._fp(a))
            out.append(a[:1250, 0].copy())
        O.orc_demod_destroy(dem)
        return np.concatenate(out[2:])

    assert bits_equal(audio({3, 5}), want)
    through = audio(set())
    assert bits_equal(through[:1250], want[:1250])  # block 2: in front of the first switch
    assert np.max(np.abs(through[1250:1300] - want[1250:1300])) > 0.1 * rms(want)  # the click


# ---- 2. closed form against the ideal-NCO yardstick --------------------------------------------------------------------------------------
def test_closed_form_against_the_ideal_nco_yardstick(backend, stream):
    """40 pushes of 5 000 samples (reference block 5 000): per-push counts equal the yardstick's, the RMS error over the run is below 1e-5 of its RMS."""
    ctx = make_ctx()
    vid = add_wfm(ctx)
    outs, ifs = run_cut(ctx, vid, stream, B)
    y = Yardstick(ideal=True)
    want = [y.process(i) for i in ifs]
    assert [len(o) for o in outs] == [len(w) for w in want]
    assert len(outs) == 40 and sum(len(o) for o in outs) == 1001  # (26, 25, 25, ...: the first block holds the output at sample 0)
    g, w = np.concatenate(outs), np.concatenate(want)
    rel = rms(g - w) / rms(w)
    print("[rds] closed form vs ideal-NCO yardstick: %.3g of the RMS (%.3g)" % (rel, rms(w)))
    assert rel < 1e-5, rel
    y.close()
    ctx.close()


# ---- 3. reference-rotator mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("push", [5000, 15000])
def test_reference_rotator_against_the_oracles_rotator(backend, stream, push):
    """nco_mode = 2, reference block 5 000, the run length of the closed-form test (200 000 samples; with pushes of 15 000 the last push is 5 000): against
    the yardstick with the oracle's own rotator called once per reference block (1 250 IF samples)."""
    x = stream
    ctx = make_ctx()
    vid = add_wfm(ctx, nco_mode=2)
    outs, ifs = run_cut(ctx, vid, x, push)
    y = Yardstick(ideal=False)
    want = [y.process(i, cut=[1250] * (len(i) // 1250)) for i in ifs]
    assert [len(o) for o in outs] == [len(w) for w in want]
    g, w = np.concatenate(outs), np.concatenate(want)
    assert len(w) == 1001
    rel = rms(g - w) / rms(w)
    print("[rds] reference rotator, pushes of %d: %.3g of the RMS" % (push, rel))
    assert rel < 1e-5, rel
    y.close()
    ctx.close()


# ---- 4. push-cut invariance --------------------------------------------------------------------------------------------------------------
def test_push_cut_invariance_closed_form(backend, stream):
    """The same stream in pushes of 5 000, of 1 234 and in one push of 200 000: equal totals, outputs within 1e-6 of the RMS (the NCO is anchored per push)."""
    res = {}
    for size in (5000, 1234, 200000):
        ctx = make_ctx()
        vid = add_wfm(ctx)
        res[size] = np.concatenate(run_cut(ctx, vid, stream, size)[0])
        ctx.close()
    a = res[5000]
    for size in (1234, 200000):
        assert len(res[size]) == len(a) == 1001
        rel = rms(res[size] - a) / rms(a)
        print("[rds] cut %d vs 5000: %.3g of the RMS" % (size, rel))
        assert rel < 1e-6, (size, rel)


@pytest.mark.parametrize("ref_block,size", [(5000, 5000), (1234, 1234)])
def test_push_cut_invariance_reference_rotator(backend, stream, ref_block, size):
    """Reference-rotator mode with a fixed reference block: bit for bit whatever the cut.  A push end is always a block end (include/sdrpp_gpu.h,
    sdrpp_set_reference_block), so a cut is compared with the one push of the whole stream under the block size it is commensurate with: pushes of 5 000 under
    blocks of 5 000, pushes of 1 234 under blocks of 1 234 (this narrows the issue's case — three cuts under ONE block size — to what the block structure
    admits; DESIGN.md 8d says so too)."""
    x = stream
    res = []
    for push in (size, len(x)):
        ctx = make_ctx(ref_block=ref_block)
        vid = add_wfm(ctx, nco_mode=2)
        res.append(np.concatenate(run_cut(ctx, vid, x, push)[0]))
        ctx.close()
    assert len(res[0]) == len(x) // 200 + 1
    assert bits_equal(res[0], res[1])


# ---- 5. pipelined and grouped ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4, 32])
def test_pipelined_and_grouped_equal_the_ordinary_path(backend, stream, group):
    """Two WFM VFOs with the branch and one NFM VFO without: result_rds of every ticket equals the ordinary path's samples of that push bit for bit, counts
    included; a ticket pushed before the attach or without the flag, and the NFM VFO, give SDRPP_ERR_NOT_FOUND; the NFM audio is untouched."""
    from sdrplusplus_amd import capi, radio

    npush, first_with = 36, 2  # (the branch of VFO b is attached behind push 2)
    sizes = [5000 if i % 3 else 4000 for i in range(npush)]
    x = stream[:sum(sizes)]

    def bank(ctx, late):
        a = add_wfm(ctx, F0)
        b = add_wfm(ctx, -150e3, rds=not late)
        d, keep = radio.vfo_desc(SR, 50e3, 12.5e3, -300e3, "NFM")
        return a, b, ctx.vfo_add(d, keep)

    rd, rkeep = radio.rds_desc(IF_RATE)
    ctx = make_ctx(ref_block=0)
    a, b, n = bank(ctx, True)
    want, pos = [], 0
    for i, sz in enumerate(sizes):
        if i == first_with:
            ctx.vfo_set_rds(b, rd, True, rkeep)
        ctx.push(x[pos:pos + sz])
        want.append((ctx.vfo_rds_read(a), ctx.vfo_rds_read(b) if i >= first_with else None, ctx.vfo_read(n)))
        pos += sz
    ctx.close()
    plain = make_ctx(ref_block=0)  # the NFM VFO alone: what its audio is without any branch in the bank
    d, keep = radio.vfo_desc(SR, 50e3, 12.5e3, -300e3, "NFM")
    pn = plain.vfo_add(d, keep)
    pos = 0
    for i, sz in enumerate(sizes):
        plain.push(x[pos:pos + sz])
        assert bits_equal(plain.vfo_read(pn), want[i][2]), i
        pos += sz
    plain.close()

    ctx = make_ctx(ref_block=0)
    a, b, n = bank(ctx, True)
    ctx.set_pipelined(True, 1)  # no flag 32 yet
    ctx.set_pipeline_group(group)
    pos = 0
    flagged_from = 1
    for i, sz in enumerate(sizes):
        if i == flagged_from:
            ctx.pipeline_flush()
            assert ctx.L.sdrpp_pipeline_set_rds_results(ctx.h, 1) == 0
        if i == first_with:
            ctx.vfo_set_rds(b, rd, True, rkeep)
        ctx.push(x[pos:pos + sz])
        pos += sz
    data, cnt = capi.c_float_p(), C.c_int()
    for i in range(npush):
        tk = i + 1
        res = ctx.result_wait(tk)
        assert bits_equal(res["vfo"][n], want[i][2]), ("nfm audio", i)
        assert ctx.L.sdrpp_result_rds(ctx.h, tk, n, C.byref(data), C.byref(cnt)) == NOT_FOUND
        if i < flagged_from:
            assert ctx.L.sdrpp_result_rds(ctx.h, tk, a, C.byref(data), C.byref(cnt)) == NOT_FOUND  # pushed without the flag
        else:
            assert bits_equal(ctx.result_rds(tk, a), want[i][0]), ("a", i)
        if i < first_with:
            assert ctx.L.sdrpp_result_rds(ctx.h, tk, b, C.byref(data), C.byref(cnt)) == NOT_FOUND  # pushed before the attach
        else:
            assert bits_equal(ctx.result_rds(tk, b), want[i][1]), ("b", i)
        ctx.result_release(tk)
        assert ctx.L.sdrpp_result_rds(ctx.h, tk, a, C.byref(data), C.byref(cnt)) == INVALID  # not held any more
    st = ctx.pipeline_stats()
    assert st["pass_blocks"] == 0, st
    ctx.set_pipelined(False)
    ctx.close()


# ---- 6. the branch is a side branch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_the_branch_changes_no_other_output(backend, stream, pipelined):
    """Three identical WFM VFOs — never attached, attached and disabled, attached and enabled — with an AF chain each: audio, IF and AF outputs are bit-identical
    among the three over 20 pushes."""
    from sdrplusplus_amd import radio

    ctx = make_ctx()
    ids = [add_wfm(ctx, rds=False), add_wfm(ctx, enabled=False), add_wfm(ctx)]
    for v in ids:
        af, akeep = radio.af_desc(IF_RATE)
        ctx.vfo_set_af(v, af, akeep)
    if pipelined:
        ctx.set_pipelined(True, 1 | 32)
    total = 0
    for i in range(20):
        ctx.push(stream[i * B:(i + 1) * B])
        if pipelined:
            res = ctx.result_wait(i + 1)
            got = [(res["vfo"][v],) for v in ids]
            total += len(ctx.result_rds(i + 1, ids[2]))
            assert ctx.L.sdrpp_result_rds(ctx.h, i + 1, ids[1], None, None) == NOT_FOUND
            ctx.result_release(i + 1)
        else:
            got = [(ctx.vfo_read(v), ctx.vfo_read_if(v), ctx.vfo_af_read(v)) for v in ids]
            total += len(ctx.vfo_rds_read(ids[2]))
            assert ctx.vfo_rds_count(ids[1]) == 0
        for k in (1, 2):
            for p, q in zip(got[0], got[k]):
                assert len(p) > 0 and bits_equal(p, q), (i, k)
    assert total == 501
    if pipelined:
        ctx.set_pipelined(False)
    ctx.close()


# ---- 7. disable, enable, reset, replace --------------------------------------------------------------------------------------------------
def test_disable_enable_reset_replace(backend, stream):
    from sdrplusplus_amd import radio

    ctx = make_ctx()
    vid = add_wfm(ctx)
    rd, rkeep = radio.rds_desc(IF_RATE)
    y = Yardstick(ideal=True)
    G, W = [], []

    def step(i, feed=True):
        ctx.push(stream[i * B:(i + 1) * B])
        got, want = ctx.vfo_rds_read(vid), y.process(ctx.vfo_read_if(vid), feed=feed)
        assert len(got) == len(want), (i, len(got), len(want))
        G.append(got)
        W.append(want)

    for i in range(0, 4):
        step(i)
    ctx.vfo_set_rds(vid, rd, False, rkeep)  # off for three pushes: the state freezes, the yardstick simply is not fed those blocks
    for i in range(4, 7):
        step(i, feed=False)
    ctx.vfo_set_rds(vid, rd, True, rkeep)
    for i in range(7, 11):
        step(i)
    ctx.vfo_reset(vid)  # the branch's state stays; the discriminator's previous phase is 0 again
    y.fresh_demod()
    for i in range(11, 15):
        step(i)
    d, keep = radio.vfo_desc(SR, IF_RATE, BW, F0, "WFM")
    old = vid
    vid = ctx.vfo_replace(old, d, 3, keep)  # keep & 2: the branch moves with the demodulator (keep & 1: the channeliser's phase and delay line)
    for i in range(15, 19):
        step(i)
    g, w = np.concatenate(G), np.concatenate(W)
    rel = rms(g - w) / rms(w)
    print("[rds] disable / enable / reset / replace: %.3g of the RMS over %d samples" % (rel, len(w)))
    assert rel < 1e-5 and len(w) > 350
    # every stretch on its own too (a lost delay line shows in the first outputs behind the switch)
    for k in (7, 11, 15):
        assert rms(G[k] - W[k]) < 1e-5 * rms(w), k
    new2 = ctx.vfo_replace(vid, d, 1, keep)  # without the bit the new handle has no branch
    assert ctx.L.sdrpp_vfo_rds_count(ctx.h, new2) == INVALID
    assert ctx.L.sdrpp_vfo_rds_count(ctx.h, vid) == NOT_FOUND  # (the old handle is gone)
    y.fresh_demod()  # (keep & 2 off: the new handle's demodulator is a new object)
    ctx.vfo_set_rds(new2, rd, True, rkeep)  # a fresh attach starts cleared: a fresh yardstick branch behind that discriminator
    y2 = Yardstick(ideal=True)
    ctx.push(stream[19 * B:20 * B])
    got = ctx.vfo_rds_read(new2)
    want = y2.branch(y.discriminate(ctx.vfo_read_if(new2)))  # (d[0] belongs to the running demodulator)
    assert len(got) == len(want) == 26  # offsets 0 again: 26 outputs for the first 1 250 samples
    assert rms(got - want) < 1e-5 * rms(w)
    y.close()
    y2.close()
    ctx.close()


# ---- 7b. tiny pushes directly behind attach, enable, reset and replace; further switches inside that window; the same pipelined --------------
@pytest.mark.parametrize("cuts", [[2, 4998], [40, 60, 4900], [100, 4900], [400, 4600], [3, 1, 4, 4992]], ids=lambda c: "-".join(map(str, c)))
def test_short_pushes_behind_every_switch(backend, stream, cuts):
    """The first decimator's delay line is set aside at attach (zeros), disable, sdrpp_vfo_reset and sdrpp_vfo_replace, and must stay in force until the branch
    has been fed its 44 samples again — however small the pushes behind the switch are (2 input samples are no IF sample at all, 100 are 25).  Every
    switch is followed by the pushes of `cuts` (one reference block of 5 000 in pieces); the outputs are compared with the yardstick fed the device's IF."""
    from sdrplusplus_amd import radio

    ctx = make_ctx(ref_block=0)
    d, keep = radio.vfo_desc(SR, IF_RATE, BW, F0, "WFM")
    rd, rkeep = radio.rds_desc(IF_RATE)
    state = {"vid": add_wfm(ctx, rds=False), "pos": 0}
    y = Yardstick(ideal=True)
    G, W = [], []

    def push(n, feed=True):
        vid = state["vid"]
        ctx.push(stream[state["pos"]:state["pos"] + n])
        state["pos"] += n
        ifs = ctx.vfo_read_if(vid)
        if feed is None:  # no branch yet: only the discriminator runs
            y.discriminate(ifs)
            return
        got, want = ctx.vfo_rds_read(vid), y.process(ifs, feed=feed)
        assert len(got) == len(want), (state["pos"], len(got), len(want))
        G.append(got)
        W.append(want)

    def pieces():
        for n in cuts:
            push(n)
        push(B)

    for _ in range(3):
        push(B, feed=None)  # the stream has a history before the attach
    ctx.vfo_set_rds(state["vid"], rd, True, rkeep)
    pieces()
    ctx.vfo_set_rds(state["vid"], rd, False, rkeep)
    push(B, feed=False)
    for n in cuts:
        push(n, feed=False)
    ctx.vfo_set_rds(state["vid"], rd, True, rkeep)
    pieces()
    ctx.vfo_reset(state["vid"])
    y.fresh_demod()
    pieces()
    state["vid"] = ctx.vfo_replace(state["vid"], d, 3, keep)
    pieces()
    g, w = np.concatenate(G), np.concatenate(W)
    assert len(w) > 190
    rel = rms(g - w) / rms(w)
    worst = max(rms(a - b) for a, b in zip(G, W) if len(a)) / rms(w)
    print("[rds] short pushes %s behind attach / enable / reset / replace: %.3g of the RMS, worst push %.3g" % (cuts, rel, worst))
    assert rel < 1e-5 and worst < 1e-5, (rel, worst)
    y.close()
    ctx.close()


SPLICE_OPS = [("push", B), ("off",), ("push", B), ("on",), ("push", 100), ("reset",), ("push", B), ("push", B),               # enable -> short push -> reset
              ("off",), ("push", B), ("on",), ("push", 100), ("off",), ("push", B), ("on",), ("push", 60), ("push", B),         # enable -> short push -> disable / enable -> short push
              ("reset",), ("push", 40), ("reset",), ("push", 8), ("push", 2), ("push", B),                                       # reset -> short push -> reset -> short pushes
              ("off",), ("push", B), ("on",), ("push", 100), ("replace",), ("push", 48), ("push", B), ("push", B)]              # enable -> short push -> replace -> short push


def _run_splice_ops(stream, pipelined=False, group=1):
    """-> (outputs per push, IF per push (ordinary mode only), the ops' feed flags per push)"""
    from sdrplusplus_amd import radio

    ctx = make_ctx(ref_block=0)
    d, keep = radio.vfo_desc(SR, IF_RATE, BW, F0, "WFM")
    rd, rkeep = radio.rds_desc(IF_RATE)
    vid, pos, on = add_wfm(ctx, rds=False), 0, True
    for _ in range(3):
        ctx.push(stream[pos:pos + B])  # the stream has a history before the attach
        pos += B
    pre_if = None if pipelined else ctx.vfo_read_if(vid)
    ctx.vfo_set_rds(vid, rd, True, rkeep)
    if pipelined:
        ctx.set_pipelined(True, 1 | 32)
        ctx.set_pipeline_group(group)
    outs, ifs, fed, vids = [], [], [], []
    for op in SPLICE_OPS:
        if op[0] == "push":
            ctx.push(stream[pos:pos + op[1]])
            pos += op[1]
            fed.append(on)
            vids.append(vid)
            if not pipelined:
                outs.append(ctx.vfo_rds_read(vid))
                ifs.append(ctx.vfo_read_if(vid))
        elif op[0] in ("on", "off"):
            on = op[0] == "on"
            ctx.vfo_set_rds(vid, rd, on, rkeep)
        elif op[0] == "reset":
            ctx.vfo_reset(vid)
        else:
            vid = ctx.vfo_replace(vid, d, 3, keep)
    if pipelined:
        for k, v in enumerate(vids):
            ctx.result_wait(k + 1)
            data, cnt = C.POINTER(C.c_float)(), C.c_int()
            rc = ctx.L.sdrpp_result_rds(ctx.h, k + 1, v, C.byref(data), C.byref(cnt))
            assert rc == (0 if fed[k] else NOT_FOUND), (k, rc)
            outs.append(ctx.result_rds(k + 1, v) if fed[k] else np.zeros(0, np.complex64))
            ctx.result_release(k + 1)
        assert ctx.pipeline_stats()["pass_blocks"] == 0
        ctx.set_pipelined(False)
    ctx.close()
    return outs, ifs, fed, pre_if


_splice_cache = {}


@pytest.fixture
def splice_ordinary(backend, stream):
    """the schedule in ordinary mode, run once per backend and shared, unchanged, by the tests below"""
    if backend not in _splice_cache:
        _splice_cache[backend] = _run_splice_ops(stream)
    return _splice_cache[backend]


def test_switches_inside_the_splice_window(backend, stream, splice_ordinary):
    """A second switch while the set-aside line is still in force (fewer than 44 IF samples fed since the first): enable -> short push -> reset, enable ->
    short push -> disable / enable, reset -> short push -> reset, enable -> short push -> replace.  Against the yardstick fed the device's own IF: the run and
    every single push below 1e-5 of the RMS."""
    outs, ifs, fed, pre_if = splice_ordinary
    y = Yardstick(ideal=True)
    y.discriminate(pre_if)
    W, k = [], 0
    for op in SPLICE_OPS:
        if op[0] == "reset":
            y.fresh_demod()
        if op[0] == "push":
            W.append(y.process(ifs[k], feed=fed[k]))
            assert len(outs[k]) == len(W[-1]), (k, len(outs[k]), len(W[-1]))
            k += 1
    y.close()
    g, w = np.concatenate(outs), np.concatenate(W)
    assert len(w) > 150
    rel = rms(g - w) / rms(w)
    worst = max(rms(a - b) for a, b in zip(outs, W) if len(a)) / rms(w)
    print("[rds] switches inside the splice window: %.3g of the RMS, worst push %.3g" % (rel, worst))
    assert rel < 1e-5 and worst < 1e-5, (rel, worst)


@pytest.mark.parametrize("group", [1, 4])
def test_splice_path_pipelined_equals_the_ordinary_path(backend, stream, splice_ordinary, group):
    """The same schedule in pipelined mode (the line jobs run as roles of a tick, one level behind the feed): result_rds of every ticket equals the ordinary
    path's samples of that push bit for bit; pushes made while the branch was off hold nothing of it."""
    outs, _ifs, _fed, _pre = _run_splice_ops(stream, pipelined=True, group=group)
    want = splice_ordinary[0]
    assert len(outs) == len(want)
    for k, (a, b) in enumerate(zip(outs, want)):
        assert bits_equal(a, b), k


def test_replace_into_the_other_nco_mode_restarts_the_branch(backend, stream):
    """sdrpp_vfo_replace with keep & 2 into a description that runs the reference rotator: the branch's parameters move, its state starts cleared."""
    from sdrplusplus_amd import radio

    ctx = make_ctx()
    vid = add_wfm(ctx)
    y = Yardstick(ideal=False)
    for i in range(3):
        ctx.push(stream[i * B:(i + 1) * B])
        y.discriminate(ctx.vfo_read_if(vid))  # (the demodulator lives on through the replace: its discriminator has a previous sample)
    d, keep = radio.vfo_desc(SR, IF_RATE, BW, F0, "WFM", nco_mode=2)
    new = ctx.vfo_replace(vid, d, 3, keep)
    ctx.push(stream[3 * B:4 * B])
    got = ctx.vfo_rds_read(new)
    want = y.branch(y.discriminate(ctx.vfo_read_if(new)), cut=[1250])  # a fresh branch behind that discriminator
    assert len(got) == len(want) == 26
    assert rms(got - want) < 1e-5 * rms(want)
    y.close()
    ctx.close()


# ---- 8. behind an IF chain ---------------------------------------------------------------------------------------------------------------
def test_behind_an_if_chain(backend, stream):
    """Noise blanker on: the branch follows the chain's output (the yardstick is fed vfo_ifc_read)."""
    from sdrplusplus_amd import radio

    x = stream[:100000].copy()
    t = np.arange(len(x)) / SR
    for at in range(3000, len(x) - 100, 7001):  # bursts for the blanker: 12 samples (3 at the IF) of amplitude 10 on the carrier's frequency
        x[at:at + 12] += (10.0 * np.exp(2j * np.pi * F0 * t[at:at + 12])).astype(np.complex64)
    ctx = make_ctx()
    vid = add_wfm(ctx)
    ctx.vfo_set_if(vid, radio.if_desc(IF_RATE, nb=True, nb_level=4.0))
    y = Yardstick(ideal=True)
    G, W, changed = [], [], 0
    for i in range(20):
        ctx.push(x[i * B:(i + 1) * B])
        fed = ctx.vfo_ifc_read(vid)
        changed += int(np.sum(fed != ctx.vfo_read_if(vid)))
        G.append(ctx.vfo_rds_read(vid))
        W.append(y.process(fed))
        assert len(G[-1]) == len(W[-1])
    g, w = np.concatenate(G), np.concatenate(W)
    rel = rms(g - w) / rms(w)
    print("[rds] behind the noise blanker (%d samples blanked): %.3g of the RMS" % (changed, rel))
    assert changed > 5 and rel < 1e-5, (changed, rel)
    y.close()
    ctx.close()


# ---- 9. bits survive ---------------------------------------------------------------------------------------------------------------------
def test_bits_survive(backend):
    """120 differentially encoded biphase symbols at 1187.5 bit/s on the 57 kHz subcarrier: each bit decided from the real part of the 5 kS/s output (first
    half-symbol minus second half-symbol, differentially decoded); delay from the yardstick's output against the sent waveform.  Condition on the input,
    asserted on the yardstick alone: every bit after the first 30 equals the sent bit.  Then the device decides every one of those bits as the yardstick does."""
    r = np.random.default_rng(11)
    bits = r.integers(0, 2, 122)
    n = 101000
    x = broadcast(n, seed=12, bits=bits)
    ctx = make_ctx()
    vid = add_wfm(ctx)
    outs, ifs = run_cut(ctx, vid, x, B)
    ctx.close()
    y = Yardstick(ideal=True)
    w = np.concatenate([y.process(i) for i in ifs])
    y.close()
    g = np.concatenate(outs)
    assert len(g) == len(w) == 506
    sent = biphase(bits, n, SR)[::200]  # the sent waveform at 5 kS/s
    lags = np.arange(0, 100)  # (the filters' combined reach is about 100 outputs)
    corr = [abs(np.dot(w.real[k:k + 400], sent[:400])) for k in lags]
    delay = int(lags[int(np.argmax(corr))])
    sign = np.sign(np.dot(w.real[delay:delay + 400], sent[:400]))

    def decide(z):
        sym = []
        for k in range(len(bits)):
            lo = delay + k * 5000.0 / 1187.5
            a, m, b = int(round(lo)), int(round(lo + 2500.0 / 1187.5)), int(round(lo + 5000.0 / 1187.5))
            if b > len(z):
                break
            sym.append(sign * (np.sum(z.real[a:m]) - np.sum(z.real[m:b])) > 0)
        sym = np.asarray(sym, dtype=np.int64)
        return sym[1:] ^ sym[:-1]  # differential decoding: bit k + 1

    dw, dg = decide(w), decide(g)
    assert len(dw) >= 100
    assert np.array_equal(dw[30:], bits[1:1 + len(dw)][30:]), "TEST BUG: the yardstick does not recover the sent bits"
    assert np.array_equal(dg[30:], dw[30:])


# ---- 10. argument checks -----------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    from sdrplusplus_amd import capi, radio

    ctx = make_ctx()
    L, h = ctx.L, ctx.h
    rd, rkeep = radio.rds_desc(IF_RATE)
    assert L.sdrpp_abi_sizeof_rds_desc() == C.sizeof(capi.RdsDesc)
    d, keep = radio.vfo_desc(SR, 50e3, 12.5e3, -300e3, "NFM")
    nfm = ctx.vfo_add(d, keep)
    assert L.sdrpp_vfo_set_rds(h, nfm, C.byref(rd), 1) == UNSUPPORTED  # not a WFM VFO
    assert L.sdrpp_vfo_set_rds(h, 4711, C.byref(rd), 1) == NOT_FOUND   # unknown id
    assert L.sdrpp_vfo_rds_count(h, 4711) == NOT_FOUND
    wfm = add_wfm(ctx, rds=False)
    assert L.sdrpp_vfo_rds_count(h, wfm) == INVALID  # no branch
    bad, _k = radio.rds_desc(IF_RATE)
    bad.stage_decim[1] = 3
    assert L.sdrpp_vfo_set_rds(h, wfm, C.byref(bad), 1) == UNSUPPORTED  # bad stages, as sdrpp_vfo_set_af
    bad, _k = radio.rds_desc(IF_RATE)
    bad.n_stages = 5
    assert L.sdrpp_vfo_set_rds(h, wfm, C.byref(bad), 1) == INVALID
    bad, _k = radio.rds_desc(IF_RATE)
    bad.resamp_ntaps = 0
    assert L.sdrpp_vfo_set_rds(h, wfm, C.byref(bad), 1) == INVALID      # interp != decim without taps
    ok, _k = radio.rds_desc(IF_RATE)
    ok.interp, ok.decim, ok.resamp_ntaps, ok.resamp_taps = 1, 1, 0, None  # interp == decim with no taps: the polyphase stage is absent
    assert L.sdrpp_vfo_set_rds(h, wfm, C.byref(ok), 1) == 0
    ctx.push(broadcast(4000, seed=1))
    assert ctx.vfo_rds_count(wfm) == 32  # 1 000 IF samples through the decimators alone: / 32, first output at sample 0
    assert L.sdrpp_vfo_rds_count(h, wfm) == 32
    assert L.sdrpp_vfo_set_rds(h, wfm, None, 0) == 0
    assert L.sdrpp_vfo_rds_count(h, wfm) == INVALID
    assert L.sdrpp_pipeline_set_rds_results(h, 1) == INVALID  # outside pipelined mode
    assert L.sdrpp_set_pipelined(h, 1, 32) == INVALID and L.sdrpp_set_pipelined(h, 0, 0) == 0  # (the flag has its own call)
    ctx.close()


# ---- 11. shared bank ---------------------------------------------------------------------------------------------------------------------
def test_identical_descriptions_share_one_bank(backend):
    from sdrplusplus_amd import radio

    ctx = make_ctx()
    ids = [add_wfm(ctx, f0) for f0 in np.linspace(-350e3, 350e3, 8)]
    assert ctx.rds_bank_count() == 1
    other, okeep = radio.rds_desc(IF_RATE, out_rate=4000.0)
    ctx.vfo_set_rds(ids[0], other, True, okeep)
    assert ctx.rds_bank_count() == 2
    for v in ids[:-1]:
        ctx.vfo_set_rds(v, None)
    assert ctx.rds_bank_count() == 1
    ctx.vfo_remove(ids[-1])
    assert ctx.rds_bank_count() == 0
    ctx.close()
