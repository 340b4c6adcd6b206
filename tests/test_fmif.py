"""FMIF, the radio's FM IF noise reduction, on the device (sdrpp_vfo_set_fmnr): the last block of the IF chain, blanker -> squelch -> FMIF -> demodulator
(decoder_modules/radio/src/radio_module.h:84-96; dsp/noise_reduction/fm_if.h:45-77).

The pin is tests/golden/fmif_ref.npz: the reference's header, compiled unmodified around an exact DFT, run by tests/golden/make_fmif_golden.py.  The
yardstick is the float64 restatement below (sliding_window_view, one matmul, first-index argmax), checked against that fixture.

Comparison rule of every value test.  FMIF DECIDES: it keeps the one bin of largest magnitude.  The clearance of sample i,
m_i = (top - second) / top, is taken from the yardstick alone, on the very input the device's FMIF saw.
  * m_i >= 1e-4: |got - want| <= 1e-5 * S_i with S_i = sum_n |w[n]| * |x[i - (N-1) + n]| — each real output is a sum of 2 N products of float-rounded
    factors, worst case (2 N + 2) * 2^-24 * sqrt(2) = 5.6e-6 of S_i at N = 32; 1e-5 leaves under a factor of two for the order of the accumulation.
  * m_i < 1e-4 (rounding decides which bin wins) or top == 0: not skipped — the value must agree, within the same bound, with the yardstick's output for
    one of the bins whose magnitude lies within 1e-4 of the top.  With two such bins that is "the top bin or the runner-up"; right behind a cleared delay
    line (and where the stream falls silent) a window holds ONE non-zero sample, every bin has the same magnitude in exact arithmetic, and the
    reference's own recorded output sits on a third bin there (test 1 shows it on the fixture), so the set cannot be cut down to two.
  * |w[n]|, not w[n]: the Nuttall window's end points evaluate to -2.4e-17, not 0, and a window that holds only its newest sample would get a negative bound.
  * at most 1 % of a case's samples may have a non-zero top and m_i < 1e-4: more is a bug of the test's input, asserted on the yardstick's side.  (Exact-zero
    windows — the silent stretch of the fade — are not rounding decisions: every bin is 0 and so is the output; they are compared, not counted.)
  * a window whose top magnitude is below 1e-18 is treated like an exact-zero one: the float magnitudes sqrtf(re * re + im * im) the reference and the device
    compare underflow there (the squares leave float32's normal range at 1.1e-19), which the float64 yardstick does not see — the value must agree with the
    yardstick's output for SOME bin, all of which are below 1e-18 themselves.  (Met where a channel filter's tail runs out into a silent stretch.)
Measured worst |got - want| / S_i over the clear samples: 4.2e-7 on an MI355X and on the emulator alike (blanker + squelch + 32 bins; 3.2e-7 for FMIF alone); every test prints its own."""
import os

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import support as S
import test_ifchain as TI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fmif_ref.npz")
BINS = [9, 15, 31, 32]  # radio_module.h:31-36
UNDERFLOW = 1e-18        # ~10 * sqrt(FLT_MIN): below it re * re + im * im leaves float32's normal range and the magnitudes FMIF compares are 0 or denormal
RAW_SR, RAW_IF, RAW_F0 = TI.RAW_SR, TI.RAW_IF, TI.RAW_F0


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------------
def nuttall(n, N):  # window/nuttall.h:5-8, window/cosine.h:7-15
    a = (0.355768, 0.487396, 0.144232, 0.012604)
    return sum(((-1.0) ** i) * a[i] * np.cos(i * 2.0 * np.pi * n / N) for i in range(4))


class Fmif:
    """fm_if.h around an exact DFT: delay line of bins - 1 samples, X = DFT(w * window), first bin of largest magnitude, times e^{+j 2 pi idx (N // 2) / N}."""

    def __init__(self, bins):
        self.set_bins(bins)

    def set_bins(self, bins):
        N = self.N = int(bins)
        self.w = np.array([nuttall(float(n), float(N - 1)) for n in range(N)]).astype(np.float32).astype(np.float64)  # fftWin is a float array
        k, n = np.arange(N)[:, None], np.arange(N)[None, :]
        self.A = self.w[None, :] * np.exp(-2j * np.pi * ((k * (n - N // 2)) % N) / N)
        self.line = np.zeros(N - 1, np.complex128)

    def reset(self):
        self.line[:] = 0

    def process(self, x):
        """-> dict(out, Y (every bin's output), mag, clear (m_i; 0 where top == 0), S)"""
        x = np.asarray(x, np.complex64).astype(np.complex128)
        buf = np.concatenate([self.line, x])
        self.line = buf[len(x):].copy()
        if len(x) == 0:
            return dict(out=np.zeros(0, complex), Y=np.zeros((0, self.N), complex), mag=np.zeros((0, self.N)), clear=np.zeros(0), S=np.zeros(0))
        win = sliding_window_view(buf, self.N)
        Y = win @ self.A.T
        mag = np.abs(Y)
        idx = np.argmax(mag, axis=1)
        rows = np.arange(len(x))
        top = mag[rows, idx]
        rest = mag.copy()
        rest[rows, idx] = -1.0
        sec = np.max(rest, axis=1)
        with np.errstate(all="ignore"):
            clear = np.where(top > 0, (top - sec) / top, 0.0)
        return dict(out=Y[rows, idx], Y=Y, mag=mag, clear=clear, S=np.abs(win) @ np.abs(self.w))


class Tally:
    """what a case has compared so far: the worst error of the clear samples, and how many samples rounding decided"""

    def __init__(self):
        self.n = self.low = self.zero = 0
        self.worst = 0.0

    def check(self, got, r, what):
        got = np.asarray(got).astype(np.complex128)
        assert got.shape == r["out"].shape, (what, got.shape, r["out"].shape)
        if not len(got):
            return
        bound = 1e-5 * r["S"]
        top = np.max(r["mag"], axis=1)
        clear = r["clear"] >= 1e-4
        e_top = np.abs(got - r["out"])
        under = top < UNDERFLOW
        clear = clear & ~under
        near = (r["mag"] >= top[:, None] * (1.0 - 1e-4)) | under[:, None]
        e_near = np.min(np.where(near, np.abs(got[:, None] - r["Y"]), np.inf), axis=1)
        ok = np.where(clear, e_top <= bound, e_near <= bound)
        with np.errstate(all="ignore"):
            rel = np.where(clear & (r["S"] > 0), e_top / r["S"], 0.0)
        self.worst = max(self.worst, float(np.max(rel)))
        self.n += len(got)
        self.low += int(np.sum(~clear & ~under))
        self.zero += int(np.sum(under))
        bad = np.nonzero(~ok)[0]
        assert not len(bad), "%s: %d samples off, first at %d: |got - want| %.3g, bound %.3g, clearance %.3g" % (what, len(bad), bad[0], e_top[bad[0]], bound[bad[0]], r["clear"][bad[0]])

    def done(self, what):
        print("[fmif] %s: %d samples, worst |got - want| / S %.3g over the clear ones, %d decided by rounding, %d exact-zero windows" % (what, self.n, self.worst, self.low, self.zero))
        assert self.low <= 0.01 * self.n, "TEST BUG: %s: %d of %d samples with a clearance below 1e-4" % (what, self.low, self.n)


def c64(a):
    a = np.asarray(a)
    return (a[:, 0] + 1j * a[:, 1]).astype(np.complex64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fm_signal(sr, n, f0, if_rate, seed, fade=False):
    """carrier 0.05 at f0, FM with a 1 kHz tone (deviation a tenth of the IF rate), + noise that arrives at the IF with sigma ~0.004 (+ silence and a 60 dB fade)"""
    return TI.wide_signal(sr, n, f0, if_rate, seed, fade=fade, mod=TI._fm(if_rate / 10.0, 1000.0))


# ---- 1. the restatement against the reference's recorded outputs (passes without the feature) -------------------------------------------
def test_restatement_reproduces_the_reference_fixture():
    z = np.load(GOLDEN)
    assert len(z["names"]) >= 10
    seen_bins, third_bin = set(), 0
    for name in z["names"]:
        x, ops, y = z[name + "_x"], z[name + "_ops"], z[name + "_y"]
        f = Fmif(int(z[name + "_bins"]))
        t = Tally()
        pos = 0
        for kind, v in ops:
            if kind == 1:
                f.set_bins(v)
            elif kind == 2:
                f.reset()
            else:
                seen_bins.add(f.N)
                r = f.process(x[pos:pos + v])
                t.check(y[pos:pos + v], r, "%s at %d" % (name, pos))
                # the recorded winner against the yardstick's two best: the samples the rule's widening exists for
                order = np.argsort(-r["mag"], axis=1, kind="stable")
                idx = z[name + "_idx"][pos:pos + v].astype(int)
                third_bin += int(np.sum((idx != order[:, 0]) & (idx != order[:, 1]) & (np.max(r["mag"], axis=1) > 0)))
                pos += v
        assert pos == len(x)
        t.done(name)
        if "fade" in name:
            assert t.zero >= 50, (name, t.zero)
    assert seen_bins == set(BINS), seen_bins
    assert third_bin >= 1, third_bin


# ---- 2. FMIF alone on a RAW VFO against the restatement over the device's own IF ----------------------------------------------------------
def _raw(ctx, f0=RAW_F0):
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(RAW_SR, RAW_IF, RAW_IF, f0, "RAW")
    return ctx.vfo_add(d, keep), d, keep


@pytest.mark.parametrize("bins", BINS)
def test_raw_vfo_fmif_equals_restatement(backend, bins):
    """768 kS/s -> 24 kS/s, three pushes of 38 400 samples (1 200 at the IF: 4 full segments and one of 176 samples, whose last tile holds 16).  `if_out` stays
    the stream in front of the chain and equals a twin VFO's; vfo_read, vfo_ifc_read and vfo_read_many(which = 3) deliver the same block."""
    B, nblk = 38400, 3
    x = fm_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=20 + bins)
    ctx = TI._ctx(B)
    vid, _, _ = _raw(ctx)
    plain, _, _ = _raw(ctx)
    ctx.vfo_set_fmnr(vid, True, bins)
    y, t = Fmif(bins), Tally()
    for b in range(nblk):
        ctx.push(x[b * B:(b + 1) * B])
        gi = ctx.vfo_read_if(vid)
        assert len(gi) == 1200 and np.array_equal(gi, ctx.vfo_read_if(plain)), "the IF in front of the chain changed"
        got = ctx.vfo_ifc_read(vid)
        t.check(got, y.process(gi), "block %d" % b)
        assert bits_equal(c64(ctx.vfo_read(vid)), got)
        many = ctx.vfo_read_many([vid, vid, plain], which=[3, 1, 0])
        assert bits_equal(c64(many[0]), got) and bits_equal(c64(many[1]), gi) and bits_equal(c64(many[2]), gi)
    t.done("raw, %d bins" % bins)
    ctx.close()


# ---- 3. the whole chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [15, 32])
def test_blanker_squelch_fmif_together(backend, bins):
    """Blanker (level 10), squelch (-20 dB) and FMIF with reference blocks of 3 840 samples (120 at the IF), on a signal with bursts, a silent stretch and a 60 dB
    fade: closed blocks reach FMIF as zeros, and the N - 1 samples behind them see those zeros.  Yardstick: the float32 restatement of tests/test_ifchain.py over
    the device's own IF, then the FMIF restatement over its output."""
    from sdrplusplus_amd import radio

    B, nblk, ref = 38400, 4, 3840
    x = TI.wide_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=13, n_imp=24, fade=True, mod=TI._fm(2400.0, 1000.0))
    ctx = TI._ctx(B, ref)
    vid, _, _ = _raw(ctx)
    plain, _, _ = _raw(ctx)
    ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=True, nb_level=10.0, squelch=-20.0))
    ctx.vfo_set_fmnr(vid, True, bins)
    ych, y, t = TI.Chain(500.0 / RAW_IF, 10.0, -20.0), Fmif(bins), Tally()
    closed = after = 0
    for b in range(nblk):
        ctx.push(x[b * B:(b + 1) * B])
        gi = ctx.vfo_read_if(vid)
        assert np.array_equal(gi, ctx.vfo_read_if(plain))
        mid = ych.process(gi, [120] * (len(gi) // 120))
        got = ctx.vfo_ifc_read(vid)
        t.check(got, y.process(mid), "block %d" % b)
        assert bits_equal(c64(ctx.vfo_read(vid)), got)
        z = (mid == 0) & (gi != 0)
        closed += int(np.sum(z))
        after += int(np.sum(~z[1:] & z[:-1]))
    ych.assert_clear()
    t.done("chain, %d bins" % bins)
    assert closed >= 120 and after >= 1, (closed, after)  # a closed block, and an open one behind it
    ctx.close()


def test_nfm_behind_fmif_against_the_oracle_demodulator(backend):
    """One NFM VFO (10 MS/s -> 50 kS/s) with 15-bin FMIF: the oracle's demodulator, fed with the yardstick's FMIF output over the device's own IF, against the
    device's audio — RMS error below the project's 1e-5 (BASELINE.json), over the stretches with no sample decided by rounding within the audio filter's reach
    (there the device may keep the neighbouring bin, a different sample: the rule above compares those at the chain's output)."""
    from sdrplusplus_amd import radio

    sr, B, nblk, bins = 10e6, 50000, 6, 15
    if_rate, bw = radio.RADIO_DEFAULTS["NFM"]
    x = TI.wide_signal(sr, B * nblk, 1.2e6, if_rate, seed=5, mod=TI._fm(2500.0, 1000.0))
    ctx = TI._ctx(B)
    d, keep = radio.vfo_desc(sr, if_rate, bw, 1.2e6, "NFM")
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_fmnr(vid, True, bins)
    och = S.OracleChain(sr, if_rate, bw, 1.2e6, S.MODES["NFM"])
    y, t = Fmif(bins), Tally()
    reach = max(int(d.audio_ntaps), 1) + 1
    errs, used, total, dirty = [], 0, 0, 0
    for b in range(nblk):
        blk = x[b * B:(b + 1) * B]
        ctx.push(blk)
        och.vfo_process(blk)  # (its RxVFO runs along; the demodulator is fed the yardstick over the DEVICE's IF)
        gi = ctx.vfo_read_if(vid)
        r = y.process(gi)
        t.check(ctx.vfo_ifc_read(vid), r, "block %d" % b)
        want = och.demod_process(r["out"].astype(np.complex64))
        got = ctx.vfo_read(vid)
        assert got.shape == want.shape, (got.shape, want.shape)
        keepm = np.ones(len(want), bool)
        for i in np.nonzero(r["clear"] < 1e-4)[0]:
            keepm[i:i + reach] = False
        if dirty:
            keepm[:dirty] = False
        low = np.nonzero(r["clear"] < 1e-4)[0]
        dirty = max(0, int(low[-1]) + reach - len(want)) if len(low) else max(0, dirty - len(want))
        errs.append(np.sum((got[keepm] - want[keepm]) ** 2))
        used += int(np.sum(keepm)) * 2
        total += len(want) * 2
    t.done("nfm, %d bins" % bins)
    err = float(np.sqrt(np.sum(errs) / used))
    print("[fmif] NFM behind FMIF: audio rms error %.3g over %d of %d values" % (err, used, total))
    assert used >= 0.5 * total, (used, total)
    assert err < 1e-5, err
    ctx.close()


# ---- 4. how the stream is cut --------------------------------------------------------------------------------------------------------------
def _run_cut(pushes, x, bins):
    ctx = TI._ctx(max(pushes))
    vid, _, _ = _raw(ctx, f0=0.0)  # (offset 0: there the IF in front of the chain is itself bit-identical however the stream is pushed, tests/test_ifchain.py)
    ctx.vfo_set_fmnr(vid, True, bins)
    outs, ifs, pos = [], [], 0
    for n in pushes:
        ctx.push(x[pos:pos + n])
        pos += n
        ifs.append(ctx.vfo_read_if(vid))
        outs.append(ctx.vfo_ifc_read(vid))
    ctx.close()
    return np.concatenate(outs), np.concatenate(ifs)


@pytest.mark.parametrize("bins", BINS)
def test_push_cut_invariance(backend, bins):
    """3 x 38 400 samples against ragged pieces, among them 320 and 640 input samples — 10 and 20 at the IF, fewer than bins - 1 for 31 and 32, so a window reaches
    across three pushes: bit-identical."""
    n = 38400 * 3
    x = fm_signal(RAW_SR, n, 1000.0, RAW_IF, seed=31)
    ragged = [38400, 320, 640, 320, 7001, 1, 33333, 8192 + 17]
    ragged.append(n - sum(ragged))
    a, ia = _run_cut([38400] * 3, x, bins)
    b, ib = _run_cut(ragged, x, bins)
    assert bits_equal(ia, ib)
    assert len(a) == 3600 and bits_equal(a, b)
    assert np.any(a != 0)


# ---- 5. state ------------------------------------------------------------------------------------------------------------------------------
def test_bin_change_clears_off_on_continues_reset_clears(backend):
    B, nblk = 38400, 7
    x = fm_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=41)
    ctx = TI._ctx(B)
    vid, _, _ = _raw(ctx)
    ctx.vfo_set_fmnr(vid, True, 15)
    y, t = Fmif(15), Tally()
    for b in range(nblk):
        on = True
        if b == 2:  # setBins -> initBuffers: the delay line starts over
            ctx.vfo_set_fmnr(vid, True, 31)
            y.set_bins(31)
        if b == 3:  # unplugged: nothing runs, the block keeps what it held
            ctx.vfo_set_fmnr(vid, False, 31)
            on = False
        if b == 4:  # plugged in again with the same bins: it continues from the delay line as it was left (the samples of block 3 never reached it)
            ctx.vfo_set_fmnr(vid, True, 31)
        if b == 5:  # RxVFO::reset + FMIF::reset
            ctx.vfo_reset(vid)
            y.reset()
        if b == 6:  # the same bin count again: nothing is cleared
            ctx.vfo_set_fmnr(vid, True, 31)
        ctx.push(x[b * B:(b + 1) * B])
        gi = ctx.vfo_read_if(vid)
        if not on:
            with pytest.raises(Exception):
                ctx.vfo_ifc_read(vid)
            assert bits_equal(c64(ctx.vfo_read(vid)), gi)
            continue
        stale = y.line.copy()
        r = y.process(gi)
        t.check(ctx.vfo_ifc_read(vid), r, "block %d" % b)
        if b == 4:  # the check has teeth: a cleared (or a refreshed) delay line gives other first samples
            fresh = Fmif(31)
            assert np.any(np.abs(fresh.process(gi)["out"][:30] - r["out"][:30]) > 1e-3 * np.max(np.abs(r["out"][:30]))) and np.any(stale != 0)
    t.done("state")
    ctx.close()


@pytest.mark.parametrize("keep4", [True, False])
def test_vfo_replace_moves_fmif_under_keep_4(backend, keep4):
    B, nblk = 38400, 4
    x = fm_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=43)
    ctx = TI._ctx(B)
    vid, d, keep = _raw(ctx)
    ctx.vfo_set_fmnr(vid, True, 31)
    y, t = Fmif(31), Tally()
    for b in range(nblk):
        if b == 2:
            vid = ctx.vfo_replace(vid, d, 1 | (4 if keep4 else 0), keep)
        ctx.push(x[b * B:(b + 1) * B])
        if b >= 2 and not keep4:
            with pytest.raises(Exception):
                ctx.vfo_ifc_read(vid)
            continue
        t.check(ctx.vfo_ifc_read(vid), y.process(ctx.vfo_read_if(vid)), "block %d" % b)  # (bins, switch and delay line carried: the yardstick's block lives on)
    t.done("replace")
    ctx.close()


def test_fmif_disabled_equals_a_vfo_that_never_had_the_call(backend):
    from sdrplusplus_amd import radio

    sr, B, nblk = 10e6, 50000, 6
    if_rate, bw = radio.RADIO_DEFAULTS["NFM"]
    x = TI.wide_signal(sr, B * nblk, 1.2e6, if_rate, seed=6, mod=TI._fm(2500.0, 1000.0))
    ctx = TI._ctx(B)
    d, keep = radio.vfo_desc(sr, if_rate, bw, 1.2e6, "NFM")
    never, off, unplugged = (ctx.vfo_add(d, keep) for _ in range(3))
    ctx.vfo_set_fmnr(off, False, 15)
    ctx.vfo_set_fmnr(unplugged, True, 9)
    diff = 0
    for b in range(nblk):
        if b == 2:
            ctx.vfo_set_fmnr(unplugged, False, 9)
        ctx.push(x[b * B:(b + 1) * B])
        a = ctx.vfo_read(never)
        assert bits_equal(a, ctx.vfo_read(off)), b
        with pytest.raises(Exception):
            ctx.vfo_ifc_read(off)
        if b < 2:
            diff += int(np.sum(ctx.vfo_read(unplugged) != a))
        if b >= 4:  # (the audio low-pass — 304 taps, blocks of 250 — remembers FMIF's output for two blocks)
            assert d.audio_ntaps <= 2 * len(a) and bits_equal(a, ctx.vfo_read(unplugged)), b
    assert diff > 400, diff
    ctx.close()


# ---- 6. pipelined mode and launch groups ---------------------------------------------------------------------------------------------------
def _bank(pipelined, group, sr, nv, max_push, ref_block):
    from sdrplusplus_amd import capi, radio, workloads

    ctx = capi.Context(0, max_push=max_push)
    vids, n_fm = [], 0
    for i, (mode, if_rate, bw, centre, _) in enumerate(workloads.vfo_plan(3, nv)):
        d, keep = radio.vfo_desc(sr, if_rate, bw, centre, mode)
        vids.append(ctx.vfo_add(d, keep))
        if i % 2 == 0:  # FMIF on every other VFO, all presets; a squelch in front of it on one
            ctx.vfo_set_fmnr(vids[-1], True, BINS[(i // 2) % 4])
            n_fm += 1
        if i == 2:
            ctx.vfo_set_if(vids[-1], radio.if_desc(if_rate, squelch=-60.0))
    ctx.set_reference_block(ref_block)
    if pipelined:
        ctx.set_pipelined(True, 1)
        if group:
            ctx.set_pipeline_group(group, adaptive=False)
    return ctx, vids, n_fm


@pytest.mark.parametrize("group", [0, 4])
def test_pipelined_and_grouped_equal_the_ordinary_path(backend, group):
    """A WFM bank (cfg 3's plan, 10 MS/s) with FMIF on every other VFO: every output of the pipelined path — a block per launch, and groups of four — is
    bit-identical to the ordinary pass; the blocks ran as ticks with the chain's role, and no role or pass form has a new name."""
    from sdrplusplus_amd import capi, workloads

    sr, nv = workloads.CFG[3]["sr"], 6
    pushes = [50000, 12503, 25597, 50000, 20000, 50000]
    x = workloads.synth(3, sum(pushes), seed=9, nvfo=nv)
    ca, va, n_fm = _bank(False, 0, sr, nv, sum(pushes), 50000)
    cb, vb, _ = _bank(True, group, sr, nv, sum(pushes), 50000)
    assert n_fm == 3
    before = cb.pipeline_stats()["roles"].get("ifc", 0)
    refs, pos = [], 0
    for n in pushes:
        blk = x[pos:pos + n]
        pos += n
        ca.push(blk)
        refs.append({v_b: ca.vfo_read(v_a).copy() for v_a, v_b in zip(va, vb)})
        cb.push(blk)
    for tk, ref in enumerate(refs, start=1):
        got = cb.result_wait(tk)
        for v, a in ref.items():
            assert bits_equal(a, got["vfo"][v]), (tk, v)
        cb.result_release(tk)
    assert np.any(refs[-1][vb[0]] != refs[-1][vb[1]])
    st = cb.pipeline_stats()
    assert st["tick_blocks"] >= 1 and st["pass_blocks"] == 0, st
    assert st["roles"].get("ifc", 0) > before, st["roles"]
    L = capi.load()
    roles = []
    while L.sdrpp_pipeline_role_name(len(roles)) is not None:
        roles.append(L.sdrpp_pipeline_role_name(len(roles)).decode())
    assert roles[-1] == "ifc" and len(roles) == 54 and not any("fm" in r for r in roles), roles  # (the names of the parent commit: FMIF runs under the chain's role)
    forms = ca.pass_form_stats()
    assert forms.get("ifc", 0) >= len(pushes) and not any("fmif" in f or "fmnr" in f for f in forms), forms
    assert set(capi.pass_form_names()[:len(roles)]) == set(roles)
    ca.close()
    cb.close()


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    from sdrplusplus_amd import capi

    ctx = TI._ctx(38400)
    vid, d, keep = _raw(ctx)
    L = capi.load()
    assert L.sdrpp_vfo_set_fmnr(ctx.h, vid, 1, 33) == -5  # SDRPP_ERR_UNSUPPORTED
    assert L.sdrpp_vfo_set_fmnr(ctx.h, vid, 1, 1) == -2  # SDRPP_ERR_INVALID
    assert L.sdrpp_vfo_set_fmnr(ctx.h, vid + 1000, 1, 15) == -6  # SDRPP_ERR_NOT_FOUND
    assert L.sdrpp_vfo_set_fmnr(ctx.h, vid, 0, 2) == 0 and L.sdrpp_vfo_set_fmnr(ctx.h, vid, 1, 32) == 0
    later = ctx.vfo_add(d, keep)  # a VFO added after the call has FMIF off
    x = fm_signal(RAW_SR, 38400, RAW_F0, RAW_IF, seed=2)
    ctx.push(x)
    assert len(ctx.vfo_ifc_read(vid)) == 1200
    with pytest.raises(Exception):
        ctx.vfo_ifc_read(later)
    assert bits_equal(c64(ctx.vfo_read(later)), ctx.vfo_read_if(later))
    ctx.close()
