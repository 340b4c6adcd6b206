"""The radio's IF chain on the device (sdrpp_vfo_set_if): NoiseBlanker -> PowerSquelch between a VFO's IF stream and its demodulator
(decoder_modules/radio/src/radio_module.h:84-96; dsp/noise_reduction/noise_blanker.h:38-57, power_squelch.h:33-50).

The pin is tests/golden/ifchain_ref.npz (the reference's two headers, compiled unmodified, run by tests/golden/make_ifchain_golden.py); the float32
restatement below is checked against it bit for bit and is then the yardstick for the device.

Both blocks DECIDE (a blanked sample jumps from level * amp to amp, a closed block goes to zero) and the device's IF differs from the oracle's by about
1e-7, so every comparison first asserts — on the yardstick's side alone — that its input keeps clear of the thresholds: |excess / level - 1| >= 1e-2 for
every sample, |block level - squelch level| >= 0.05 dB for every block.  An input that does not is a bug of the test."""
import os

import numpy as np
import pytest

import support as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ifchain_ref.npz")
f32 = np.float32


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


# ---- the float32 restatement ----------------------------------------------------------------------------------------------------------
class Blanker:
    """NoiseBlanker::process (noise_blanker.h:38-57): every operation in float32, in the reference's order."""

    def __init__(self, rate, level):
        self.set(rate, level)
        self.amp = f32(1.0)

    def set(self, rate, level):
        self.rate = f32(rate)
        self.inv = f32(1.0) - self.rate
        self.level = f32(level)

    def process(self, x):
        """-> (out, excess / level per sample; 0 where the input is exactly zero)"""
        x = np.asarray(x, np.complex64)
        re, im = x.real.astype(f32), x.imag.astype(f32)
        a = np.sqrt(re * re + im * im)  # float32 throughout: sqrtf((re * re) + (im * im))
        out = x.copy()
        ratio = np.zeros(len(x), f32)
        amp, inv, rate, level = self.amp, self.inv, self.rate, self.level
        for i in range(len(x)):
            ia = a[i]
            if ia != 0.0:
                amp = f32(f32(amp * inv) + f32(ia * rate))
                ex = f32(ia / amp)
                ratio[i] = ex / level
                if ex > level:
                    g = f32(f32(1.0) / ex)
                    out[i] = complex(f32(re[i] * g), f32(im[i] * g))
        self.amp = amp
        return out, ratio


def squelch(x, cut, level):
    """PowerSquelch::process per block of `cut` -> (out, level of every block in dB)."""
    x = np.asarray(x, np.complex64)
    out = x.copy()
    dbs = []
    pos = 0
    for c in cut:
        c = int(c)
        if c == 0:
            continue
        b = x[pos:pos + c]
        re, im = b.real.astype(f32), b.imag.astype(f32)
        a = np.sqrt(re * re + im * im)
        s = f32(0.0)
        for v in a:  # volk_32f_accumulator_s32f: sequential float sum
            s = f32(s + v)
        s = f32(s / f32(c))
        with np.errstate(divide="ignore"):
            db = f32(f32(10.0) * np.log10(s, dtype=f32))
        dbs.append(float(db))
        if not db >= f32(level):
            out[pos:pos + c] = 0
        pos += c
    assert pos == len(x), (pos, len(x))
    return out, np.asarray(dbs)


class Chain:
    """blanker (optional) -> squelch (optional), block by block; collects the clearances of everything it has decided"""

    def __init__(self, rate=None, nb_level=None, sq_level=None):
        self.nb = Blanker(rate, nb_level) if nb_level is not None else None
        self.sq_level = sq_level
        self.min_nb, self.min_sq = np.inf, np.inf

    def process(self, x, cut=None):
        y = np.asarray(x, np.complex64)
        if self.nb is not None:
            y, ratio = self.nb.process(y)
            nz = ratio[ratio != 0.0]
            if len(nz):
                self.min_nb = min(self.min_nb, float(np.min(np.abs(nz.astype(np.float64) - 1.0))))
        if self.sq_level is not None:
            y, dbs = squelch(y, [len(y)] if cut is None else cut, self.sq_level)
            if len(dbs):
                self.min_sq = min(self.min_sq, float(np.min(np.abs(dbs - self.sq_level))))
        return y

    def assert_clear(self):
        assert self.min_nb >= 1e-2, "TEST BUG: a sample within 1 %% of the blanker's threshold (%.3g)" % self.min_nb
        assert self.min_sq >= 0.05, "TEST BUG: a block within 0.05 dB of the squelch level (%.3g dB)" % self.min_sq


def _agree(backend, got, want, what):
    """emulator: bit for bit.  Device: the same decisions (zeros where the yardstick has zeros and nowhere else is implied by the bound) and every sample
    within 1e-5 relative."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if backend == "emu":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, float(np.max(np.abs(got - want), initial=0.0)))
        return 0.0
    assert np.array_equal(got == 0, want == 0), what + ": squelch decisions differ"
    den = np.maximum(np.abs(want), 1e-30)
    worst = float(np.max(np.abs(got - want) / den, initial=0.0))
    print("[ifchain] %s: max relative error %.3g" % (what, worst))
    assert worst <= 1e-5, (what, worst)
    return worst


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def wide_signal(sr, n, f0, if_rate, seed, n_imp=0, fade=False, amp=0.05, mod=None, imp_len=1, imp_amp=2.0):
    """A carrier of amplitude `amp` at f0 (+ `mod`(t): phase in rad) + noise that arrives at the IF with sigma ~0.004, + `n_imp` bursts of amplitude `imp_amp`, `imp_len` IF samples
    long (a narrow channel filter needs several to let them through), + (fade) a silent stretch and a 60 dB fade over the second half."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * t + (mod(t) if mod is not None else 0.0)
    x = amp * np.exp(1j * ph)
    g = np.ones(n)
    if fade:
        g[n // 4:n // 4 + n // 8] = 0.0
        g[n // 2:] = 10.0 ** (-3.0 * np.arange(n - n // 2) / (n - n // 2))
    x = x * g
    sig = 0.004 * np.sqrt(sr / if_rate)
    x = x + g * sig * (r.standard_normal(n) + 1j * r.standard_normal(n)) / np.sqrt(2.0)
    w = int(round(sr / if_rate)) * imp_len
    for at in r.choice(np.arange(4 * w, n - 4 * w, 8 * w), n_imp, replace=False):
        x[at:at + w] += imp_amp * np.exp(1j * (ph[at:at + w] + r.random() * 2 * np.pi))
    return x.astype(np.complex64)


def _ctx(max_push, ref_block=0):
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max_push)
    ctx.set_reference_block(ref_block)
    return ctx


def _if_cut(chain, x, blocks):
    """IF samples the oracle's RxVFO delivers per reference block (drives the oracle over x)."""
    out, pos = [], 0
    for n in blocks:
        out.append(chain.vfo_process(x[pos:pos + n]))
        pos += n
    return out


# ---- 1. the restatement against the reference's recorded outputs (passes without the feature) --------------------------------------------
def test_restatement_equals_reference_fixture():
    z = np.load(GOLDEN)
    assert len(z["names"]) >= 5
    blanked = closed = 0
    for name in z["names"]:
        x, cut = z[name + "_x"], z[name + "_cut"]
        rate, nbl, sql = z[name + "_par"]
        nb = Chain(rate, nbl, None).process(x)
        sq = Chain(None, None, sql).process(x, cut)
        both = Chain(rate, nbl, sql).process(x, cut)
        for got, key in ((nb, "nb"), (sq, "sq"), (both, "both")):
            want = z[name + "_" + key]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, key)
        blanked += int(np.sum(nb != x))
        closed += int(np.sum((sq == 0) & (x != 0)))
    assert blanked > 20 and closed > 100, (blanked, closed)  # the fixture exercises both decisions


# ---- 2. the chain on a RAW VFO against the restatement applied to the device's own IF ----------------------------------------------------
RAW_SR, RAW_IF, RAW_F0 = 768e3, 24000.0, 100e3


@pytest.mark.parametrize("nb_level,sq_level", [(10.0, -20.0), (3.0, -30.0), (10.0, None), (None, -20.0)])
def test_raw_vfo_chain_equals_restatement(backend, nb_level, sq_level):
    """Noise blanker and squelch on a RAW VFO (768 kS/s -> 24 kS/s, carrier 0.05 + noise + 24 bursts of amplitude 2, a silent stretch and a 60 dB fade; reference
    blocks of 3 840 samples = 120 at the IF): the chain's output equals the restatement applied to the device's own `if_out` — bit for bit on the emulator; on the
    device the same blanking / squelch decisions and every sample within 1e-5 relative (measured on an MI355X: 0, bit-exact — hipcc's float divide and sqrt are
    correctly rounded and the tracker keeps the reference's operation order).  `if_out` itself stays the stream in front of the chain."""
    from sdrplusplus_amd import radio

    B, nblk, ref = 38400, 4, 3840
    x = wide_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=13, n_imp=24, fade=True)
    ctx = _ctx(B, ref)
    d, keep = radio.vfo_desc(RAW_SR, RAW_IF, RAW_IF, RAW_F0, "RAW")
    vid = ctx.vfo_add(d, keep)
    plain = ctx.vfo_add(d, keep)  # the same channel without a chain
    ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=nb_level is not None, nb_level=nb_level or 10.0, squelch=sq_level))
    ych = Chain(500.0 / RAW_IF, nb_level, sq_level)
    n_changed = n_zeroed = 0
    for b in range(nblk):
        ctx.push(x[b * B:(b + 1) * B])
        gi = ctx.vfo_read_if(vid)
        assert np.array_equal(gi, ctx.vfo_read_if(plain)), "the IF in front of the chain changed"
        assert len(gi) == B * RAW_IF / RAW_SR
        want = ych.process(gi, [120] * (len(gi) // 120))
        got = ctx.vfo_ifc_read(vid)
        _agree(backend, got, want, "block %d" % b)
        out = ctx.vfo_read(vid)  # a RAW VFO with a chain delivers the chain's output
        assert np.array_equal(out[:, 0] + 1j * out[:, 1], got)
        many = ctx.vfo_read_many([vid, vid, plain], which=[3, 1, 0])
        assert np.array_equal(many[0][:, 0] + 1j * many[0][:, 1], got) and np.array_equal(many[1][:, 0] + 1j * many[1][:, 1], gi)
        assert np.array_equal(many[2][:, 0] + 1j * many[2][:, 1], gi)
        n_changed += int(np.sum((want != gi) & (want != 0)))
        n_zeroed += int(np.sum((want == 0) & (gi != 0)))
    ych.assert_clear()
    if nb_level is not None:
        assert n_changed >= 10, n_changed
    if sq_level is not None:
        assert n_zeroed >= 120, n_zeroed
    ctx.close()


# ---- 3. chain + demodulator against the oracle -------------------------------------------------------------------------------------------
def _fm(dev, tone):
    return lambda t: (dev / tone) * np.sin(2 * np.pi * tone * t)


@pytest.mark.parametrize("mode,nb_level,sq_level", [("NFM", None, -22.0), ("AM", None, -20.0), ("USB", 5.0, -30.0), ("WFM", None, -20.0)])
def test_chain_and_demodulator_against_the_oracle(backend, mode, nb_level, sq_level):
    """OracleChain.vfo_process -> restatement per reference block -> OracleChain.demod_process against the device's audio, oracle pairing and tolerance of the
    no-chain tests of tests/test_parity_vfo.py (FM / AM: the pinned oracle; USB: the oracle with the ideal NCO, as test_closed_form_nco_vs_ideal_nco_oracle;
    audio RMS error below 1e-5 * max(1, rms))."""
    from sdrplusplus_amd import radio

    sr, B, nblk = 10e6, 50000, 8
    if_rate, bw = radio.RADIO_DEFAULTS[mode]
    f0 = {"NFM": 1.2e6, "AM": -2.2e6, "USB": 1.0014e6, "WFM": 0.9e6}[mode]
    mod = {"NFM": _fm(2500.0, 1000.0), "WFM": _fm(50e3, 1000.0), "AM": None, "USB": None}[mode]
    # (USB: a 2.8 kHz channel filter stretches any burst over ~9 IF samples while the tracker follows at rate 1 / 48: the excess it can reach is about 8.5
    # whatever the burst's amplitude — the blanker is exercised at level 5)
    x = wide_signal(sr, B * nblk, f0 + (300.0 if mode == "USB" else 0.0), if_rate, seed=1 if mode == "USB" else 5, n_imp=2 if nb_level is not None else 0, fade=True, mod=mod,
                    imp_len=3, imp_amp=10.0)
    ctx = _ctx(2 * B, B)
    d, keep = radio.vfo_desc(sr, if_rate, bw, f0, mode)
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_if(vid, radio.if_desc(if_rate, nb=nb_level is not None, nb_level=nb_level or 10.0, squelch=sq_level))
    och = S.OracleChain(sr, if_rate, bw, f0, S.MODES[mode], ideal_nco=(mode == "USB"))
    ych = Chain(500.0 / if_rate, nb_level, sq_level)
    closed = opened = blanked = 0
    for p in range(nblk // 2):  # pushes of two reference blocks
        want = []
        for b in (2 * p, 2 * p + 1):
            ifs = och.vfo_process(x[b * B:(b + 1) * B])
            y = ych.process(ifs)
            blanked += int(np.sum((y != ifs) & (y != 0)))
            closed += int(len(y) > 0 and not np.any(y != 0) and np.any(ifs != 0))
            opened += int(np.any(y != 0))
            want.append(och.demod_process(y))
        want = np.concatenate(want)
        ctx.push(x[2 * p * B:(2 * p + 2) * B])
        got = ctx.vfo_read(vid)
        assert got.shape == want.shape, (got.shape, want.shape)
        err = rms(got - want)
        print("[ifchain] %s push %d: audio rms error %.3g (rms %.3g)" % (mode, p, err, rms(want)))
        assert err < 1e-5 * max(1.0, rms(want)), (mode, p, err)
    ych.assert_clear()
    assert closed >= 1 and opened >= 2, (closed, opened)
    assert blanked >= 3 or nb_level is None, blanked
    ctx.close()


# ---- 4. how the stream is cut --------------------------------------------------------------------------------------------------------------
def _raw_pair_outputs(pushes, ref_block, x, nb_level=10.0, sq_level=-20.0, tune=None, f0=RAW_F0):
    from sdrplusplus_amd import radio

    ctx = _ctx(max(pushes), ref_block)
    d, keep = radio.vfo_desc(RAW_SR, RAW_IF, RAW_IF, f0, "RAW")
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=nb_level is not None, nb_level=nb_level or 10.0, squelch=sq_level))
    outs, ifs, pos = [], [], 0
    for i, n in enumerate(pushes):
        if tune:
            tune(ctx, vid, i)
        ctx.push(x[pos:pos + n])
        pos += n
        ifs.append(ctx.vfo_read_if(vid))
        outs.append(ctx.vfo_ifc_read(vid))
    ctx.close()
    return outs, ifs


def test_push_size_invariance_with_reference_blocks(backend):
    """With sdrpp_set_reference_block the squelch follows the reference's blocks, not the pushes: one push and pushes of 1, 7, 3, 11 and 8 blocks give the same
    stream, bit for bit.  (A VFO at offset 0: there the IF in front of the chain is itself bit-identical however the stream is pushed — the closed-form NCO of a
    tuned VFO is anchored where a push starts and rounds its last bit accordingly.)"""
    n = 38400 * 3
    x = wide_signal(RAW_SR, n, 1000.0, RAW_IF, seed=12, n_imp=16, fade=True)
    one, if1 = _raw_pair_outputs([n], 3840, x, f0=0.0)
    many, if2 = _raw_pair_outputs([3840 * k for k in (1, 7, 3, 11, 8)], 3840, x, f0=0.0)
    a, b = np.concatenate(one), np.concatenate(many)
    assert np.array_equal(np.concatenate(if1), np.concatenate(if2))
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.any(a == 0) and np.any(a != 0)


def test_ragged_pushes_cut_like_the_reference(backend):
    """Pushes that are no multiples of the reference block: a push is cut into whole reference blocks and a shorter last one (as the AGC's look-ahead is,
    tests/test_parity_vfo.py::test_agc_look_ahead_follows_reference_blocks), carried down to the IF rate — against the restatement over the device's own IF,
    cut where the oracle's RxVFO, driven with those blocks, delivers."""
    n, R = 38400 * 3, 3840
    pushes = [R + 37, 7001, R * 5 - 37, 1, 12345, 33333]
    pushes.append(n - sum(pushes))
    x = wide_signal(RAW_SR, n, RAW_F0, RAW_IF, seed=13, n_imp=0, fade=True)
    outs, ifs = _raw_pair_outputs(pushes, R, x, nb_level=None, sq_level=-20.0)
    och = S.OracleChain(RAW_SR, RAW_IF, RAW_IF, RAW_F0, None)
    ych = Chain(None, None, -20.0)
    pos = 0
    for i, (p, o, f) in enumerate(zip(pushes, outs, ifs)):
        blocks = [R] * (p // R) + ([p % R] if p % R else [])
        cut = [len(q) for q in _if_cut(och, x[pos:pos + p], blocks)]
        pos += p
        assert sum(cut) == len(f), (i, cut, len(f))
        _agree(backend, o, ych.process(f, cut), "push %d" % i)
    ych.assert_clear()


def test_squelch_follows_the_push_cut_without_reference_blocks(backend):
    """Reference block 0: one push = one block (power_squelch.h:33-50 decides per process() call)."""
    pushes = [38400, 19200, 57600, 3840, 34560]
    x = wide_signal(RAW_SR, sum(pushes), RAW_F0, RAW_IF, seed=13, n_imp=0, fade=True)
    outs, ifs = _raw_pair_outputs(pushes, 0, x, nb_level=None, sq_level=-24.0)
    ych = Chain(None, None, -24.0)
    states = set()
    for i, (o, f) in enumerate(zip(outs, ifs)):
        _agree(backend, o, ych.process(f), "push %d" % i)
        states.add(bool(np.any(o != 0)))
    ych.assert_clear()
    assert states == {True, False}


# ---- 5. state: parameter changes, reset, replace, detach -------------------------------------------------------------------------------------
def test_parameter_change_keeps_amp_and_reset_clears_it(backend):
    from sdrplusplus_amd import radio

    B, nblk = 38400, 6
    x = wide_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=3, n_imp=12, fade=False)
    ctx = _ctx(B)
    d, keep = radio.vfo_desc(RAW_SR, RAW_IF, RAW_IF, RAW_F0, "RAW")
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=True, nb_level=10.0))
    ych = Chain(500.0 / RAW_IF, 10.0, None)
    amps = []
    for b in range(nblk):
        if b == 2:  # setLevel: amp stays (noise_blanker.h:26-30)
            ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=True, nb_level=3.0))
            ych.nb.set(500.0 / RAW_IF, 3.0)
        if b == 3:  # squelch switched on beside it: amp stays
            ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=True, nb_level=3.0, squelch=-40.0))
            ych.sq_level = -40.0
        if b == 4:  # RxVFO::reset + NoiseBlanker::reset
            ctx.vfo_reset(vid)
            ych.nb.amp = f32(1.0)
        if b == 5:  # blanker off and on again: it starts at amp = 1
            ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=False, squelch=-40.0))
            ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=True, nb_level=3.0, squelch=-40.0))
            ych.nb.amp = f32(1.0)
        amps.append(float(ych.nb.amp))
        ctx.push(x[b * B:(b + 1) * B])
        _agree(backend, ctx.vfo_ifc_read(vid), ych.process(ctx.vfo_read_if(vid)), "block %d" % b)
    ych.assert_clear()
    assert amps[2] < 0.2 and amps[3] < 0.2  # (a chain that lost amp at the change would have restarted from 1: visible in the first samples' gains)
    ctx.close()


def test_chain_with_both_blocks_off_and_detach_equal_no_chain(backend):
    """Both blocks disabled, or the chain detached again: audio bit-identical to a VFO that never had a chain."""
    from sdrplusplus_amd import radio

    sr, B, nblk = 10e6, 50000, 5
    if_rate, bw = radio.RADIO_DEFAULTS["NFM"]
    x = wide_signal(sr, B * nblk, 1.2e6, if_rate, seed=6, fade=False, mod=_fm(2500.0, 1000.0))
    ctx = _ctx(B)
    d, keep = radio.vfo_desc(sr, if_rate, bw, 1.2e6, "NFM")
    never, off, detached = (ctx.vfo_add(d, keep) for _ in range(3))
    ctx.vfo_set_if(off, radio.if_desc(if_rate, nb=False, squelch=None))
    ctx.vfo_set_if(detached, radio.if_desc(if_rate, nb=False, squelch=-90.0))  # open on every block: the samples pass unchanged
    for b in range(nblk):
        if b == 2:
            ctx.vfo_set_if(detached, None)
        ctx.push(x[b * B:(b + 1) * B])
        a = ctx.vfo_read(never)
        for other in (off, detached):
            o = ctx.vfo_read(other)
            assert a.shape == o.shape and np.array_equal(a.view(np.uint32), o.view(np.uint32)), (b, other)
        if b >= 2:
            with pytest.raises(Exception):
                ctx.vfo_ifc_read(detached)
    ctx.close()


@pytest.mark.parametrize("keep4", [True, False])
def test_vfo_replace_moves_the_chain_under_keep_4(backend, keep4):
    from sdrplusplus_amd import radio

    B, nblk = 38400, 4
    x = wide_signal(RAW_SR, B * nblk, RAW_F0, RAW_IF, seed=3, n_imp=12, fade=False)
    ctx = _ctx(B)
    d, keep = radio.vfo_desc(RAW_SR, RAW_IF, RAW_IF, RAW_F0, "RAW")
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_if(vid, radio.if_desc(RAW_IF, nb=True, nb_level=3.0))
    ych = Chain(500.0 / RAW_IF, 3.0, None)
    for b in range(nblk):
        if b == 2:
            vid = ctx.vfo_replace(vid, d, 1 | (4 if keep4 else 0), keep)
        ctx.push(x[b * B:(b + 1) * B])
        if b >= 2 and not keep4:
            with pytest.raises(Exception):
                ctx.vfo_ifc_read(vid)
            continue
        _agree(backend, ctx.vfo_ifc_read(vid), ych.process(ctx.vfo_read_if(vid)), "block %d" % b)  # (amp carried: the yardstick's blanker lives on)
    ych.assert_clear()
    ctx.close()


# ---- 6. pipelined mode and launch groups ----------------------------------------------------------------------------------------------------
def _bank(pipelined, group, sr, nv, cfg, max_push, ref_block, levels):
    from sdrplusplus_amd import capi, radio, workloads

    ctx = capi.Context(0, max_push=max_push)
    vids, chained = [], {}
    for i, (mode, if_rate, bw, centre, _) in enumerate(workloads.vfo_plan(cfg, nv)):
        d, keep = radio.vfo_desc(sr, if_rate, bw, centre, mode)
        vids.append(ctx.vfo_add(d, keep))
        f = levels(i, mode, if_rate)
        if f is not None:
            ctx.vfo_set_if(vids[-1], f)
            chained[vids[-1]] = f
    ctx.set_reference_block(ref_block)
    if pipelined:
        ctx.set_pipelined(True, 1)
        if group:
            ctx.set_pipeline_group(group)
    return ctx, vids, chained


@pytest.mark.parametrize("group", [0, 3])
def test_pipelined_and_grouped_equal_the_ordinary_path(backend, group):
    """A cfg 4 bank (NFM / AM / USB) with a chain on a third of the VFOs: every output of the pipelined path — one block per launch, and groups of three — is
    bit-identical to the ordinary pass, and the blocks really ran as ticks with the chain as a role."""
    from sdrplusplus_amd import radio, workloads

    sr, nv = workloads.CFG[4]["sr"], 27
    pushes = [38400, 12503, 25597, 38400, 20000, 38400]
    x = workloads.synth(4, sum(pushes), seed=9, nvfo=nv)

    def levels(i, mode, if_rate):
        if i % 3 != (i // 3) % 3:  # a third of the VFOs, every mode among them
            return None
        return radio.if_desc(if_rate, nb=(mode == "USB"), nb_level=10.0, squelch=-30.0 if (i // 3) % 2 == 0 else -10.0)

    ca, va, cha = _bank(False, 0, sr, nv, 4, sum(pushes), int(sr / 1600), levels)
    cb, vb, chb = _bank(True, group, sr, nv, 4, sum(pushes), int(sr / 1600), levels)
    assert len(cha) == 9
    refs, pos = [], 0
    for n in pushes:
        blk = x[pos:pos + n]
        pos += n
        ca.push(blk)
        refs.append({v_b: ca.vfo_read(v_a).copy() for v_a, v_b in zip(va, vb)})
        cb.push(blk)
    zeros = 0
    for t, ref in enumerate(refs, start=1):
        got = cb.result_wait(t)
        for v, a in ref.items():
            b = got["vfo"][v]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, v)
            zeros += int(v in chb and a.size > 0 and not np.any(a != 0))
        cb.result_release(t)
    assert zeros >= 3, zeros  # the squelch at -10 dB closes its channels
    st = cb.pipeline_stats()
    assert st["tick_blocks"] >= 1 and st["pass_blocks"] == 0, st
    assert st["roles"].get("ifc", 0) >= 1, st["roles"]
    ca.close()
    cb.close()


# ---- 7. cfg 4's geometry on the device --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cfg4_geometry_pipelined_against_the_oracle():
    """128 mixed VFOs at 61.44 MS/s, 307 200-sample blocks, pipelined: squelch on the NFM third (alternately open at -30 dB and closed at -10 dB), blanker + squelch
    on the USB third, every VFO's audio against the oracle (restatement between its RxVFO and its demodulator), bar 1e-5 * max(1, rms) as test_cfg4_mixed_modes."""
    from sdrplusplus_amd import capi, radio, workloads

    capi.DEFAULT_LIB = os.path.join(S.ROOT, "sdrplusplus_amd", "csrc", "libsdrpp_gpu.so")
    sr, nv, B, nblk = workloads.CFG[4]["sr"], 128, 307200, 3
    x = workloads.synth(4, B * nblk, seed=4, nvfo=nv)
    plan = workloads.vfo_plan(4, nv)

    def levels(i, mode, if_rate):
        if mode == "NFM":
            return radio.if_desc(if_rate, squelch=-30.0 if (i // 3) % 2 == 0 else -10.0)
        if mode == "USB":
            return radio.if_desc(if_rate, nb=True, nb_level=10.0, squelch=-30.0 if (i // 3) % 2 == 0 else -12.0)
        return None

    ctx, vids, chained = _bank(True, 0, sr, nv, 4, B, 0, levels)
    # USB at arbitrary offsets: the oracle with the ideal NCO (the closed-form NCO's pairing, tests/test_parity_vfo.py)
    chains = [S.OracleChain(sr, r, bw, c, S.MODES[m], ideal_nco=(m == "USB")) for m, r, bw, c, _ in plan]
    ych = {}
    for i, (vid, (m, r, bw, c, _)) in enumerate(zip(vids, plan)):
        f = chained.get(vid)
        ych[vid] = Chain(f.nb_rate, f.nb_level if f.nb_enabled else None, f.squelch_level if f.squelch_enabled else None) if f is not None else None
    for b in range(nblk):
        ctx.push(x[b * B:(b + 1) * B])
    worst, closed = 0.0, 0
    for b in range(nblk):
        got = ctx.result_wait(b + 1)
        for vid, ch, (m, _, _, _, _) in zip(vids, chains, plan):
            ifs = ch.vfo_process(x[b * B:(b + 1) * B])
            if ych[vid] is not None:
                y = ych[vid].process(ifs)
                closed += int(not np.any(y != 0))
                ifs = y
            want = ch.demod_process(ifs)
            ga = got["vfo"][vid]
            assert ga.shape == want.shape, (m, vid, ga.shape, want.shape)
            e = rms(ga - want) / max(1.0, rms(want))
            worst = max(worst, e)
            assert e <= 1e-5, (m, vid, b, e)
        ctx.result_release(b + 1)
    for q in ych.values():
        if q is not None:
            q.assert_clear()
    print("[ifchain] cfg 4 geometry: worst audio error %.3g, %d closed blocks" % (worst, closed))
    assert closed >= 40, closed
    st = ctx.pipeline_stats()
    assert st["pass_blocks"] == 0 and st["roles"].get("ifc", 0) >= nblk, st
    ctx.close()
