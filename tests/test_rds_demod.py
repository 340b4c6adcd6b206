"""The RDS demodulator on the device (sdrpp_vfo_set_rds_demod): AGC -> Costas loop -> complex band-pass -> Costas loop -> Mueller-Mueller clock recovery ->
slicer -> differential decoder, against the reference's RDSDemod (decoder_modules/radio/src/rds_demod.h) as tests/golden/make_rds_demod_golden.py recorded it
(tests/golden/rds_demod_ref.npz), on the emulator and (-m gpu) on a device.

THE BAR on soft values is the symbol branch's (tests/test_pager.py): max(1e-5 x the RMS of the reference's soft values, 4 x the fixture's per-symbol spread),
the spread being the reference's own answer to inputs changed by 1 +- 2^-24; the test demands that the bar stands at its 1e-5 floor for at least 90 % of a
case's symbols.  Counts and bits must be equal.  The exact rows are in tests/test_rds_demod_rows.py."""
import ctypes as C
import os

import numpy as np
import pytest

import rdsd_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rds_demod_ref.npz")
RATE = 5000.0
NOT_FOUND, INVALID, UNSUPPORTED = -6, -2, -5


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype.itemsize == 4 else np.array_equal(a, b)


def same(a, b):
    """(soft, bits) pairs equal bit for bit"""
    return bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])


def cat(parts):
    return (np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.float32), np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint8))


def make_ctx(max_push=4096):
    from sdrplusplus_amd import capi

    return capi.Context(0, max_push=max_push)


def add_transparent(ctx, demod=True, enabled=True, desc=None):
    """5 kS/s in and out, bandwidth = rate, offset 0: RxVFO does nothing, a source-1 demodulator sees the pushed samples themselves"""
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    vid = ctx.vfo_add(d, keep)
    if demod:
        rd, rk = desc if desc is not None else radio.rds_demod_desc(RATE, 1)
        ctx.vfo_set_rds_demod(vid, rd, enabled, rk)
    return vid


def pushes_of(x, size):
    return [x[i:i + size] for i in range(0, len(x), size)]


def run_cut(ctx, vids, x, sizes):
    """push x in pushes of `sizes` (cycled) -> per VFO the list of (soft, bits) per push"""
    out, pos, k = {v: [] for v in vids}, 0, 0
    while pos < len(x):
        s = min(sizes[k % len(sizes)], len(x) - pos)
        ctx.push(x[pos:pos + s])
        for v in vids:
            out[v].append(ctx.vfo_rds_demod_read(v))
        pos += s
        k += 1
    return out


def run_pipelined(ctx, vids, x, sizes, group, flags=None):
    """the same in pipelined mode with launch groups of `group` -> per VFO the list of (soft, bits) per push"""
    from sdrplusplus_amd import capi

    ctx.set_pipelined(True, capi.RESULT_RDS_BITS if flags is None else flags)
    ctx.set_pipeline_group(group)
    pos, k = 0, 0
    while pos < len(x):
        s = min(sizes[k % len(sizes)], len(x) - pos)
        ctx.push(x[pos:pos + s])
        pos += s
        k += 1
    out = {v: [] for v in vids}
    for i in range(k):
        ctx.result_wait(i + 1)
        for v in vids:
            out[v].append(ctx.result_rds_bits(i + 1, v))
        ctx.result_release(i + 1)
    out["groups"] = ctx.pipeline_group_stats()
    ctx.set_pipelined(False)
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def stream():
    return rdsd_ref.rds_signal(6000, seed=41, df=1.5, sigma=1e-3)[0]


def case_input(z, name):
    return (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)


# ---- 1. design -----------------------------------------------------------------------------------------------------------------------------
def test_design_equals_the_reference_bit_for_bit(golden):
    """sdrpp_design_rds_demod(5000) leaves every field as RDSDemod::init leaves its members: the AGC's four floats, both loops' coefficients, initial values and
    limits (the phase limits are the kernel's constants +-FL_M_PI and their float difference), the 190 complex taps, MM's fields and its bank."""
    from sdrplusplus_amd import capi, radio

    z = golden
    d, (taps, bank) = radio.rds_demod_desc(RATE)
    assert d.source == 0
    assert bits_equal(np.array([d.agc_set_point, d.agc_max_gain, d.agc_rate, d.agc_init_gain, d.agc_init_gain], np.float32), z["agc"])
    for l, want in ((d.loop1, z["loop1"]), (d.loop2, z["loop2"])):
        mine = np.array([l.alpha, l.beta, l.init_phase, l.init_freq, l.min_freq, l.max_freq], np.float32)
        assert bits_equal(mine, want[:6]), (mine, want)
        assert bits_equal(want[6:9], np.array([-rdsd_ref.FL_M_PI, rdsd_ref.FL_M_PI, rdsd_ref.FL_M_PI - (-rdsd_ref.FL_M_PI)], np.float32))
        assert bits_equal(want[9:11], mine[2:4])  # _initPhase, _initFreq: what reset() restores
    assert d.n_taps == 190 and taps.shape == (190,) and bits_equal(taps.view(np.float32), z["taps"].view(np.float32))
    assert bits_equal(np.array([d.omega, d.min_omega, d.max_omega, d.mu_gain, d.omega_gain], np.float32), z["mm"])
    assert (d.interp_phases, d.interp_ntaps) == (128, 8) and bits_equal(bank, z["bank"])
    L = capi.load()
    assert L.sdrpp_abi_sizeof_rdsd_desc() == C.sizeof(capi.RdsdDesc)
    assert L.sdrpp_design_rds_demod(0.0, C.byref(d), None, 0, None, 0) == INVALID
    t = np.zeros(2 * 100, np.float32)
    assert L.sdrpp_design_rds_demod(RATE, C.byref(capi.RdsdDesc()), t.ctypes.data_as(capi.c_float_p), 100, bank.ctypes.data_as(capi.c_float_p), 1024) == INVALID  # 190 taps do not fit


# ---- 2. the reference's recorded outputs ---------------------------------------------------------------------------------------------------
CASES = ["steady", "offset", "noisy", "weak", "cuts", "fresh", "reset"]


@pytest.mark.parametrize("name", CASES)
def test_fixture_case(backend, golden, name):
    """Every fixture case through a do-nothing 5 kS/s RAW VFO, source 1, in the reference's own block schedule, checked per push: counts equal, every bit equal,
    soft values inside the bar.  `fresh`: a new RDSDemod in mid-stream = detach and attach; `reset`: RDSDemod::reset() = sdrpp_vfo_rds_demod_reset.
    Largest |error| / bar: emulator 0 in every case (the emulator's cosf / sinf are the reference's C library; every other operation is the reference's);
    the device's figures are in DESIGN.md 8i."""
    from sdrplusplus_amd import radio

    z = golden
    x = case_input(z, name)
    ctx = make_ctx()
    vid = add_transparent(ctx)
    rd, rk = radio.rds_demod_desc(RATE, 1)
    got, pos = [], 0
    for b, s in enumerate(z[name + "_cut"]):
        if b in z[name + "_fresh"]:
            ctx.vfo_set_rds_demod(vid, None)
            ctx.vfo_set_rds_demod(vid, rd, True, rk)
        if b in z[name + "_reset"]:
            ctx.vfo_rds_demod_reset(vid)
        ctx.push(x[pos:pos + s])
        got.append(ctx.vfo_rds_demod_read(vid))
        pos += int(s)
    ctx.close()
    counts = np.array([len(g[0]) for g in got], np.int32)
    soft, bits = cat(got)
    want = z[name + "_soft"]
    floor = 1e-5 * rms(want)
    bar = np.maximum(floor, 4.0 * z[name + "_dev_max"].astype(np.float64))
    at_floor = float((bar == floor).mean())
    if len(soft) == len(want):
        err = np.abs(soft.astype(np.float64) - want.astype(np.float64))
        print("%s [%s]: %d symbols, largest |error| / bar %.3g (|error| %.3g), bar at its floor for %.1f %% of the symbols, bits differing %d" % (
            name, backend, len(want), float((err / bar).max()), float(err.max()), 100 * at_floor, int((bits != z[name + "_bits"]).sum())))
    assert at_floor >= 0.9, at_floor
    assert np.array_equal(counts, z[name + "_counts"]), (counts, z[name + "_counts"])
    assert np.array_equal(bits, z[name + "_bits"])
    assert (err <= bar).all(), float((err / bar).max())


def test_the_fixture_is_a_working_link(golden):
    """What the recorder's CPU runs showed, asserted on the committed data: 1187.5 symbols/s, no |soft| below 0.05 of the RMS in the second half, and in the
    offset case the decoded bits equal the transmitted ones over the second half at one constant lag."""
    z = golden
    for name in ("steady", "offset", "noisy", "weak"):
        s = z[name + "_soft"]
        assert len(s) == 4750
        half = s[len(s) // 2:]
        assert np.abs(half).min() > 0.05 * rms(half), name
    bits = z["offset_bits"]
    h = len(bits) // 2
    lag, errors = rdsd_ref.best_lag(bits[h:], z["offset_tx"][h:])
    assert errors == 0, (lag, errors)


# ---- 3. cut independence -------------------------------------------------------------------------------------------------------------------
def test_cut_independence_ordinary(backend, stream):
    """One push against cuts of 1, 7, 63, 64, 65 and 997 samples (and a mix), device against itself: the concatenated soft values and bits are equal bit for bit,
    and every symbol lies in the push its start lies in (the counts add up per stretch)."""
    x = stream[:3000]
    ctx = make_ctx()
    vid = add_transparent(ctx)
    whole = run_cut(ctx, [vid], x, [len(x)])[vid]
    ctx.close()
    assert len(whole[0][0]) in (712, 713)
    for sizes in ([1], [7], [63], [64], [65], [997], [1, 130, 64, 2]):
        n = len(x) if sizes != [1] else 700
        ctx = make_ctx()
        vid = add_transparent(ctx)
        parts = run_cut(ctx, [vid], x[:n], sizes)[vid]
        ctx.close()
        got = cat(parts)
        m = len(got[0])
        assert same(got, (whole[0][0][:m], whole[0][1][:m])), sizes
        assert abs(m - n * 1187.5 / RATE) <= 1.5, (sizes, m)


@pytest.mark.parametrize("group", [1, 3, 8])
def test_cut_independence_pipelined(backend, stream, group):
    """Pipelined, result flag 128 alone, launch groups of 1, 3 and 8, through a VFO that halves the rate (10 kS/s in, 5 kS/s out): pushes of one input sample
    give no sample every other time and pushes of a few give no symbol.  Every push's slice equals the ordinary run's, bit for bit."""
    from sdrplusplus_amd import radio

    x = np.repeat(stream[:1500], 2)  # (any 10 kS/s input: the two runs see the same)
    sizes = [1, 1, 1, 400, 3, 2, 1, 129, 64, 1000]
    d, keep = radio.vfo_desc(2 * RATE, RATE, RATE, 0.0, "RAW")

    def ctx_with_vfo():
        ctx = make_ctx()
        vid = ctx.vfo_add(d, keep)
        rd, rk = radio.rds_demod_desc(RATE, 1)
        ctx.vfo_set_rds_demod(vid, rd, True, rk)
        return ctx, vid

    ctx, vid = ctx_with_vfo()
    want = run_cut(ctx, [vid], x, sizes)[vid]
    ctx.close()
    ctx, vid = ctx_with_vfo()
    got = run_pipelined(ctx, [vid], x, sizes, group)[vid]
    ctx.close()
    assert len(got) == len(want) and sum(len(w[0]) for w in want) > 300
    assert any(len(w[0]) == 0 for w in want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (group, i, len(g[0]), len(w[0]))


# ---- 4. the control surface ---------------------------------------------------------------------------------------------------------------
def test_disable_enable_freezes_and_continues(backend, stream):
    """enabled = 0 freezes everything while the VFO's stream moves on; enabled = 1 with the same description continues: the outputs equal an uninterrupted run
    over the pushes the demodulator was switched on for."""
    from sdrplusplus_amd import radio

    blocks = pushes_of(stream[:3000], 500)
    rd, rk = radio.rds_demod_desc(RATE, 1)
    ctx = make_ctx()
    vid = add_transparent(ctx)
    out = []
    for i, blk in enumerate(blocks):
        if i == 2:
            ctx.vfo_set_rds_demod(vid, rd, False, rk)
        if i == 4:
            ctx.vfo_set_rds_demod(vid, rd, True, rk)
        ctx.push(blk)
        out.append(ctx.vfo_rds_demod_read(vid))
    ctx.close()
    assert len(out[2][0]) == 0 and len(out[3][0]) == 0
    ctx = make_ctx()
    vid = add_transparent(ctx)
    want = run_cut(ctx, [vid], np.concatenate(blocks[:2] + blocks[4:]), [500])[vid]
    ctx.close()
    assert same(cat(out), cat(want)) and [len(o[0]) for o in out[4:]] == [len(w[0]) for w in want[2:]]


def test_what_starts_cleared_and_what_does_not(backend, stream):
    """A new description, a fresh attach and sdrpp_vfo_rds_demod_reset start cleared (the first two like a new RDSDemod; reset() leaves MM's delay samples, as
    the reference does — the restatement says what that gives); sdrpp_vfo_reset and sdrpp_vfo_replace with keep & 2 leave the demodulator alone; a replace
    without the bit leaves the new handle without one."""
    from sdrplusplus_amd import radio

    blocks = pushes_of(stream[:2000], 500)
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    rd, rk = radio.rds_demod_desc(RATE, 1)
    rd2, rk2 = radio.rds_demod_desc(RATE, 1)
    rd2.agc_rate = 0.05

    def run(action):
        ctx = make_ctx()
        vid = add_transparent(ctx)
        out = []
        for i, blk in enumerate(blocks):
            if i == 2:
                vid = action(ctx, vid) or vid
            ctx.push(blk)
            out.append(ctx.vfo_rds_demod_read(vid))
        return ctx, vid, out

    c0, _, plain = run(lambda c, v: None)
    ctx = make_ctx()
    vid = add_transparent(ctx)
    fresh = run_cut(ctx, [vid], np.concatenate(blocks[2:]), [500])[vid]
    ctx.close()

    def reattach(c, v):
        c.vfo_set_rds_demod(v, None)
        c.vfo_set_rds_demod(v, rd, True, rk)

    def other_then_back(c, v):
        c.vfo_set_rds_demod(v, rd2, True, rk2)
        assert c.rdsd_bank_count() == 1  # (the tables are the same: the AGC's rate is not part of them)
        c.vfo_set_rds_demod(v, rd, True, rk)

    c1, _, re = run(reattach)
    c2, _, ob = run(other_then_back)
    c3, _, vr = run(lambda c, v: c.vfo_reset(v))
    c4, v4, mv = run(lambda c, v: c.vfo_replace(v, d, 3, keep))
    c5, _, rs = run(lambda c, v: c.vfo_rds_demod_reset(v))
    for i in range(2):
        assert same(re[2 + i], fresh[i]) and same(ob[2 + i], fresh[i]), i
    assert not same(plain[2], fresh[0])
    for i in range(4):
        assert same(vr[i], plain[i]) and same(mv[i], plain[i]), i
    # reset(): counts and bits against the restatement on both backends; soft values bit for bit on the emulator, whose arithmetic the restatement's is (on a device
    # reset() stands under the project's bar in test_fixture_case[reset], which has the spread this stream lacks)
    ref = rdsd_ref.RdsDemodRef(rdsd_ref.params_of(rd, *rk))
    want = []
    for i, blk in enumerate(blocks):
        if i == 2:
            ref.reset()
        want.append(ref.process(blk))
    for i in range(4):
        assert np.array_equal(rs[i][1], want[i][1]) and len(rs[i][0]) == len(want[i][0]), i
        assert backend == "gpu" or bits_equal(rs[i][0], want[i][0]), i
    new = c4.vfo_replace(v4, d, 1, keep)
    assert c4.L.sdrpp_vfo_rds_demod_count(c4.h, new) == INVALID and c4.rdsd_bank_count() == 0
    for c in (c0, c1, c2, c3, c4, c5):
        c.close()


def wfm_ctx(max_push=50000):
    """one WFM VFO at 250 kS/s in and out with its RDS branch"""
    from sdrplusplus_amd import radio

    ctx = make_ctx(max_push)
    d, keep = radio.vfo_desc(250e3, 250e3, 250e3, 0.0, "WFM")
    vid = ctx.vfo_add(d, keep)
    return ctx, vid, (d, keep)


def test_source_0_needs_and_follows_the_rds_branch(backend):
    """Source 0 without sdrpp_vfo_set_rds: SDRPP_ERR_INVALID; detaching the RDS branch detaches the demodulator; a switched-off RDS branch plans nothing for
    it; removing the VFO gives back the tables."""
    from sdrplusplus_amd import radio

    ctx, vid, _ = wfm_ctx()
    rd, rk = radio.rds_demod_desc(RATE, 0)
    assert ctx.L.sdrpp_vfo_set_rds_demod(ctx.h, vid, C.byref(rd), 1) == INVALID and b"RDS branch" in ctx.L.sdrpp_last_error(ctx.h)
    rds, rdsk = radio.rds_desc(250e3)
    ctx.vfo_set_rds(vid, rds, True, rdsk)
    ctx.vfo_set_rds_demod(vid, rd, True, rk)
    assert ctx.rdsd_bank_count() == 1 and ctx.vfo_rds_demod_count(vid) == 0
    x = (0.1 * np.exp(1j * 2 * np.pi * 0.01 * np.arange(20000))).astype(np.complex64)
    ctx.push(x)
    n_rds = ctx.L.sdrpp_vfo_rds_count(ctx.h, vid)
    assert n_rds == 400 and abs(ctx.vfo_rds_demod_count(vid) - 95) <= 1
    ctx.vfo_set_rds(vid, rds, False, rdsk)
    ctx.push(x)
    assert ctx.vfo_rds_demod_count(vid) == 0
    ctx.vfo_set_rds(vid, None)
    assert ctx.L.sdrpp_vfo_rds_demod_count(ctx.h, vid) == INVALID and ctx.rdsd_bank_count() == 0
    ctx.vfo_set_rds(vid, rds, True, rdsk)
    ctx.vfo_set_rds_demod(vid, rd, True, rk)
    ctx.vfo_remove(vid)
    assert ctx.rdsd_bank_count() == 0
    ctx.close()


def test_source_0_in_launch_groups(backend):
    """Source 0 pipelined in launch groups of 3, behind a WFM VFO that decimates (1 MS/s in, 250 kS/s IF: a bank of rate-preserving VFOs never forms a group,
    tick_host.h group_eligible): the pushes really go out grouped (sdrpp_pipeline_group_stats), the job is handed the push ends at the RDS branch's rate
    (Vfo::Rds::tk, not the IF stream's), and every push's count and slice equal the ordinary run's, bit for bit."""
    from sdrplusplus_amd import radio

    r = np.random.default_rng(9)
    x = (0.2 * np.exp(1j * np.cumsum(0.2 * r.standard_normal(280000)))).astype(np.complex64)
    sizes = [80000, 40000, 20000, 80000, 60000]

    def attach():
        ctx = make_ctx(300000)  # (a launch group holds at most max_push samples)
        d, keep = radio.vfo_desc(1e6, 250e3, 250e3, 0.0, "WFM")
        vid = ctx.vfo_add(d, keep)
        rds, rdsk = radio.rds_desc(250e3)
        ctx.vfo_set_rds(vid, rds, True, rdsk)
        rd, rk = radio.rds_demod_desc(RATE, 0)
        ctx.vfo_set_rds_demod(vid, rd, True, rk)
        return ctx, vid

    ctx, vid = attach()
    want = run_cut(ctx, [vid], x, sizes)[vid]
    ctx.close()
    ctx, vid = attach()
    out = run_pipelined(ctx, [vid], x, sizes, 3)
    ctx.close()
    got, groups = out[vid], out["groups"]
    assert groups["multi_groups"] >= 1 and groups["largest"] == 3, groups
    assert [len(w[0]) for w in want] == [len(g[0]) for g in got] and min(len(w[0]) for w in want) > 20
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), i


def test_argument_checks(backend):
    """Every error the header names, one per rejection, each with its reason in sdrpp_last_error."""
    from sdrplusplus_amd import capi, radio

    ctx = make_ctx()
    raw = add_transparent(ctx, demod=False)
    d, keep = radio.vfo_desc(50e3, 50e3, 12.5e3, 0.0, "NFM")
    nfm = ctx.vfo_add(d, keep)
    L, h = ctx.L, ctx.h
    good, gkeep = radio.rds_demod_desc(RATE, 1)

    def code(vid=raw, loop=None, **changes):
        s, k = radio.rds_demod_desc(RATE, 1)
        for name, value in changes.items():
            setattr(s, name, value)
        for name, value in (loop or {}).items():
            which, field = name.split(".")
            setattr(getattr(s, which), field, value)
        rc = L.sdrpp_vfo_set_rds_demod(h, vid, C.byref(s), 1)
        if rc:
            assert len(L.sdrpp_last_error(h)) > 10
        return rc

    assert code() == 0
    assert code(nfm) == UNSUPPORTED                       # source 1: only RAW VFOs
    assert code(source=2) == INVALID and code(source=-1) == INVALID
    assert code(source=0) == INVALID                      # no RDS branch on a RAW VFO
    assert L.sdrpp_vfo_set_rds_demod(h, 9999, C.byref(good), 1) == NOT_FOUND
    assert L.sdrpp_vfo_set_rds_demod(None, raw, C.byref(good), 1) == INVALID
    for bad in (float("nan"), float("inf")):
        for field in ("agc_set_point", "agc_max_gain", "agc_rate", "agc_init_gain", "omega", "mu_gain", "omega_gain", "min_omega", "max_omega"):
            assert code(**{field: bad}) == INVALID, (field, bad)
        for which in ("loop1", "loop2"):
            for field in ("alpha", "beta", "init_phase", "init_freq", "min_freq", "max_freq"):
                assert code(loop={which + "." + field: bad}) == INVALID, (which, field, bad)
    assert code(n_taps=0) == INVALID and code(n_taps=rdsd_ref.MAX_TAPS + 1) == INVALID and code(taps=capi.c_float_p()) == INVALID
    assert code(interp_ntaps=0) == INVALID and code(interp_ntaps=17) == INVALID and code(interp_bank=capi.c_float_p()) == INVALID
    assert code(interp_phases=0) == INVALID and code(interp_phases=1025) == INVALID
    assert code(min_omega=4.3, max_omega=4.3) == INVALID
    assert code(min_omega=1.0) == INVALID and code(min_omega=1.5, mu_gain=1.0) == INVALID  # min_omega - |mu_gain| >= 1
    assert code(max_omega=4096.0, mu_gain=1.0) == INVALID and code(max_omega=4095.0, mu_gain=1.0) == 0
    for which in ("loop1", "loop2"):
        assert code(loop={which + ".min_freq": 1.0, which + ".max_freq": 1.0}) == INVALID
        # the bounded-loop rule: max(|min|, |max|) + |alpha| <= 2 pi, |initial phase| <= pi
        assert code(loop={which + ".min_freq": -6.0, which + ".max_freq": 6.0, which + ".alpha": 0.2}) == 0
        assert code(loop={which + ".min_freq": -6.0, which + ".max_freq": 6.0, which + ".alpha": 0.3}) == INVALID
        assert code(loop={which + ".min_freq": -6.3, which + ".max_freq": 1.0, which + ".alpha": 0.0}) == INVALID
        assert code(loop={which + ".alpha": -5.0}) == INVALID
        assert code(loop={which + ".init_phase": 3.2}) == INVALID and code(loop={which + ".init_phase": -3.0}) == 0
    assert L.sdrpp_vfo_set_rds_demod(h, raw, None, 0) == 0  # detach
    assert L.sdrpp_vfo_rds_demod_count(h, raw) == INVALID and L.sdrpp_vfo_rds_demod_read(h, raw, None, None, 0) == INVALID
    assert L.sdrpp_vfo_rds_demod_device_buffers(h, raw, None, None, None) == INVALID and L.sdrpp_vfo_rds_demod_reset(h, raw) == INVALID
    assert L.sdrpp_vfo_rds_demod_count(h, 9999) == NOT_FOUND
    assert L.sdrpp_vfo_set_rds_demod(h, raw, C.byref(good), 0) == 0
    assert L.sdrpp_vfo_rds_demod_count(h, raw) == 0        # attached, switched off
    assert L.sdrpp_vfo_rds_demod_read(h, raw, None, None, -1) == INVALID
    assert L.sdrpp_pipeline_set_rds_bits_results(h, 1) == INVALID  # outside pipelined mode
    assert L.sdrpp_set_pipelined(h, 1, 128) == INVALID and L.sdrpp_set_pipelined(h, 0, 0) == 0  # (the flag has its own call)
    assert L.sdrpp_result_rds_bits(h, 1, raw, None, None, None) == INVALID  # nothing held
    assert L.sdrpp_rdsd_bank_count(None) == INVALID
    ctx.close()


def test_results_of_tickets_without_the_demodulator_or_the_flag(backend, stream):
    """Pipelined: a ticket pushed without flag 128, a VFO without the demodulator and one whose demodulator is switched off give SDRPP_ERR_NOT_FOUND; a released
    ticket SDRPP_ERR_INVALID; device buffers name the last ordinary push."""
    ctx = make_ctx()
    a = add_transparent(ctx)
    ctx.push(stream[:1000])
    want = ctx.vfo_rds_demod_read(a)
    soft, bits, n = C.c_void_p(), C.c_void_p(), C.c_int()
    assert ctx.L.sdrpp_vfo_rds_demod_device_buffers(ctx.h, a, C.byref(soft), C.byref(bits), C.byref(n)) == 0 and n.value == len(want[0]) > 200 and soft.value and bits.value
    ctx.close()
    ctx = make_ctx()
    a, off, none = add_transparent(ctx), add_transparent(ctx, enabled=False), add_transparent(ctx, demod=False)
    ctx.set_pipelined(True, 1)
    ctx.push(stream[:1000])
    ctx.pipeline_flush()
    assert ctx.L.sdrpp_pipeline_set_rds_bits_results(ctx.h, 1) == 0
    ctx.push(stream[1000:2000])
    ctx.result_wait(1)
    assert ctx.L.sdrpp_result_rds_bits(ctx.h, 1, a, None, None, None) == NOT_FOUND
    ctx.result_release(1)
    ctx.result_wait(2)
    assert len(ctx.result_rds_bits(2, a)[0]) > 200
    assert ctx.L.sdrpp_result_rds_bits(ctx.h, 2, off, None, None, None) == NOT_FOUND
    assert ctx.L.sdrpp_result_rds_bits(ctx.h, 2, none, None, None, None) == NOT_FOUND
    ctx.result_release(2)
    assert ctx.L.sdrpp_result_rds_bits(ctx.h, 2, a, None, None, None) == INVALID
    ctx.set_pipelined(False)
    ctx.close()


def test_every_other_output_of_a_mixed_bank_is_unchanged(backend):
    """A bank of a WFM VFO with RDS branch, an NFM VFO and a RAW VFO with the pager's symbol branch, ordinary and pipelined: with a demodulator on the WFM VFO's
    RDS branch (source 0) and one on the RAW VFO (source 1), audio, RDS samples, symbol branch outputs and the RAW VFO's IF are what they are without them,
    bit for bit; and a bank whose demodulators are switched off plans what a bank without them plans (the same outputs again)."""
    from sdrplusplus_amd import capi, radio

    sr, wfm_if = 1e6, 250e3  # (every VFO decimates: a bank with a rate-preserving VFO never forms a launch group)
    r = np.random.default_rng(5)
    x = (0.1 * (r.standard_normal(120000) + 1j * r.standard_normal(120000))).astype(np.complex64)
    pushes = pushes_of(x, 40000)

    def run(demod, pipelined):
        ctx = make_ctx(80000)
        d, keep = radio.vfo_desc(sr, wfm_if, wfm_if, 0.0, "WFM")
        w = ctx.vfo_add(d, keep)
        rds, rdsk = radio.rds_desc(wfm_if)
        ctx.vfo_set_rds(w, rds, True, rdsk)
        d, keep = radio.vfo_desc(sr, 50e3, 12.5e3, 40e3, "NFM")
        nfm = ctx.vfo_add(d, keep)
        d, keep = radio.vfo_desc(sr, 25e3, 12.5e3, -60e3, "RAW")
        raw = ctx.vfo_add(d, keep)
        sd, sk = radio.pager_desc(25e3, 2400.0)
        ctx.vfo_set_symbols(raw, sd, True, sk)
        if demod is not None:
            rd0, rk0 = radio.rds_demod_desc(RATE, 0)
            rd1, rk1 = radio.rds_demod_desc(RATE, 1)  # (the 5 kS/s description on a 25 kS/s channel: to the block the rate is only a number)
            ctx.vfo_set_rds_demod(w, rd0, demod, rk0)
            ctx.vfo_set_rds_demod(raw, rd1, demod, rk1)
        out = []
        if pipelined:
            ctx.set_pipelined(True, 1 | capi.RESULT_RDS | capi.RESULT_SYM | (capi.RESULT_RDS_BITS if demod else 0))
            ctx.set_pipeline_group(2)
            for p in pushes:
                ctx.push(p)
            for i in range(len(pushes)):
                res = ctx.result_wait(i + 1)
                out.append([res["vfo"][w], res["vfo"][nfm], res["vfo"][raw], ctx.result_rds(i + 1, w), *ctx.result_sym(i + 1, raw)])
                if demod:
                    assert len(ctx.result_rds_bits(i + 1, w)[0]) in (47, 48) and len(ctx.result_rds_bits(i + 1, raw)[0]) > 200
                ctx.result_release(i + 1)
            assert ctx.pipeline_group_stats()["multi_groups"] >= 1  # the pushes did go out as a group of 2
            ctx.set_pipelined(False)
        else:
            for p in pushes:
                ctx.push(p)
                out.append([ctx.vfo_read(w), ctx.vfo_read(nfm), ctx.vfo_read(raw), ctx.vfo_rds_read(w), *ctx.vfo_sym_read(raw)])
                if demod:
                    assert len(ctx.vfo_rds_demod_read(w)[0]) in (47, 48) and len(ctx.vfo_rds_demod_read(raw)[0]) > 200
        ctx.close()
        return out

    for pipelined in (False, True):
        base = run(None, pipelined)
        for demod in (True, False):
            got = run(demod, pipelined)
            for i, (g, b) in enumerate(zip(got, base)):
                for k, (p, q) in enumerate(zip(g, b)):
                    assert bits_equal(np.asarray(p).view(np.float32) if np.asarray(p).dtype == np.complex64 else np.asarray(p),
                                      np.asarray(q).view(np.float32) if np.asarray(q).dtype == np.complex64 else np.asarray(q)), (pipelined, demod, i, k)


# ---- 5. banks: the workgroup edges of four jobs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 4, 5, 9])
def test_banks_with_two_descriptions(backend, stream, nv):
    """nv transparent channels fed the same samples, two descriptions alternating (the radio's, and one with another band-pass and AGC rate): every channel
    equals the channel alone, bit for bit, in one push and in pushes of 130; the context holds two table pairs (one for nv = 1)."""
    from sdrplusplus_amd import radio

    x = stream[:1300]

    def desc(k):
        rd, rk = radio.rds_demod_desc(RATE, 1)
        if k % 2:
            rk[0][:] = rk[0][::-1].copy()
            rd.agc_rate = 0.2
        return rd, rk

    alone = []
    for k in range(min(nv, 2)):
        ctx = make_ctx()
        vid = add_transparent(ctx, desc=desc(k))
        alone.append(cat(run_cut(ctx, [vid], x, [len(x)])[vid]))
        ctx.close()
    if nv > 1:
        assert not same(alone[0], alone[1])
    for sizes in ([len(x)], [130]):
        ctx = make_ctx()
        vids = [add_transparent(ctx, desc=desc(k)) for k in range(nv)]
        assert ctx.rdsd_bank_count() == min(nv, 2)
        got = run_cut(ctx, vids, x, sizes)
        ctx.close()
        for k, v in enumerate(vids):
            assert same(cat(got[v]), alone[k % 2]), (nv, sizes, k)


# ---- 6. end to end, source 0 ------------------------------------------------------------------------------------------------------------
def test_end_to_end_behind_the_rds_branch(backend):
    """One WFM VFO at 250 kS/s in and out; the multiplex carries the fixture's kind of signal on a 57 kHz subcarrier (7.5 kHz deviation of 75 kHz full scale,
    beside a 1 kHz tone), for 1.2 s, pushed in blocks of 50 000.  Counts per push and bits equal the float32 restatement of RDSDemod::process fed the device's
    own sdrpp_vfo_rds_read samples; the bits of the last half equal the transmitted ones at one constant lag."""
    from sdrplusplus_amd import radio

    sr, n = 250e3, 300000
    t = np.arange(n) / sr
    r = np.random.default_rng(77)
    data = r.integers(0, 2, int(n / sr * 1187.5) + 2).astype(np.uint8)
    enc = np.bitwise_xor.accumulate(data)
    sym = t * 1187.5
    k = np.floor(sym).astype(np.int64)
    bb = np.where(enc[k] == 1, 1.0, -1.0) * np.sin(2 * np.pi * (sym - k))
    mpx = 0.5 * np.sin(2 * np.pi * 1000.0 * t) + 0.1 * bb * np.cos(2 * np.pi * 57000.0 * t + 0.4)
    x = (0.3 * np.exp(1j * 2 * np.pi * 75e3 * np.cumsum(mpx) / sr)).astype(np.complex64)
    ctx, vid, _ = wfm_ctx()
    rds, rdsk = radio.rds_desc(sr)
    ctx.vfo_set_rds(vid, rds, True, rdsk)
    rd, rk = radio.rds_demod_desc(RATE, 0)
    ctx.vfo_set_rds_demod(vid, rd, True, rk)
    ref = rdsd_ref.RdsDemodRef(rdsd_ref.params_of(rd, *rk))
    got, want = [], []
    for blk in pushes_of(x, 50000):
        ctx.push(blk)
        got.append(ctx.vfo_rds_demod_read(vid))
        want.append(ref.process(ctx.vfo_rds_read(vid)))
    ctx.close()
    assert [len(g[0]) for g in got] == [len(w[0]) for w in want]
    gs, gb = cat(got)
    ws, wb = cat(want)
    assert len(gb) in (1424, 1425, 1426) and np.array_equal(gb, wb)
    print("end to end [%s]: %d symbols, largest |soft - restatement| %.3g of the RMS" % (backend, len(gs), np.abs(gs - ws).max() / rms(ws)))
    h = len(gb) // 2
    lag, errors = rdsd_ref.best_lag(gb[h:], data[h:])
    assert errors == 0, (lag, errors)


# ---- 7. samples that are not numbers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["emu"], indirect=True)
def test_nan_and_inf_samples_end_inside_the_arrays(backend):
    """Emulator only — where a mistake costs a CPU process, not a GPU: a push containing NaN and +-inf samples ends, its count is within the outputs' capacity
    ceil(n / floor(min_omega - |mu gain|)) + 1 (Vfo::Rdsd::cap_of; floor(4.168 - 0.01) = 4 for the radio's description), and a fresh attach behind it gives the
    fixture's result."""
    from sdrplusplus_amd import radio

    z = np.load(GOLDEN)
    x = case_input(z, "cuts")[:1250].copy()
    bad = x.copy()
    bad[100] = np.complex64(complex(float("nan"), 0.0))
    bad[300] = np.complex64(complex(float("inf"), 1.0))
    bad[500] = np.complex64(complex(0.0, float("-inf")))
    rd, rk = radio.rds_demod_desc(RATE, 1)
    min_step = int(np.floor(np.float32(rd.min_omega) - np.float32(abs(rd.mu_gain))))
    assert min_step == 4
    ctx = make_ctx()
    vid = add_transparent(ctx)
    for blk in (bad, x, bad[:64], bad[90:110]):
        ctx.push(blk)
        n = ctx.vfo_rds_demod_count(vid)
        assert 0 <= n <= (len(blk) + min_step - 1) // min_step + 1, n
    ctx.vfo_set_rds_demod(vid, None)
    ctx.vfo_set_rds_demod(vid, rd, True, rk)
    got, pos = [], 0
    for s in z["cuts_cut"][:6]:
        ctx.push(case_input(z, "cuts")[pos:pos + s])
        got.append(ctx.vfo_rds_demod_read(vid))
        pos += int(s)
    ctx.close()
    m = int(z["cuts_counts"][:6].sum())
    assert [len(g[0]) for g in got] == list(z["cuts_counts"][:6])
    soft, bits = cat(got)
    bar = np.maximum(1e-5 * rms(z["cuts_soft"]), 4.0 * z["cuts_dev_max"][:m].astype(np.float64))
    assert np.array_equal(bits, z["cuts_bits"][:m]) and (np.abs(soft.astype(np.float64) - z["cuts_soft"][:m]) <= bar).all()
