"""The Meteor QPSK demodulator on the device (sdrpp_vfo_set_qpsk): root-raised-cosine FIR -> AGC -> QPSK Costas loop -> OQPSK delay -> complex Mueller-Mueller
clock recovery -> int8 pairs, against the reference's dsp::demod::Meteor (decoder_modules/meteor_demodulator/src/meteor_demod.h) and the module's sink as
tests/golden/make_meteor_golden.py recorded them (tests/golden/meteor_ref.npz), on the emulator and (-m gpu) on a device.

THE BAR on soft components is the project's (tests/test_pager.py, tests/test_rds_demod.py): max(1e-5 x the RMS of the reference's soft components, 4 x the
fixture's per-component spread), the spread being the reference's own answer to inputs changed by 1 +- 2^-24; the test demands that the bar stands at its 1e-5
floor for at least 90 % of a case's symbols.  Counts and the sign of every component must be equal.  The int8 pairs must equal, byte for byte, the sink's rule
applied in numpy to the device's own soft values; against the recorded pairs at most 1 % of the values may differ, none by more than 1 (a soft value within the
bar of an integer boundary may truncate to the neighbour).  On the emulator the soft values equal the recorded ones bit for bit: its cosf / sinf / atan2f /
sqrtf are the recorder's library."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "meteor_ref.npz")
RATE = 150000.0
SEG = 512  # SDRPP_QPSK_SEG (vfo_qpsk_kernels.h): samples per front job
NOT_FOUND, INVALID, UNSUPPORTED = -6, -2, -5
FL_M_PI = np.float32(3.1415926535)


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.complex64:
        a, b = a.view(np.float32), b.view(np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype.itemsize == 4 else np.array_equal(a, b)


def same(a, b):
    """(soft, packed) pairs equal bit for bit"""
    return bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])


def cat(parts):
    return (np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.complex64), np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 2), np.int8))


def sink(soft, scale=84.0):
    """the module's sinkHandler (main.cpp:197-200) in numpy: clamp<int>(v * scale, -127, 127), the conversion truncating towards zero; a NaN gives 0"""
    v = np.ascontiguousarray(soft).view(np.float32).reshape(-1, 2) * np.float32(scale)
    v = np.where(np.isnan(v), np.float32(0.0), np.clip(v, np.float32(-127.0), np.float32(127.0)))
    return np.trunc(v).astype(np.int8)


def make_ctx(max_push=8192):
    from sdrplusplus_amd import capi

    return capi.Context(0, max_push=max_push)


def meteor(broken=False, oqpsk=False, **kw):
    from sdrplusplus_amd import radio

    return radio.meteor_desc(broken=broken, oqpsk=oqpsk, **kw)


def add_transparent(ctx, demod=True, enabled=True, desc=None):
    """150 kS/s in and out, bandwidth = rate, offset 0: RxVFO does nothing, the demodulator sees the pushed samples themselves"""
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    vid = ctx.vfo_add(d, keep)
    if demod:
        rd, rk = desc if desc is not None else meteor()
        ctx.vfo_set_qpsk(vid, rd, enabled, rk)
    return vid


def pushes_of(x, size):
    return [x[i:i + size] for i in range(0, len(x), size)]


def run_cut(ctx, vids, x, sizes):
    """push x in pushes of `sizes` (cycled) -> per VFO the list of (soft, packed) per push"""
    out, pos, k = {v: [] for v in vids}, 0, 0
    while pos < len(x):
        s = min(sizes[k % len(sizes)], len(x) - pos)
        ctx.push(x[pos:pos + s])
        for v in vids:
            out[v].append(ctx.vfo_qpsk_read(v))
        pos += s
        k += 1
    return out


def run_pipelined(ctx, vids, x, sizes, group, with_soft=True, flags=None):
    """the same in pipelined mode with launch groups of `group` -> per VFO the list of (soft, packed) per push"""
    from sdrplusplus_amd import capi

    ctx.set_pipelined(True, capi.RESULT_QPSK if flags is None else flags)
    if with_soft and (flags is None or flags & capi.RESULT_QPSK):
        ctx.set_qpsk_results(True, True)
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
            out[v].append(ctx.result_qpsk(i + 1, v))
        ctx.result_release(i + 1)
    ctx.set_pipelined(False)
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case_input(z, name):
    key = name + "_x" if name + "_x" in z.files else str(z[name + "_xof"]) + "_x"
    return (z[key].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)[:int(z[name + "_cut"].sum())]


@pytest.fixture(scope="module")
def stream(golden):
    """a locked link with a carrier offset: the fixture's `offset` input"""
    return case_input(golden, "offset")


# ---- 1. design -----------------------------------------------------------------------------------------------------------------------------
def test_design_equals_the_reference_bit_for_bit(golden):
    """sdrpp_design_meteor with the module's arguments (main.cpp:66) leaves every field as Meteor::init leaves its members: the 33 root-raised-cosine taps, the
    AGC's four floats, the loop's coefficients, initial values and limits (the phase limits are the kernel's constants +-FL_M_PI and their float difference),
    MM's fields — with the limit 0.01 that init does not pass on — and its bank; sdrpp_design_root_raised_cosine alone gives the same taps."""
    from sdrplusplus_amd import capi, radio

    z = golden
    d, (taps, bank) = radio.meteor_desc()
    assert bits_equal(np.array([d.agc_set_point, d.agc_max_gain, d.agc_rate, d.agc_init_gain, d.agc_init_gain], np.float32), z["agc"])
    assert d.agc_max_gain == np.float32(10e6) and d.agc_init_gain == 1.0
    mine = np.array([d.loop.alpha, d.loop.beta, d.loop.init_phase, d.loop.init_freq, d.loop.min_freq, d.loop.max_freq], np.float32)
    want = z["loop"]
    assert bits_equal(mine, want[:6]), (mine, want)
    assert bits_equal(want[6:9], np.array([-FL_M_PI, FL_M_PI, FL_M_PI - (-FL_M_PI)], np.float32))
    assert bits_equal(want[9:11], mine[2:4])  # _initPhase, _initFreq: what reset() restores
    assert d.n_taps == 33 and taps.shape == (33,) and bits_equal(taps, z["taps"])
    assert bits_equal(capi.design_root_raised_cosine(33, capi._F32(0.6), 72000.0, 150000.0), z["taps"])
    assert bits_equal(np.array([d.omega, d.min_omega, d.max_omega, d.mu_gain, d.omega_gain], np.float32), z["mm"])
    assert (d.interp_phases, d.interp_ntaps) == (128, 8) and bits_equal(bank, z["bank"])
    assert d.soft_scale == 84.0 and (d.broken, d.oqpsk) == (0, 0)
    d2, _ = radio.meteor_desc(broken=True, oqpsk=True)
    assert (d2.broken, d2.oqpsk) == (1, 1)
    L = capi.load()
    assert L.sdrpp_abi_sizeof_qpsk_desc() == C.sizeof(capi.QpskDesc)
    t = np.zeros(64, np.float32)
    tp, bp = t.ctypes.data_as(capi.c_float_p), bank.ctypes.data_as(capi.c_float_p)
    assert L.sdrpp_design_root_raised_cosine(0, 0.6, 72000.0, 150000.0, tp, 64) == INVALID
    assert L.sdrpp_design_root_raised_cosine(65, 0.6, 72000.0, 150000.0, tp, 64) == INVALID
    assert L.sdrpp_design_root_raised_cosine(33, 0.6, 0.0, 150000.0, tp, 64) == INVALID
    assert L.sdrpp_design_meteor(72000.0, 150000.0, 33, 0.6, 0.1, 0.005, 0, 0, 1e-6, 0.01, C.byref(capi.QpskDesc()), tp, 32, bp, 1024) == INVALID  # 33 taps do not fit
    assert L.sdrpp_design_meteor(72000.0, 150000.0, 33, 0.6, 0.1, 0.005, 0, 0, 1e-6, 0.01, C.byref(capi.QpskDesc()), tp, 64, bp, 1023) == INVALID


def test_root_raised_cosine_takes_all_three_branches():
    """taps/root_raised_cosine.h has a tap in the middle (an odd count), two at +-Ts / (4 beta) (Ts = 8, beta = 0.5: t = +-4) and the general one; the first two
    stated here from their formulas, every tap finite, the filter even."""
    from sdrplusplus_amd import capi

    h = capi.design_root_raised_cosine(17, 0.5, 1.0, 8.0)
    assert np.isfinite(h).all() and np.array_equal(h, h[::-1])
    assert h[8] == np.float32((1.0 + 0.5 * (4.0 / np.pi - 1.0)) / 8.0)
    edge = ((1.0 + 2.0 / np.pi) * np.sin(np.pi / 2.0) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / 2.0)) * 0.5 / (8.0 * np.sqrt(2.0))
    assert abs(float(h[4]) - edge) <= 1e-9 and h[4] == h[12]
    assert abs(float(h[5]) - 0.5 * (float(h[4]) + float(h[6]))) < 0.01  # (the special taps lie on the curve of their neighbours)


# ---- 2. the reference's recorded outputs ---------------------------------------------------------------------------------------------------
CASES = ["steady", "offset", "noisy", "weak", "oqpsk", "broken", "cuts", "fresh", "reset", "reset_oqpsk", "mode"]


def run_case(z, name):
    """a fixture case in the reference's own block schedule -> the list of (soft, packed) per push"""
    x = case_input(z, name)
    broken, oqpsk = (int(v) for v in z[name + "_mode"])
    ops = {int(b): int(o) for b, o in z[name + "_ops"]}
    ctx = make_ctx()
    vid = add_transparent(ctx, desc=meteor(broken, oqpsk))
    got, pos = [], 0
    for b, s in enumerate(z[name + "_cut"]):
        if ops.get(b) == 1:  # a fresh Meteor
            ctx.vfo_set_qpsk(vid, None)
            rd, rk = meteor(broken, oqpsk)
            ctx.vfo_set_qpsk(vid, rd, True, rk)
        if ops.get(b) == 2:  # reset()
            ctx.vfo_qpsk_reset(vid)
        if ops.get(b) == 3:  # setOQPSK(true)
            ctx.vfo_qpsk_set_mode(vid, broken, True)
        ctx.push(x[pos:pos + s])
        got.append(ctx.vfo_qpsk_read(vid))
        pos += int(s)
    ctx.close()
    return got


@pytest.mark.parametrize("name", CASES)
def test_fixture_case(backend, golden, name):
    """Every fixture case through a do-nothing 150 kS/s RAW VFO, in the reference's own block schedule, checked per push: counts equal, the sign of every soft
    component equal, soft components inside the bar, the int8 pairs the sink's rule of the device's own soft values and within one step of the recorded pairs
    for all but 1 %.  `fresh`: a new Meteor in mid-stream = detach and attach; `reset`: Meteor::reset() = sdrpp_vfo_qpsk_reset — lastI and MM's delay samples
    stay (`reset_oqpsk`: in the mode in which lastI is read); `mode`: setOQPSK(true) = sdrpp_vfo_qpsk_set_mode.  Emulator: bit-equal soft values in every case.  The device's largest |error| / bar per case is in
    DESIGN.md 8j."""
    z = golden
    got = run_case(z, name)
    counts = np.array([len(g[0]) for g in got], np.int32)
    soft, packed = cat(got)
    want = z[name + "_soft"]
    w2 = want.view(np.float32).reshape(-1, 2).astype(np.float64)
    floor = 1e-5 * rms(w2)
    bar = np.maximum(floor, 4.0 * z[name + "_dev_max"].astype(np.float64))
    at_floor = float((bar == floor).all(axis=1).mean())
    if len(soft) == len(want):
        s2 = soft.view(np.float32).reshape(-1, 2).astype(np.float64)
        err = np.abs(s2 - w2)
        di = np.abs(packed.astype(np.int32) - z[name + "_i8"].astype(np.int32))
        print("%s [%s]: %d symbols, largest |error| / bar %.3g (|error| %.3g), bar at its floor for %.1f %% of the symbols, int8 values differing from the recorded %d (largest step %d)" % (
            name, backend, len(want), float((err / bar).max()), float(err.max()), 100 * at_floor, int((di != 0).sum()), int(di.max())))
    assert at_floor >= 0.9, at_floor
    assert np.array_equal(counts, z[name + "_counts"]), (counts, z[name + "_counts"])
    assert np.array_equal(s2 > 0, w2 > 0)
    assert (err <= bar).all(), float((err / bar).max())
    assert np.array_equal(packed, sink(soft))
    assert (di != 0).mean() <= 0.01 and di.max() <= 1
    if backend == "emu":
        assert bits_equal(soft, want) and np.array_equal(packed, z[name + "_i8"])


def test_the_fixture_is_a_working_link(golden):
    """What the recorder's CPU runs showed, asserted on the committed data: 72 000 symbols/s, and an open eye where the chain has locked — no |component| below
    0.3 of the RMS over the second half (the last quarter in the cases that start over in mid-stream)."""
    z = golden
    for name in CASES:
        s = z[name + "_soft"].view(np.float32).reshape(-1, 2)
        n = len(case_input(z, name))
        assert abs(len(s) - n * 72000.0 / RATE) <= 2.5, (name, len(s))
        tail = s[(3 * len(s)) // 4 if len(z[name + "_ops"]) else len(s) // 2:]
        assert np.abs(tail).min() >= 0.3 * rms(tail), name
        assert np.array_equal(z[name + "_i8"], sink(z[name + "_soft"])), name


# ---- 3. cut independence -------------------------------------------------------------------------------------------------------------------
CUTS = [[1], [63], [64], [65], [SEG - 1], [SEG], [SEG + 1], [1, 130, 64, 2, 2 * SEG + 1]]


def test_cut_independence_ordinary(backend, stream):
    """One push against cuts of 1, 63, 64, 65 samples, the front's segment size and one less and more (and a mix), device against itself: the concatenated soft
    symbols and int8 pairs are equal bit for bit, and every symbol lies in the push its start lies in (the counts add up per stretch)."""
    x = stream[:3000]
    ctx = make_ctx()
    vid = add_transparent(ctx)
    whole = run_cut(ctx, [vid], x, [len(x)])[vid]
    ctx.close()
    assert len(whole[0][0]) in (1440, 1441)
    for sizes in CUTS:
        n = len(x) if sizes != [1] else 300
        ctx = make_ctx()
        vid = add_transparent(ctx)
        parts = run_cut(ctx, [vid], x[:n], sizes)[vid]
        ctx.close()
        got = cat(parts)
        m = len(got[0])
        assert same(got, (whole[0][0][:m], whole[0][1][:m])), sizes
        assert abs(m - n * 72000.0 / RATE) <= 1.5, (sizes, m)


@pytest.mark.parametrize("group", [1, 4, 32])
def test_cut_independence_pipelined(backend, stream, group):
    """Pipelined, result flag 256 with the float pairs, launch groups of 1, 4 and 32, through a VFO that halves the rate (300 kS/s in, 150 kS/s out): pushes of
    one input sample give no sample every other time and no symbol half of the time.  Every push's slice equals the ordinary run's, bit for bit; the sizes at the
    channel's rate cover 1, 63, 64, 65 and the front's segment size and one less and more."""
    from sdrplusplus_amd import radio

    x = np.repeat(stream[:2400], 2)  # (any 300 kS/s input: the two runs see the same)
    sizes = [1, 1, 1, 2, 126, 128, 130, 3, 2 * (SEG - 1), 2 * SEG, 2 * (SEG + 1), 1, 4 * SEG + 2]
    d, keep = radio.vfo_desc(2 * RATE, RATE, RATE, 0.0, "RAW")

    def ctx_with_vfo():
        ctx = make_ctx()
        vid = ctx.vfo_add(d, keep)
        rd, rk = meteor()
        ctx.vfo_set_qpsk(vid, rd, True, rk)
        return ctx, vid

    ctx, vid = ctx_with_vfo()
    want = run_cut(ctx, [vid], x, sizes)[vid]
    ctx.close()
    ctx, vid = ctx_with_vfo()
    got = run_pipelined(ctx, [vid], x, sizes, group)[vid]
    ctx.close()
    assert len(got) == len(want) and sum(len(w[0]) for w in want) > 1000
    assert any(len(w[0]) == 0 for w in want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (group, i, len(g[0]), len(w[0]))


def test_pipelined_default_is_the_int8_pairs_alone(backend, stream):
    """Result flag 256 through sdrpp_set_pipelined's Python wrapper, without the switch: the float pairs are not delivered (NULL), the int8 pairs equal the
    ordinary run's."""
    sizes = [700, 1, 65, 900]
    ctx = make_ctx()
    vid = add_transparent(ctx)
    want = run_cut(ctx, [vid], stream[:2500], sizes)[vid]
    ctx.close()
    ctx = make_ctx()
    vid = add_transparent(ctx)
    got = run_pipelined(ctx, [vid], stream[:2500], sizes, 1, with_soft=False)[vid]
    ctx.close()
    for g, w in zip(got, want):
        assert g[0] is None and np.array_equal(g[1], w[1])


# ---- 4. the control surface ---------------------------------------------------------------------------------------------------------------
def test_disable_enable_freezes_and_continues(backend, stream):
    """enabled = 0 freezes everything while the VFO's stream moves on; enabled = 1 with the same description continues: the outputs equal an uninterrupted run
    over the pushes the demodulator was switched on for."""
    blocks = pushes_of(stream[:3000], 500)
    rd, rk = meteor()
    ctx = make_ctx()
    vid = add_transparent(ctx)
    out = []
    for i, blk in enumerate(blocks):
        if i == 2:
            ctx.vfo_set_qpsk(vid, rd, False, rk)
        if i == 4:
            ctx.vfo_set_qpsk(vid, rd, True, rk)
        ctx.push(blk)
        out.append(ctx.vfo_qpsk_read(vid))
    ctx.close()
    assert len(out[2][0]) == 0 and len(out[3][0]) == 0
    ctx = make_ctx()
    vid = add_transparent(ctx)
    want = run_cut(ctx, [vid], np.concatenate(blocks[:2] + blocks[4:]), [500])[vid]
    ctx.close()
    assert same(cat(out), cat(want)) and [len(o[0]) for o in out[4:]] == [len(w[0]) for w in want[2:]]


def test_set_mode_keeps_state(backend, stream):
    """sdrpp_vfo_qpsk_set_mode changes what the next push computes and nothing the demodulator holds: switched there and back between two pushes it equals the
    plain run; switched for good it differs from the plain run from that push on and from a demodulator attached with the mode (whose state started over);
    the same description with other modes through sdrpp_vfo_set_qpsk does what set_mode does."""
    blocks = pushes_of(stream[:2000], 500)

    def run(action, desc=None):
        ctx = make_ctx()
        vid = add_transparent(ctx, desc=desc)
        out = []
        for i, blk in enumerate(blocks):
            if i == 2:
                action(ctx, vid)
            ctx.push(blk)
            out.append(ctx.vfo_qpsk_read(vid))
        ctx.close()
        return out

    plain = run(lambda c, v: None)

    def there_and_back(c, v):
        c.vfo_qpsk_set_mode(v, True, True)
        c.vfo_qpsk_set_mode(v, False, False)

    def by_desc(c, v):
        rd, rk = meteor(oqpsk=True)
        c.vfo_set_qpsk(v, rd, True, rk)

    back = run(there_and_back)
    oq = run(lambda c, v: c.vfo_qpsk_set_mode(v, False, True))
    oq2 = run(by_desc)
    br = run(lambda c, v: c.vfo_qpsk_set_mode(v, True, False))
    for i in range(4):
        assert same(back[i], plain[i]), i
        assert same(oq[i], oq2[i]), i
    for other in (oq, br):
        assert same(other[0], plain[0]) and same(other[1], plain[1]) and not same(other[2], plain[2])
        assert len(other[2][0]) == len(plain[2][0])
    # the real parts of the first push in OQPSK mode are the plain run's up to where the changed symbols steer the clock: its first symbol's is the same bit for bit
    assert oq[2][0][0].real == plain[2][0][0].real and oq[2][0][0].imag != plain[2][0][0].imag
    ctx = make_ctx()
    vid = add_transparent(ctx, desc=meteor(oqpsk=True))
    fresh = run_cut(ctx, [vid], np.concatenate(blocks[2:]), [500])[vid]
    ctx.close()
    assert not same(oq[2], fresh[0])


def test_what_starts_cleared_and_what_does_not(backend, stream):
    """A new description and a fresh attach start like a new Meteor; sdrpp_vfo_reset and sdrpp_vfo_replace with keep & 2 leave the demodulator alone; a replace
    without the bit leaves the new handle without one.  sdrpp_vfo_qpsk_reset is Meteor::reset(): it clears the filter line, the gain, the loop and MM's walk,
    and leaves lastI and MM's T - 1 delay samples (the fixture's `reset` case holds it to the compiled reference; here: it differs from a fresh attach in the
    first symbols, which read MM's delay samples, equals it in nothing but those once they are gone — and with the delay samples made equal, it IS a fresh one)."""
    from sdrplusplus_amd import radio

    blocks = pushes_of(stream[:2000], 500)
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    rd, rk = meteor()
    rd2, rk2 = meteor(agc_rate=0.05)

    def run(action, blocks=blocks, desc=None):
        ctx = make_ctx()
        vid = add_transparent(ctx, desc=desc)
        out = []
        for i, blk in enumerate(blocks):
            if i == 2:
                vid = action(ctx, vid) or vid
            ctx.push(blk)
            out.append(ctx.vfo_qpsk_read(vid))
        return ctx, vid, out

    c0, _, plain = run(lambda c, v: None)
    ctx = make_ctx()
    vid = add_transparent(ctx)
    fresh = run_cut(ctx, [vid], np.concatenate(blocks[2:]), [500])[vid]
    ctx.close()

    def reattach(c, v):
        c.vfo_set_qpsk(v, None)
        c.vfo_set_qpsk(v, rd, True, rk)

    def other_then_back(c, v):
        c.vfo_set_qpsk(v, rd2, True, rk2)
        assert c.qpsk_bank_count() == 1  # (the tables are the same: the AGC's rate is not part of them)
        c.vfo_set_qpsk(v, rd, True, rk)

    c1, _, re = run(reattach)
    c2, _, ob = run(other_then_back)
    c3, _, vr = run(lambda c, v: c.vfo_reset(v))
    c4, v4, mv = run(lambda c, v: c.vfo_replace(v, d, 3, keep))
    c5, _, rs = run(lambda c, v: c.vfo_qpsk_reset(v))
    for i in range(2):
        assert same(re[2 + i], fresh[i]) and same(ob[2 + i], fresh[i]), i
    assert not same(plain[2], fresh[0])
    for i in range(4):
        assert same(vr[i], plain[i]) and same(mv[i], plain[i]), i
    # reset(): MM's 7 delay samples are the old stream's, so the first symbols differ from a fresh attach's; the counts are a fresh attach's (offset starts at 0)
    assert [len(r[0]) for r in rs[2:]] == [len(f[0]) for f in fresh] and not same(rs[2], fresh[0])
    assert not bits_equal(rs[2][0][:3], fresh[0][0][:3])
    # ... and where the two blocks in front of the reset are silence (delay samples and lastI zero, as a new object's), reset() equals a fresh attach bit for bit
    quiet = [np.zeros(500, np.complex64)] * 2 + blocks[2:]
    c6, _, rq = run(lambda c, v: c.vfo_qpsk_reset(v), quiet)
    for i in range(2):
        assert same(rq[2 + i], fresh[i]), i
    # lastI stays: in OQPSK mode the first symbols' imaginary parts read it.  Silence cannot show it (lastI is then 0); a stream in front can
    c7, _, ro = run(lambda c, v: c.vfo_qpsk_reset(v), desc=meteor(oqpsk=True))
    ctx = make_ctx()
    vid = add_transparent(ctx, desc=meteor(oqpsk=True))
    fresh_o = run_cut(ctx, [vid], np.concatenate(blocks[2:]), [500])[vid]
    ctx.close()
    assert not bits_equal(ro[2][0][:4].imag.copy(), fresh_o[0][0][:4].imag.copy())
    c8 = make_ctx()
    v8 = c8.vfo_replace(add_transparent(c8), d, 1, keep)
    assert c8.L.sdrpp_vfo_qpsk_count(c8.h, v8) == INVALID and c8.qpsk_bank_count() == 0
    for c in (c0, c1, c2, c3, c4, c5, c6, c7, c8):
        c.close()


def test_argument_checks(backend):
    """Every error the header names, one per rejection, each with its reason in sdrpp_last_error."""
    from sdrplusplus_amd import capi, radio

    ctx = make_ctx()
    raw = add_transparent(ctx, demod=False)
    d, keep = radio.vfo_desc(50e3, 50e3, 12.5e3, 0.0, "NFM")
    nfm = ctx.vfo_add(d, keep)
    L, h = ctx.L, ctx.h
    good, gkeep = meteor()

    def code(vid=raw, loop=None, tap_values=None, **changes):
        s, k = meteor()
        for name, value in changes.items():
            setattr(s, name, value)
        for name, value in (loop or {}).items():
            setattr(s.loop, name, value)
        if tap_values is not None:
            k[0][:len(tap_values)] = tap_values
        rc = L.sdrpp_vfo_set_qpsk(h, vid, C.byref(s), 1)
        if rc:
            assert len(L.sdrpp_last_error(h)) > 10
        return rc

    assert code() == 0
    assert code(nfm) == UNSUPPORTED                       # only RAW VFOs
    assert L.sdrpp_vfo_set_qpsk(h, 9999, C.byref(good), 1) == NOT_FOUND
    assert L.sdrpp_vfo_set_qpsk(None, raw, C.byref(good), 1) == INVALID
    for bad in (float("nan"), float("inf")):
        for field in ("agc_set_point", "agc_max_gain", "agc_rate", "agc_init_gain", "omega", "mu_gain", "omega_gain", "min_omega", "max_omega", "soft_scale"):
            assert code(**{field: bad}) == INVALID, (field, bad)
        for field in ("alpha", "beta", "init_phase", "init_freq", "min_freq", "max_freq"):
            assert code(loop={field: bad}) == INVALID, (field, bad)
        assert code(tap_values=[bad]) == INVALID
    assert code(n_taps=0) == INVALID and code(n_taps=257) == INVALID and code(taps=capi.c_float_p()) == INVALID
    assert code(interp_ntaps=0) == INVALID and code(interp_ntaps=17) == INVALID and code(interp_bank=capi.c_float_p()) == INVALID
    assert code(interp_phases=0) == INVALID and code(interp_phases=1025) == INVALID
    assert code(min_omega=2.0, max_omega=2.0) == INVALID
    assert code(min_omega=1.0) == INVALID and code(min_omega=1.5, mu_gain=1.0) == INVALID  # min_omega - |mu_gain| >= 1
    assert code(max_omega=4096.0, mu_gain=1.0) == INVALID and code(max_omega=4095.0, min_omega=2.0, mu_gain=1.0) == 0
    assert code(loop={"min_freq": 1.0, "max_freq": 1.0}) == INVALID
    # the bounded-loop rule: max(|min|, |max|) + |alpha| <= 2 pi, |initial phase| <= pi
    assert code(loop={"min_freq": -6.0, "max_freq": 6.0, "alpha": 0.2}) == 0
    assert code(loop={"min_freq": -6.0, "max_freq": 6.0, "alpha": 0.3}) == INVALID
    assert code(loop={"min_freq": -6.3, "max_freq": 1.0, "alpha": 0.0}) == INVALID
    assert code(loop={"alpha": -5.0}) == INVALID
    assert code(loop={"init_phase": 3.2}) == INVALID and code(loop={"init_phase": -3.0}) == 0
    assert L.sdrpp_vfo_set_qpsk(h, raw, None, 0) == 0  # detach
    assert L.sdrpp_vfo_qpsk_count(h, raw) == INVALID and L.sdrpp_vfo_qpsk_read(h, raw, None, None, 0) == INVALID
    assert L.sdrpp_vfo_qpsk_device_buffers(h, raw, None, None, None) == INVALID and L.sdrpp_vfo_qpsk_reset(h, raw) == INVALID
    assert L.sdrpp_vfo_qpsk_set_mode(h, raw, 0, 1) == INVALID
    assert L.sdrpp_vfo_qpsk_count(h, 9999) == NOT_FOUND
    assert L.sdrpp_vfo_set_qpsk(h, raw, C.byref(good), 0) == 0
    assert L.sdrpp_vfo_qpsk_count(h, raw) == 0        # attached, switched off
    assert L.sdrpp_vfo_qpsk_read(h, raw, None, None, -1) == INVALID
    assert L.sdrpp_pipeline_set_qpsk_results(h, 1, 0) == INVALID  # outside pipelined mode
    assert L.sdrpp_set_pipelined(h, 1, 256) == INVALID and L.sdrpp_set_pipelined(h, 0, 0) == 0  # (the flag has its own call)
    assert L.sdrpp_result_qpsk(h, 1, raw, None, None, None) == INVALID  # nothing held
    assert L.sdrpp_qpsk_bank_count(None) == INVALID
    ctx.close()


def test_results_of_tickets_without_the_demodulator_or_the_flag(backend, stream):
    """Pipelined: a ticket pushed without flag 256, a VFO without the demodulator and one whose demodulator is switched off give SDRPP_ERR_NOT_FOUND; a released
    ticket SDRPP_ERR_INVALID; device buffers name the last ordinary push."""
    ctx = make_ctx()
    a = add_transparent(ctx)
    ctx.push(stream[:1000])
    want = ctx.vfo_qpsk_read(a)
    soft, packed, n = C.c_void_p(), C.c_void_p(), C.c_int()
    assert ctx.L.sdrpp_vfo_qpsk_device_buffers(ctx.h, a, C.byref(soft), C.byref(packed), C.byref(n)) == 0 and n.value == len(want[0]) > 400 and soft.value and packed.value
    ctx.close()
    ctx = make_ctx()
    a, off, none = add_transparent(ctx), add_transparent(ctx, enabled=False), add_transparent(ctx, demod=False)
    ctx.set_pipelined(True, 1)
    ctx.push(stream[:1000])
    ctx.pipeline_flush()
    assert ctx.L.sdrpp_pipeline_set_qpsk_results(ctx.h, 1, 1) == 0
    ctx.push(stream[1000:2000])
    ctx.result_wait(1)
    assert ctx.L.sdrpp_result_qpsk(ctx.h, 1, a, None, None, None) == NOT_FOUND
    ctx.result_release(1)
    ctx.result_wait(2)
    assert len(ctx.result_qpsk(2, a)[0]) > 400
    assert ctx.L.sdrpp_result_qpsk(ctx.h, 2, off, None, None, None) == NOT_FOUND
    assert ctx.L.sdrpp_result_qpsk(ctx.h, 2, none, None, None, None) == NOT_FOUND
    ctx.result_release(2)
    assert ctx.L.sdrpp_result_qpsk(ctx.h, 2, a, None, None, None) == INVALID
    ctx.set_pipelined(False)
    ctx.close()


def test_every_other_output_of_a_mixed_bank_is_unchanged(backend):
    """A bank of a WFM VFO with RDS branch and RDS demodulator, an NFM VFO, a RAW VFO with the pager's symbol branch and a RAW VFO for this demodulator, ordinary
    and pipelined in launch groups: with the QPSK demodulator attached (on, and switched off) audio, RDS samples, RDS bits, symbol branch outputs and both RAW
    VFOs' IF are what they are without it, bit for bit."""
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
        rd0, rk0 = radio.rds_demod_desc(5000.0, 0)
        ctx.vfo_set_rds_demod(w, rd0, True, rk0)
        d, keep = radio.vfo_desc(sr, 50e3, 12.5e3, 40e3, "NFM")
        nfm = ctx.vfo_add(d, keep)
        d, keep = radio.vfo_desc(sr, 25e3, 12.5e3, -60e3, "RAW")
        raw = ctx.vfo_add(d, keep)
        sd, sk = radio.pager_desc(25e3, 2400.0)
        ctx.vfo_set_symbols(raw, sd, True, sk)
        d, keep = radio.vfo_desc(sr, 125e3, 125e3, 200e3, "RAW")
        met = ctx.vfo_add(d, keep)
        if demod is not None:
            md, mk = meteor()  # (the 150 kS/s description on a 125 kS/s channel: to the block the rate is only a number)
            ctx.vfo_set_qpsk(met, md, demod, mk)
        out = []
        if pipelined:
            ctx.set_pipelined(True, 1 | capi.RESULT_RDS | capi.RESULT_SYM | capi.RESULT_RDS_BITS | (capi.RESULT_QPSK if demod else 0))
            ctx.set_pipeline_group(2)
            for p in pushes:
                ctx.push(p)
            for i in range(len(pushes)):
                res = ctx.result_wait(i + 1)
                out.append([res["vfo"][w], res["vfo"][nfm], res["vfo"][raw], res["vfo"][met], ctx.result_rds(i + 1, w), *ctx.result_sym(i + 1, raw), *ctx.result_rds_bits(i + 1, w)])
                if demod:
                    assert len(ctx.result_qpsk(i + 1, met)[1]) in range(2395, 2406)
                ctx.result_release(i + 1)
            assert ctx.pipeline_group_stats()["multi_groups"] >= 1  # the pushes did go out as a group of 2
            ctx.set_pipelined(False)
        else:
            for p in pushes:
                ctx.push(p)
                out.append([ctx.vfo_read(w), ctx.vfo_read(nfm), ctx.vfo_read(raw), ctx.vfo_read(met), ctx.vfo_rds_read(w), *ctx.vfo_sym_read(raw), *ctx.vfo_rds_demod_read(w)])
                if demod:
                    assert len(ctx.vfo_qpsk_read(met)[0]) in range(2395, 2406)
        ctx.close()
        return out

    for pipelined in (False, True):
        base = run(None, pipelined)
        for demod in (True, False):
            got = run(demod, pipelined)
            for i, (g, b) in enumerate(zip(got, base)):
                for k, (p, q) in enumerate(zip(g, b)):
                    assert bits_equal(np.asarray(p), np.asarray(q)), (pipelined, demod, i, k)


# ---- 5. banks: the workgroup edges of four jobs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 4, 5, 9])
def test_banks_with_two_descriptions(backend, stream, nv):
    """nv transparent channels fed the same samples, two descriptions alternating (the module's, and one with 65 taps and another AGC rate): every channel
    equals the channel alone, bit for bit, in one push and in pushes of 130; the context holds two table pairs (one for nv = 1)."""
    x = stream[:1300]

    def desc(k):
        return meteor(rrc_taps=65, agc_rate=0.2) if k % 2 else meteor()

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
        assert ctx.qpsk_bank_count() == min(nv, 2)
        got = run_cut(ctx, vids, x, sizes)
        ctx.close()
        for k, v in enumerate(vids):
            assert same(cat(got[v]), alone[k % 2]), (nv, sizes, k)


# ---- 6. samples that are not numbers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["emu"], indirect=True)
def test_nan_and_inf_samples_end_inside_the_arrays(backend):
    """Emulator only — where a mistake costs a CPU process, not a GPU: a push containing NaN and +-inf samples ends, in both error modes, its count is within the
    outputs' capacity ceil(n / floor(min_omega - |mu gain|)) + 1 (Vfo::Qpsk::cap_of; floor(2.0625 - 0.01) = 2 for the module's description), every int8 pair is
    the sink's rule of its soft value (a NaN gives 0), and a fresh attach behind it gives the fixture's result bit for bit."""
    z = np.load(GOLDEN)
    x = case_input(z, "cuts")[:1250].copy()
    bad = x.copy()
    bad[100] = np.complex64(complex(float("nan"), 0.0))
    bad[300] = np.complex64(complex(float("inf"), 1.0))
    bad[500] = np.complex64(complex(0.0, float("-inf")))
    rd, rk = meteor()
    min_step = int(np.floor(np.float32(rd.min_omega) - np.float32(abs(rd.mu_gain))))
    assert min_step == 2
    ctx = make_ctx()
    vid = add_transparent(ctx)
    for broken in (False, True):
        ctx.vfo_qpsk_set_mode(vid, broken, False)
        for blk in (bad, x, bad[:64], bad[90:110]):
            ctx.push(blk)
            n = ctx.vfo_qpsk_count(vid)
            assert 0 <= n <= (len(blk) + min_step - 1) // min_step + 1, n
            soft, packed = ctx.vfo_qpsk_read(vid)
            assert np.array_equal(packed, sink(soft))
    assert np.isnan(soft.view(np.float32)).any() and (packed[np.isnan(soft.view(np.float32).reshape(-1, 2))] == 0).all()
    ctx.vfo_set_qpsk(vid, None)
    ctx.vfo_set_qpsk(vid, rd, True, rk)
    got, pos = [], 0
    for s in z["cuts_cut"][:6]:
        ctx.push(case_input(z, "cuts")[pos:pos + s])
        got.append(ctx.vfo_qpsk_read(vid))
        pos += int(s)
    ctx.close()
    m = int(z["cuts_counts"][:6].sum())
    assert [len(g[0]) for g in got] == list(z["cuts_counts"][:6])
    soft, packed = cat(got)
    assert bits_equal(soft, z["cuts_soft"][:m]) and np.array_equal(packed, z["cuts_i8"][:m])
