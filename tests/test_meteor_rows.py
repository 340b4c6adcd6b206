"""The Meteor QPSK demodulator per symbol, bit for bit, at every edge of its two kernels (vfo_qpsk_kernels.h) — in the manner of tests/test_rds_demod_rows.py.

cosf / sinf / atan2f differ between libraries, so the EXACT rows freeze the Costas loop: alpha = beta = 0, phase and frequency 0.  The phasor is then exactly
(1, -0) everywhere and every remaining operation — the real-tap complex FIR in the generic VOLK order, the AGC, the OQPSK exchange, MM's complex symbol step, the
int8 conversion — is a single IEEE float32 operation, so device, emulator and the float32 restatement (tests/qpsk_ref.py) must agree in every soft word
(compared as uint32), every int8 and every per-push count.  Taps and banks are random with all entries distinct.  Each row asserts its own edge from the
kernels' constants on the CPU before any device output is looked at.  The LIVE rows run the module's loop, in both error modes, against the restatement under the
bar of tests/test_meteor.py: max(1e-5 x RMS, 4 x spread), the spread taken from the restatement by the fixture recorder's recipe (every input component times
1 +- 2^-24; 4 runs); on the emulator, whose library the restatement's is, they are bit-equal.  test_restatement_is_the_reference pins the restatement to the
reference's recorded outputs on the CPU."""
import os

import numpy as np
import pytest

import qpsk_ref
from qpsk_ref import CHUNK, MAX_INTERP_TAPS, MAX_PHASES, MAX_TAPS, SEG, TILE

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "meteor_ref.npz")
RATE = 150000.0


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def u32(a):
    return np.ascontiguousarray(np.asarray(a, np.complex64)).view(np.uint32)


def comps(a):
    return np.ascontiguousarray(np.asarray(a, np.complex64)).view(np.float32).reshape(-1, 2).astype(np.float64)


def case_input(z, name):
    key = name + "_x" if name + "_x" in z.files else str(z[name + "_xof"]) + "_x"
    return (z[key].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)[:int(z[name + "_cut"].sum())]


# ---- the restatement is the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["offset", "weak", "oqpsk", "broken", "cuts", "reset", "reset_oqpsk", "mode"])
def test_restatement_is_the_reference(name):
    """CPU only.  The float32 restatement over the first 3000 samples of the fixture's input (all of it where the case starts over in mid-stream) in the fixture's
    cuts, reset() and setOQPSK(true) where the fixture calls them: counts and int8 pairs exactly the recorded ones, soft components inside the fixture's bar (with
    the C library the reference was recorded with they are the recorded bits: the printed share)."""
    from sdrplusplus_amd import radio

    z = np.load(GOLDEN)
    x = case_input(z, name)
    ops = {int(b): int(o) for b, o in z[name + "_ops"]}
    if not ops:
        x = x[:3000]
    broken, oqpsk = (int(v) for v in z[name + "_mode"])
    rd, rk = radio.meteor_desc(broken=broken, oqpsk=oqpsk)
    ref = qpsk_ref.MeteorRef(qpsk_ref.params_of(rd, *rk))
    soft, i8, counts, pos = [], [], [], 0
    for b, s in enumerate(z[name + "_cut"]):
        if pos + s > len(x):  # (whole blocks only)
            break
        if ops.get(b) == 2:
            ref.reset()
        if ops.get(b) == 3:
            ref.oqpsk = True
        so, pk = ref.process(x[pos:pos + s])
        soft.append(so)
        i8.append(pk)
        counts.append(len(so))
        pos += int(s)
    soft, i8 = np.concatenate(soft), np.concatenate(i8)
    m = len(soft)
    assert counts == list(z[name + "_counts"][:len(counts)])
    want = z[name + "_soft"][:m]
    bar = np.maximum(1e-5 * rms(comps(z[name + "_soft"])), 4.0 * z[name + "_dev_max"][:m].astype(np.float64))
    err = np.abs(comps(soft) - comps(want))
    print("%s: %d symbols, %.1f %% bit-equal, largest |error| / bar %.3g" % (name, m, 100.0 * float((u32(soft) == u32(want)).mean()), float((err / bar).max())))
    assert (err <= bar).all()
    assert np.array_equal(i8, z[name + "_i8"][:m])


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
def distinct(r, n, lo=0.1, hi=1.0):
    """n random values of magnitude lo .. hi with random signs, all different"""
    while True:
        v = (r.uniform(lo, hi, n) * np.where(r.integers(0, 2, n) == 1, 1.0, -1.0)).astype(np.float32)
        if len(np.unique(v)) == n:
            return v


def make_params(K=33, T=8, P=128, omega=2.08, mu=0.01, og=1e-6, rel=0.01, mn=None, mx=None, set_point=1.0, max_gain=10e6, agc_rate=0.1, oqpsk=0, scale=84.0, seed=0):
    r = np.random.default_rng(2000 + seed)
    taps = distinct(r, K) / np.float32(np.sqrt(K))
    bank = (distinct(r, P * T) / np.float32(np.sqrt(T))).reshape(P, T)
    f = np.float32
    return dict(agc=[f(set_point), f(max_gain), f(agc_rate), f(1.0)], loop=[0.0, 0.0, 0.0, 0.0, -1.0, 1.0], taps=taps, broken=0, oqpsk=oqpsk, omega=f(omega), mu_gain=f(mu),
                omega_gain=f(og), min_omega=f(mn if mn is not None else omega * (1 - rel)), max_omega=f(mx if mx is not None else omega * (1 + rel)), bank=bank, soft_scale=f(scale))


def live_params(broken=0, oqpsk=0, K=33):
    from sdrplusplus_amd import radio

    rd, rk = radio.meteor_desc(broken=broken, oqpsk=oqpsk, rrc_taps=K)
    return qpsk_ref.params_of(rd, *rk)


def desc_of(p):
    from sdrplusplus_amd import capi

    d = capi.QpskDesc()
    d.agc_set_point, d.agc_max_gain, d.agc_rate, d.agc_init_gain = (float(v) for v in p["agc"])
    l = d.loop
    l.alpha, l.beta, l.init_phase, l.init_freq, l.min_freq, l.max_freq = (float(v) for v in p["loop"])
    taps = np.ascontiguousarray(p["taps"], np.float32)
    bank = np.ascontiguousarray(p["bank"], np.float32)
    d.n_taps = len(taps)
    d.taps = taps.ctypes.data_as(capi.c_float_p)
    d.broken, d.oqpsk = int(p["broken"]), int(p["oqpsk"])
    d.omega, d.mu_gain, d.omega_gain, d.min_omega, d.max_omega = (float(p[k]) for k in ("omega", "mu_gain", "omega_gain", "min_omega", "max_omega"))
    d.interp_phases, d.interp_ntaps = bank.shape
    d.interp_bank = bank.ctypes.data_as(capi.c_float_p)
    d.soft_scale = float(p["soft_scale"])
    return d, [taps, bank]


def noise(n, seed, amp=0.3):
    r = np.random.default_rng(seed)
    return (amp * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64)


def cuts_of(n, sizes):
    out, pos, k = [], 0, 0
    while pos < n:
        s = min(sizes[k % len(sizes)], n - pos)
        out.append(s)
        pos += s
        k += 1
    return out


class Row:
    def __init__(self, id, params, x, cuts, edge, live=False):
        self.id, self.params, self.x, self.cuts, self.edge, self.live = id, params, x, cuts_of(len(x), cuts), edge, live


def ends(row):
    return np.cumsum(row.cuts)


def K_(K):
    def edge(row, ref):
        assert len(row.params["taps"]) == K and 1 <= K <= MAX_TAPS and row.cuts[0] > TILE + 1 and len(row.cuts) >= 2  # more than one tile, and the line handed over
    return Row("K%d" % K, make_params(K=K, seed=K), noise(520 if K < 100 else 700, K), [260 if K < 100 else 350], edge)


def T_(T):
    def edge(row, ref):
        assert row.params["bank"].shape[1] == T and 1 <= T <= MAX_INTERP_TAPS and len(row.x) > 2 * CHUNK  # MM's line carried over chunk and push ends
    return Row("T%d" % T, make_params(K=5, T=T, seed=20 + T), noise(400, 20 + T), [150], edge)


def P_(P):
    def edge(row, ref):
        assert row.params["bank"].shape[0] == P and 1 <= P <= MAX_PHASES
        assert len(np.unique(row.params["bank"])) == row.params["bank"].size  # (all rows differ: the soft values themselves say which row was read)
    return Row("P%d" % P, make_params(K=5, T=8 if P < 1024 else 4, P=P, mu=0.3, og=0.01, rel=0.05, seed=40 + P), noise(500, 40 + P), [500], edge)


def block_(B):
    def edge(row, ref):
        assert row.cuts[0] == B and len(row.cuts) >= 3
    return Row("block%d" % B, make_params(K=9, seed=60 + B), noise(max(3 * B + 5, 40), 60 + B), [B], edge)


def seg_(n, name):
    def edge(row, ref):
        assert row.cuts[0] == n and n in (SEG - 1, SEG, SEG + 1, 2 * SEG + 1) and len(row.cuts) == 2  # a second push reads the line the last segment left
    return Row("seg_" + name, make_params(K=40, seed=80 + n % 7), noise(n + 100, 80 + n), [n], edge)


def one_sample_pushes():
    def edge(row, ref):
        assert len(row.cuts) == 200 and set(row.cuts) == {1} and len(row.params["taps"]) - 1 > 1 and row.params["bank"].shape[1] - 1 > 1  # both lines longer than the block
    return Row("one_sample_pushes", make_params(K=33, T=16, seed=90), noise(200, 90), [1], edge)


def max_gain_hit():
    def edge(row, ref):
        assert ref.hits["max_gain"] > 50
    return Row("max_gain", make_params(K=3, max_gain=3.0, seed=91), noise(300, 91, amp=0.01), [300], edge)


def error_clamps():
    def edge(row, ref):
        assert ref.hits["err_hi"] > 3 and ref.hits["err_lo"] > 3
    return Row("mm_error_clamps", make_params(K=3, set_point=3.0, agc_rate=0.5, mu=0.2, og=1e-3, rel=0.05, seed=92), noise(400, 92, amp=1.0), [170], edge)


def omega_limits():
    def edge(row, ref):
        assert ref.hits["omega_hi"] > 3 and ref.hits["omega_lo"] > 3
    return Row("omega_limits", make_params(K=3, set_point=3.0, agc_rate=0.5, mu=0.1, og=0.05, rel=0.02, seed=93), noise(500, 93, amp=1.0), [500], edge)


def omega_(om, n):
    def edge(row, ref):
        assert float(row.params["min_omega"]) - float(row.params["mu_gain"]) >= 1.0
        assert (om > CHUNK) == bool(np.diff(ref.starts).max() > CHUNK)  # omega 70: chunks without a symbol
    return Row("omega%g" % om, make_params(K=5, omega=om, mu=0.05, og=1e-4, seed=94), noise(n, 94), [n // 2 + 3], edge)


def starts_on_edges():
    """omega exactly 2, gains 0: a symbol at every even sample — on every chunk edge, every segment edge and (pushes of 64 and 512) every push end"""
    def edge(row, ref):
        s = np.asarray(ref.starts)
        assert np.array_equal(s, np.arange(0, len(row.x), 2))
        assert set(ends(row)[:-1]) <= set(s) and SEG in s and CHUNK in s
    return Row("starts_on_edges", make_params(K=7, omega=2.0, mu=0.0, og=0.0, mn=1.5, mx=2.5, seed=95), noise(2 * SEG + 64, 95), [64, SEG, 64, SEG - 64], edge)


def oqpsk_chunk_edge():
    def edge(row, ref):
        assert row.params["oqpsk"] == 1 and len(row.x) > 2 * CHUNK and row.cuts[0] == CHUNK + 1  # the partner of sample 64 is sample 63: another chunk, and of 65 it is 64: another push
    return Row("oqpsk_chunk_edge", make_params(K=4, oqpsk=1, seed=96), noise(300, 96), [CHUNK + 1, 200], edge)


def int8_edges():
    """a scale at which both clamps are hit and values truncate towards zero from each side"""
    def edge(row, ref):
        so, pk = qpsk_ref.MeteorRef(row.params).process(row.x)
        v = comps(so) * float(row.params["soft_scale"])
        assert (pk == 127).sum() > 5 and (pk == -127).sum() > 5 and (pk == -128).sum() == 0
        inside = np.abs(v) < 127
        assert ((v > 0.5) & inside & (v - np.floor(v) > 0.5)).sum() > 5 and ((v < -0.5) & inside & (np.ceil(v) - v > 0.5)).sum() > 5  # rounding would give the neighbour
        assert np.array_equal(pk[inside], np.trunc(v[inside]).astype(np.int8))
    return Row("int8_edges", make_params(K=3, scale=150.0, seed=97), noise(400, 97), [400], edge)


def counts_odd_even():
    def edge(row, ref):
        st = np.asarray(ref.starts)
        per = [int(((st >= lo) & (st < hi)).sum()) for lo, hi in zip(np.r_[0, ends(row)[:-1]], ends(row))]
        assert any(c % 2 for c in per) and any(c % 2 == 0 and c > 0 for c in per) and 0 in per  # odd, even and empty pushes: the packed stores' tail
    return Row("counts_odd_even", make_params(K=3, omega=3.0, mu=0.0, og=0.0, mn=2.5, mx=3.5, seed=98), noise(60, 98), [3, 6, 1, 1, 1, 9, 12], edge)


def live_(name, broken, oqpsk, K, cuts, n=900):
    def edge(row, ref):
        assert row.params["loop"][0] != 0 and row.params["broken"] == broken and len(row.params["taps"]) == K
    z = np.load(GOLDEN)
    return Row("live_" + name, live_params(broken, oqpsk, K), case_input(z, "offset")[:n], cuts, edge, live=True)


ROWS = ([K_(K) for K in (1, 2, 33, 63, 64, 65, 256)] + [T_(T) for T in (1, 7, 8, 9, 16)] + [P_(P) for P in (1, 127, 128, 1024)] +
        [block_(B) for B in (1, 2, 63, 64, 65, 127, 128, 129)] + [seg_(SEG - 1, "minus1"), seg_(SEG, "exact"), seg_(SEG + 1, "plus1"), seg_(2 * SEG + 1, "two_plus1")] +
        [one_sample_pushes(), max_gain_hit(), error_clamps(), omega_limits(), omega_(1.2, 300), omega_(70.0, 900), starts_on_edges(), oqpsk_chunk_edge(), int8_edges(),
         counts_odd_even()])
LIVE = [live_("blocks65", 0, 0, 33, [65]), live_("broken_blocks65", 1, 0, 33, [65]), live_("one_sample_pushes", 0, 1, 33, [1], n=260), live_("broken_one_sample", 1, 0, 33, [1], n=260),
        live_("K32", 0, 0, 32, [450]), live_("K64", 0, 0, 64, [450]), live_("K65", 1, 0, 65, [450]), live_("K256", 0, 0, 256, [450])]


def run_ref(row):
    ref = qpsk_ref.MeteorRef(row.params)
    out, pos = [], 0
    for s in row.cuts:
        out.append(ref.process(row.x[pos:pos + s]))
        pos += s
    return ref, out


def run_device(row, group=None):
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=4096)
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    vid = ctx.vfo_add(d, keep)
    rd, rk = desc_of(row.params)
    ctx.vfo_set_qpsk(vid, rd, True, rk)
    out, pos = [], 0
    for s in row.cuts:
        ctx.push(row.x[pos:pos + s])
        out.append(ctx.vfo_qpsk_read(vid))
        pos += s
    ctx.close()
    return out


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_exact_row(backend, row):
    """Loop frozen: device (or emulator) and restatement agree in every soft word as uint32, every int8 and every per-push count."""
    ref, want = run_ref(row)
    row.edge(row, ref)
    assert sum(len(w[0]) for w in want) >= 5
    got = run_device(row)
    assert [len(g[0]) for g in got] == [len(w[0]) for w in want]
    gs, ws = np.concatenate([g[0] for g in got]), np.concatenate([w[0] for w in want])
    assert np.array_equal(u32(gs), u32(ws)), int((u32(gs) != u32(ws)).sum())
    assert np.array_equal(np.concatenate([g[1] for g in got]), np.concatenate([w[1] for w in want]))


@pytest.mark.parametrize("row", LIVE, ids=[r.id for r in LIVE])
def test_live_row(backend, row):
    """The module's loop on, both error modes: counts equal, soft components under max(1e-5 x RMS, 4 x the restatement's own spread); bit-equal on the emulator."""
    ref, want = run_ref(row)
    row.edge(row, ref)
    ws = np.concatenate([w[0] for w in want])
    r = np.random.default_rng(7)
    spread = np.zeros((len(ws), 2))
    for _ in range(4):
        sgn = np.where(r.integers(0, 2, (len(row.x), 2)) == 1, 1.0, -1.0)
        xk = (row.x.view(np.float32).reshape(-1, 2).astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32).view(np.complex64).reshape(-1)
        _, alt = run_ref(Row(row.id, row.params, xk, row.cuts, row.edge))
        a = np.concatenate([w[0] for w in alt])
        assert len(a) == len(ws)
        spread = np.maximum(spread, np.abs(comps(a) - comps(ws)))
    got = run_device(row)
    assert [len(g[0]) for g in got] == [len(w[0]) for w in want]
    gs = np.concatenate([g[0] for g in got])
    bar = np.maximum(1e-5 * rms(comps(ws)), 4.0 * spread)
    err = np.abs(comps(gs) - comps(ws))
    print("%s [%s]: %d symbols, largest |error| / bar %.3g" % (row.id, backend, len(ws), float((err / bar).max())))
    assert (err <= bar).all(), float((err / bar).max())
    assert np.array_equal(np.concatenate([g[1] for g in got]), qpsk_ref.sink(gs, row.params["soft_scale"]))
    if backend == "emu":
        assert np.array_equal(u32(gs), u32(ws))
