"""The RDS demodulator per symbol, bit for bit, at every edge of its kernel (vfo_rdsd_kernels.h) — in the manner of tests/test_pager_rows.py.

cosf / sinf differ between libraries, so the EXACT rows freeze both Costas loops: alpha = beta = 0, phase and frequency 0.  The phasor is then exactly (1, -0)
everywhere and every remaining operation — AGC, the complex FIR in the generic VOLK order, MM's symbol step, slicer, differential decoder — is a single IEEE
float32 operation, so device, emulator and the float32 restatement (tests/rdsd_ref.py) must agree in every soft value (compared as uint32), bit and per-push
count.  Taps and banks are random with all entries distinct.  Each row asserts its own edge from the kernel's constants on the CPU before any device output
is looked at.  The LIVE rows run the same kind of edges with the radio's real loop coefficients against the restatement under the bar of tests/test_rds_demod.py:
max(1e-5 x RMS, 4 x spread), the spread taken from the restatement by the fixture recorder's recipe (8 runs, every input component times 1 +- 2^-24).
test_restatement_is_the_reference pins the restatement to the reference's recorded outputs on the CPU."""
import os

import numpy as np
import pytest

import rdsd_ref
from rdsd_ref import CHUNK, MAX_INTERP_TAPS, MAX_PHASES, MAX_TAPS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rds_demod_ref.npz")
RATE = 5000.0


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the restatement is the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["offset", "weak", "cuts", "fresh", "reset"])
def test_restatement_is_the_reference(name):
    """CPU only.  The float32 restatement over the fixture's input in the fixture's cuts, a new object where the fixture starts one and reset() where it calls it:
    counts and bits exactly the recorded ones, soft values inside the fixture's bar (with the C library the reference was recorded with they are the recorded
    bits: the printed share)."""
    from sdrplusplus_amd import radio

    z = np.load(GOLDEN)
    x = (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
    if name in ("offset", "weak"):
        x = x[:7500]  # six of the fixture's blocks
    rd, rk = radio.rds_demod_desc(RATE, 1)
    p = rdsd_ref.params_of(rd, *rk)
    ref = rdsd_ref.RdsDemodRef(p)
    soft, bits, counts, pos = [], [], [], 0
    for b, s in enumerate(z[name + "_cut"]):
        if pos >= len(x):
            break
        if b in z[name + "_fresh"]:
            ref = rdsd_ref.RdsDemodRef(p)
        if b in z[name + "_reset"]:
            ref.reset()
        so, bi = ref.process(x[pos:pos + s])
        soft.append(so)
        bits.append(bi)
        counts.append(len(so))
        pos += int(s)
    soft, bits = np.concatenate(soft), np.concatenate(bits)
    m = len(soft)
    assert counts == list(z[name + "_counts"][:len(counts)])
    assert np.array_equal(bits, z[name + "_bits"][:m])
    want = z[name + "_soft"][:m]
    bar = np.maximum(1e-5 * rms(z[name + "_soft"]), 4.0 * z[name + "_dev_max"][:m].astype(np.float64))
    err = np.abs(soft.astype(np.float64) - want)
    print("%s: %d symbols, %.1f %% bit-equal, largest |error| / bar %.3g" % (name, m, 100.0 * float((u32(soft) == u32(want)).mean()), float((err / bar).max())))
    assert (err <= bar).all()


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
def distinct(r, n, lo=0.1, hi=1.0):
    """n random values of magnitude lo .. hi with random signs, all different"""
    while True:
        v = (r.uniform(lo, hi, n) * np.where(r.integers(0, 2, n) == 1, 1.0, -1.0)).astype(np.float32)
        if len(np.unique(v)) == n:
            return v


def make_params(K=190, T=8, P=128, omega=4.2, mu=0.01, og=1e-6, rel=0.01, mn=None, mx=None, set_point=1.0, max_gain=1e6, agc_rate=0.1, seed=0):
    r = np.random.default_rng(1000 + seed)
    v = distinct(r, 2 * K) / np.float32(np.sqrt(K))
    taps = (v[:K] + 1j * v[K:]).astype(np.complex64)
    bank = (distinct(r, P * T) / np.float32(np.sqrt(T))).reshape(P, T)
    f = np.float32
    l1 = l2 = [0.0, 0.0, 0.0, 0.0, -1.0, 1.0]  # both loops frozen
    return dict(agc=[f(set_point), f(max_gain), f(agc_rate), f(1.0)], loop1=l1, loop2=l2, taps=taps, omega=f(omega), mu_gain=f(mu), omega_gain=f(og),
                min_omega=f(mn if mn is not None else omega * (1 - rel)), max_omega=f(mx if mx is not None else omega * (1 + rel)), bank=bank)


def desc_of(p):
    from sdrplusplus_amd import capi

    d = capi.RdsdDesc()
    d.source = 1
    d.agc_set_point, d.agc_max_gain, d.agc_rate, d.agc_init_gain = (float(v) for v in p["agc"])
    for l, q in ((d.loop1, p["loop1"]), (d.loop2, p["loop2"])):
        l.alpha, l.beta, l.init_phase, l.init_freq, l.min_freq, l.max_freq = (float(v) for v in q)
    taps = np.ascontiguousarray(p["taps"], np.complex64)
    bank = np.ascontiguousarray(p["bank"], np.float32)
    d.n_taps = len(taps)
    d.taps = taps.view(np.float32).ctypes.data_as(capi.c_float_p)
    d.omega, d.mu_gain, d.omega_gain, d.min_omega, d.max_omega = (float(p[k]) for k in ("omega", "mu_gain", "omega_gain", "min_omega", "max_omega"))
    d.interp_phases, d.interp_ntaps = bank.shape
    d.interp_bank = bank.ctypes.data_as(capi.c_float_p)
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
        assert len(row.params["taps"]) == K and 1 <= K <= MAX_TAPS and len(row.x) > 2 * CHUNK + K  # the line is carried over more than one chunk
    return Row("K%d" % K, make_params(K=K, seed=K), noise(400 if K < 100 else 700, K), [400 if K < 100 else 350], edge)


def T_(T):
    def edge(row, ref):
        assert row.params["bank"].shape[1] == T and 1 <= T <= MAX_INTERP_TAPS
    return Row("T%d" % T, make_params(K=5, T=T, seed=20 + T), noise(400, 20 + T), [150], edge)


def P_(P):
    def edge(row, ref):
        assert row.params["bank"].shape[0] == P and 1 <= P <= MAX_PHASES
        assert len(np.unique(row.params["bank"])) == row.params["bank"].size  # (all rows differ: the soft values themselves say which row was read)
    return Row("P%d" % P, make_params(K=5, T=8 if P < 1024 else 4, P=P, mu=0.3, og=0.01, rel=0.05, seed=40 + P), noise(500, 40 + P), [500], edge)


def B_(size):
    def edge(row, ref):
        e = ends(row)
        assert all(c == size for c in row.cuts[:-1])
        if size < CHUNK:
            assert size < len(row.params["taps"]) - 1 or size >= 63  # (blocks of 1 and 2: the FIR's line and MM's line are longer than the block)
        assert (size % CHUNK == 0) == bool(all(v % CHUNK == 0 for v in e[:-1]))
    n = {1: 200, 2: 300}.get(size, 3 * size + 17)
    return Row("block%d" % size, make_params(K=190 if size <= 2 else 70, T=8, seed=60 + size), noise(n, 60 + size), [size], edge)


def hits_(id, want, **kw):
    def edge(row, ref):
        for k in want:
            assert ref.hits[k] > 0, (k, ref.hits)
    x_amp = kw.pop("amp", 0.3)
    return Row(id, make_params(K=9, seed=len(id), **kw), noise(600, 7 + len(id), x_amp), [257], edge)


def omega_(omega, mu, og, n, cut):
    def edge(row, ref):
        st = np.diff(np.asarray(ref.starts))
        if omega < 2:
            assert (st == 1).sum() > 50 and (st == 2).sum() > 3  # several symbols per sample of a chunk: one per sample, most of the time
        else:
            assert st.min() > CHUNK  # chunks without a symbol
            assert any(c == 0 for c in ref_counts(row, ref))
    return Row("omega%g" % omega, make_params(K=9, omega=omega, mu=mu, og=og, rel=0.02, seed=int(omega)), noise(n, int(omega) + 3), cut, edge)


def ref_counts(row, ref):
    e = np.concatenate([[0], ends(row)])
    s = np.asarray(ref.starts)
    return [int(((s >= e[i]) & (s < e[i + 1])).sum()) for i in range(len(row.cuts))]


def on_edges():
    """omega exactly 4 with both gains 0: a symbol starts every fourth sample — at 64, 128, ... (chunk edges) and at the push ends 100 and 200; the symbol that
    starts AT a push end belongs to the next push"""
    def edge(row, ref):
        s = np.asarray(ref.starts)
        assert np.array_equal(s, np.arange(0, len(row.x), 4))
        assert CHUNK in s and 2 * CHUNK in s and 100 in s and 200 in s
        assert ref_counts(row, ref) == [25, 25, 28]
    return Row("starts_on_edges", make_params(K=9, omega=4.0, mu=0.0, og=0.0, mn=3.5, mx=4.5, seed=99), noise(312, 99), [100, 100, 112], edge)


ROWS = ([K_(K) for K in (1, 2, 63, 64, 65, 190, MAX_TAPS)] + [T_(T) for T in (1, 7, 8, 9, 16)] + [P_(P) for P in (1, 127, 128, 1024)] +
        [B_(s) for s in (1, 2, 63, 64, 65, 127, 128, 129)] + [
    hits_("max_gain", ["max_gain"], max_gain=5.0, amp=1e-3),
    hits_("mm_clamps", ["err_hi", "err_lo", "omega_hi", "omega_lo"], omega=6.0, mu=0.5, og=0.5, rel=0.05, set_point=5.0),
    omega_(1.2, 0.05, 0.001, 300, [300]),
    omega_(70.0, 0.5, 0.01, 1500, [40, 30, 20, 700]),
    on_edges(),
])

_cache = {}


def restated(row):
    """the float32 restatement of a row in its own schedule -> (ref, [(soft, bits) per push]); computed once, then left alone"""
    if row.id not in _cache:
        ref = rdsd_ref.RdsDemodRef(row.params)
        parts, pos = [], 0
        for s in row.cuts:
            parts.append(ref.process(row.x[pos:pos + s]))
            pos += s
        _cache[row.id] = (ref, parts)
    return _cache[row.id]


def run_device(row):
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=4096)
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    vid = ctx.vfo_add(d, keep)
    rd, rk = desc_of(row.params)
    ctx.vfo_set_rds_demod(vid, rd, True, rk)
    out, pos = [], 0
    for s in row.cuts:
        ctx.push(row.x[pos:pos + s])
        out.append(ctx.vfo_rds_demod_read(vid))
        pos += s
    ctx.close()
    return out


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_rds_demod_symbol_by_symbol(backend, row):
    """Every exact row: the row's own edge on the CPU first, then per push counts, soft values as uint32 and bits against the float32 restatement."""
    ref, want = restated(row)
    assert all(v == 0 for v in row.params["loop1"][:4]) and all(v == 0 for v in row.params["loop2"][:4])
    assert ref.ph1 == 0 and ref.fr1 == 0 and ref.ph2 == 0 and ref.fr2 == 0
    assert sum(len(w[0]) for w in want) >= 3
    row.edge(row, ref)
    got = run_device(row)
    assert [len(g[0]) for g in got] == [len(w[0]) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(u32(g[0]), u32(w[0])), (row.id, i, int((u32(g[0]) != u32(w[0])).sum()), len(w[0]))
        assert np.array_equal(g[1], w[1]), (row.id, i)


# ---- live loops --------------------------------------------------------------------------------------------------------------------------------
def live_rows():
    rows = []
    for id, cut, n in (("live_block65", [65], 1500), ("live_ones", [1], 260), ("live_mixed", [1, 128, 63, 700, 2], 1500)):
        x, _ = rdsd_ref.rds_signal(n, seed=len(id), df=2.0, sigma=2e-3)
        rows.append(Row(id, None, x, cut, None, live={}))  # (the radio's own description: live_restated)
    # the K, T and phase edges of the exact rows with the loops alive: the radio's loops and AGC around a DESIGNED band-pass of K taps (its transition width chosen
    # for the tap count) or a designed interpolator of P x T
    for K, tw in ((63, 300.0), (64, 296.8), (65, 292.0), (MAX_TAPS, 74.2)):
        rows.append(Row("live_K%d" % K, None, rdsd_ref.rds_signal(900, seed=K, df=2.0, sigma=2e-3)[0], [333], None, live=dict(K=K, tw=tw)))
    for P, T in ((128, 7), (128, 9), (128, MAX_INTERP_TAPS), (127, 8), (MAX_PHASES, 8)):
        rows.append(Row("live_P%dxT%d" % (P, T), None, rdsd_ref.rds_signal(900, seed=P + T, df=2.0, sigma=2e-3)[0], [333], None, live=dict(P=P, T=T)))
    return rows


LIVE = live_rows()
_live_cache = {}


def live_restated(row):
    """-> (parts, per-symbol spread): nine restatement runs, which must agree in counts and bits"""
    if row.id in _live_cache:
        return _live_cache[row.id]
    from sdrplusplus_amd import capi, radio

    rd, rk = radio.rds_demod_desc(RATE, 1)
    row.params = rdsd_ref.params_of(rd, *rk)
    if "K" in row.live:
        row.params["taps"] = capi.design_band_pass_complex(0.0, 2375.0, row.live["tw"], RATE)
        assert len(row.params["taps"]) == row.live["K"]
    if "P" in row.live:
        row.params["bank"] = capi.design_mm_interp(row.live["P"], row.live["T"])

    def once(x):
        ref = rdsd_ref.RdsDemodRef(row.params)
        parts, pos = [], 0
        for s in row.cuts:
            parts.append(ref.process(x[pos:pos + s]))
            pos += s
        return parts

    parts = once(row.x)
    soft = np.concatenate([p[0] for p in parts]).astype(np.float64)
    bits = np.concatenate([p[1] for p in parts])
    r = np.random.default_rng(4242)
    xf = row.x.view(np.float32)
    dev = np.zeros(len(soft))
    for k in range(8):
        sgn = np.where(r.integers(0, 2, xf.shape) == 1, 1.0, -1.0)
        xk = (xf.astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32).view(np.complex64)
        pk = once(xk)
        assert [len(p[0]) for p in pk] == [len(p[0]) for p in parts] and np.array_equal(np.concatenate([p[1] for p in pk]), bits), "another seed"
        dev = np.maximum(dev, np.abs(np.concatenate([p[0] for p in pk]).astype(np.float64) - soft))
    _live_cache[row.id] = (parts, dev)
    return _live_cache[row.id]


@pytest.mark.parametrize("row", LIVE, ids=[r.id for r in LIVE])
def test_rds_demod_live_rows(backend, row):
    """The same edges with the loops alive: blocks of 65, one-sample pushes (lines longer than the block) and a mix of chunk-edge cuts, the radio's own description;
    counts and bits equal, soft values under the bar."""
    want, spread = live_restated(row)
    got = run_device(row)
    assert [len(g[0]) for g in got] == [len(w[0]) for w in want]
    gs, ws = np.concatenate([g[0] for g in got]).astype(np.float64), np.concatenate([w[0] for w in want]).astype(np.float64)
    assert np.array_equal(np.concatenate([g[1] for g in got]), np.concatenate([w[1] for w in want]))
    floor = 1e-5 * rms(ws)
    bar = np.maximum(floor, 4.0 * spread)
    err = np.abs(gs - ws)
    print("%s [%s]: %d symbols, largest |error| / bar %.3g, bar at its floor for %.1f %% of the symbols" % (row.id, backend, len(ws), float((err / bar).max()), 100.0 * float((bar == floor).mean())))
    assert float((bar == floor).mean()) >= 0.9
    assert (err <= bar).all()


def header_constants():
    """the #defines of the kernel headers the rows are built around"""
    import re

    out = {}
    for name in ("vfo_rdsd_kernels.h", "vfo_sym_kernels.h"):
        with open(os.path.join(os.path.dirname(HERE), "sdrplusplus_amd", "csrc", name)) as f:
            for m in re.finditer(r"^#define (SDRPP_\w+) (\d+)\b", f.read(), re.M):
                out[m.group(1)] = int(m.group(2))
    return out


def test_the_rows_stand_at_the_kernel_headers_edges():
    """The constants the rows are built from (tests/rdsd_ref.py) are the kernel headers' own #defines — a chunk, a tap or a phase limit changed in the kernel moves
    the edges, and this test says so — and the table holds a row at every edge those constants make."""
    h = header_constants()
    assert (h["SDRPP_RDSD_CHUNK"], h["SDRPP_RDSD_MAX_TAPS"], h["SDRPP_SYM_MAX_INTERP_TAPS"], h["SDRPP_SYM_MAX_PHASES"], h["SDRPP_SYM_MAX_STEP"]) == (
        CHUNK, MAX_TAPS, MAX_INTERP_TAPS, MAX_PHASES, rdsd_ref.MAX_STEP)
    ids = {r.id for r in ROWS}
    for k in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 190, MAX_TAPS):
        assert "K%d" % k in ids
    for t in (1, 7, 8, 9, MAX_INTERP_TAPS):
        assert "T%d" % t in ids
    for p in (1, 127, 128, MAX_PHASES):
        assert "P%d" % p in ids
    for b in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        assert "block%d" % b in ids
    assert {"max_gain", "mm_clamps", "omega1.2", "omega70", "starts_on_edges"} <= ids
