"""The pager's symbol branch (vfo_sym_kernels.h: the WK_SYM_FRONT and WK_SYM_LOOP kinds of the wavefront-job role), symbol by symbol and BIT FOR BIT.

test_pager.py runs ONE description (radio.pager_desc: ten equal shaping taps, the 128 x 8 interpolator, the pager's gains) and, apart from six fixture cases in
pushes of 500, compares two runs of the device with each other.  Here every edge of the two bodies, of the planner's cutting and of the control surface is placed
on purpose — ROWS below, one row per edge, each stating what it is there for — and every soft value, bit and per-push count is compared with a restatement.

THE RESTATEMENT (Restate) is POCSAGDSP::process (pocsag/dsp.h) in numpy over a `dtype`, resuming across pushes from its own state: the discriminator (quadrature.h:
arctan2, the difference against the BRANCH's previous phase — 0 at a fresh attach and after sdrpp_vfo_reset, unmoved while the branch is off — normalizePhase with
FL_PI = 3.1415926535f, * inv_deviation), the shaping FIR (k ascending over [K - 1 carried values][block], product and sum rounded apart) and MM<float>::process
(clock_recovery/mm.h:100-156) as written: the work buffer [T - 1 carried][block], clamp(floorf(phase * P), 0, P - 1), the dot product k ascending, the error from
step(), its clamp, pcl.advance with the omega clamp, floorf, offset += delta, offset -= count, and the memmove of the last T - 1 values (a block shorter than T - 1
included).  It counts the hits of every clamp side and records the symbol steps and the per-push offsets and counts.  float32 is the reference's arithmetic; float64
only serves the printed report.  test_restatement_is_the_reference_per_symbol pins it, without a device, to every case of tests/golden/pager_ref.npz.

EXACT ROWS: INPUTS ON THE FOUR AXES.  Every IF sample is (a, 0), (0, a), (-a, 0) or (0, -a) with the zero part +0.0.  In fm_phase (vfo_fir_kernels.h) that gives
z = 0 * rcp(max) = 0, r = 0 and a result of exactly 0, float32(pi / 2), float32(pi) or -float32(pi / 2): atan2f's own answer.  Behind that point every operation
of the branch is a single IEEE float32 operation in the reference's order (the library is built without contraction), so the device must equal the float32
restatement BIT FOR BIT — soft values as uint32, bits, per-push counts — and no tolerance hides a wrong sample behind a phase-bin flip of MM's recursion.  The
discriminator's stream takes the values {0, +-pi / 2, pi} x inv_deviation in random order; shaping taps and interpolator banks are random, every entry different
and none small (|h| >= 0.1 max |h|), so a wrong tap, phase or sample index always shows (design_mm_interp's T = 1 bank is about 1e-6 and would hide one).
Rows go through the transparent RAW VFO of test_pager.add_transparent and first assert that vfo_read_if is the input bit for bit; the launch-group and mixed-bank
rows sit behind a one-tap decimate-by-2 stage (test_rds_rows' hand_desc) whose output must be every second input sample bit for bit.

CONDITIONS, asserted on the CPU before a device's output is looked at (check_exact): the row's own edge restated from the kernel's constants (front_tiles, the hit
counters, the steps), at least 50 symbols (large-omega rows: 6), soft RMS >= 1e-3, and no float32 intermediate of the restatement a non-zero value below 1e-30.

SIGNAL ROWS (real FSK behind the real wideband chain, radio.pager_desc at 2400 / 1200 / 512 baud, the restatement fed what vfo_read_if delivered): the device's
discriminator is a polynomial, not atan2f, so the bar is test_pager.py's: counts equal, bits equal where |soft_ref| >= 0.05, soft within max(1e-5 RMS, 4 x
spread), the spread from the RESTATEMENT by make_pager_golden.py's recipe (eight float32 runs, every input part scaled by 1 +- 2^-24, per-symbol maximum).
Conditions on the CPU: all nine runs agree in counts and bits, at most 1 % weak symbols, the bar at its floor for at least 90 % of the symbols.  Seeds are chosen
by these conditions alone."""
import math

import numpy as np
import pytest

from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_kernel_forms import hand_desc
from test_pager import GOLDEN, IF_RATE, bits_equal, case_input, fsk, rms

# the kernel's constants (vfo_sym_kernels.h), under the names the source gives them
SEG, TILE, PACK, MAX_STEP = 1024, 256, 64, 4096
LOAD_ROUND, CHUNK = 256, 64  # the phase loader's round (64 lanes x U = 4 loads in flight), the difference pass's chunk
FL_PI = np.float32(3.1415926535)
INV_DEV = np.float32(1.0 / (2.0 * math.pi * (4500.0 / IF_RATE)))
MIN_SYMBOLS, MIN_SYMBOLS_LARGE, MIN_RMS, TINY = 50, 6, 1e-3, 1e-30
INF = float("inf")
LAG = 16  # results are taken this many pushes behind (SDRPP_RESULT_SLOTS is 24)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
class Restate:
    """cfg: dict(inv_dev, taps [K], bank [P, T], omega, mu, og, mn, mx), float32 values.  push(y) -> (soft, bits) of that push; reset() for sdrpp_vfo_reset;
    fresh() for a new POCSAGDSP.  hits: clamp sides hit; steps: floorf(phase) per symbol; offsets / counts: per push."""

    def __init__(self, cfg, f=np.float32):
        self.c, self.f = cfg, f
        self.h = [f(np.float32(v)) for v in cfg["taps"]]
        self.bank = np.asarray(cfg["bank"], np.float32).astype(f)
        self.P, self.T = self.bank.shape
        self.K = len(self.h)
        self.inv_dev, self.alpha, self.beta = (f(np.float32(cfg[k])) for k in ("inv_dev", "mu", "og"))
        self.mn, self.mx = f(np.float32(cfg["mn"])), f(np.float32(cfg["mx"]))
        self.hits = dict(err_hi=0, err_lo=0, om_hi=0, om_lo=0, phase=0)
        self.steps, self.offsets, self.counts, self.softs, self.pidx = [], [], [], [], set()
        self.tiny = INF
        self.fresh()

    def fresh(self):
        f = self.f
        self.prev, self.line, self.fh = f(0), np.zeros(self.K - 1, f), np.zeros(self.T - 1, f)
        self.phase, self.freq, self.last, self.off = f(0), f(np.float32(self.c["omega"])), f(0), 0

    def reset(self):
        self.prev = self.f(0)

    def _seen(self, a):
        a = np.abs(np.asarray(a, np.float64)).reshape(-1)
        a = a[a > 0.0]
        if a.size:
            self.tiny = min(self.tiny, float(a.min()))

    def push(self, y):
        f, n, K, T = self.f, len(y), self.K, self.T
        self.offsets.append(self.off)
        if n == 0:  # (process(0): nothing moves)
            self.counts.append(0)
            return np.zeros(0, np.float32), np.zeros(0, np.uint8)
        PI = f(FL_PI)
        TWO = f(2) * PI
        # quadrature.h:39-46
        ph = np.arctan2(y.imag.astype(np.float32).astype(f), y.real.astype(np.float32).astype(f)).astype(f)
        d = (ph - np.concatenate([[self.prev], ph[:-1]]).astype(f)).astype(f)
        self.prev = ph[-1]
        d = np.where(d > PI, d - TWO, np.where(d <= -PI, d + TWO, d)).astype(f)
        d = (d * self.inv_dev).astype(f)
        self._seen(d)
        # FIR<float, float>: k ascending over [line][block], product and sum rounded apart
        buf = np.concatenate([self.line, d]).astype(f)
        acc = np.zeros(n, f)
        for k in range(K):
            prod = (buf[k:k + n] * self.h[k]).astype(f)
            acc = (acc + prod).astype(f)
            self._seen(prod)
            self._seen(acc)
        self.line = buf[n:].copy()
        # MM<float>::process
        work = np.concatenate([self.fh, acc]).astype(f)
        fP, one, zero = f(self.P), f(1), f(0)
        off, phase, freq, last = self.off, self.phase, self.freq, self.last
        out_vals, seen = [], []
        while off < n:
            p = int(np.floor(phase * fP))
            if p < 0 or p > self.P - 1:
                self.hits["phase"] += 1
                p = min(max(p, 0), self.P - 1)
            self.pidx.add(p)
            prod = (work[off:off + T] * self.bank[p]).astype(f)
            out = zero
            for v in prod:
                out = out + v
                seen.append(out)
            seen.extend(prod)
            out_vals.append(out)
            error = (((one if last > 0 else -one) * out) - (last * (one if out > 0 else -one)))
            last = out
            seen.append(error)
            if error > one:
                error = one
                self.hits["err_hi"] += 1
            if error < -one:
                error = -one
                self.hits["err_lo"] += 1
            be, ae = self.beta * error, self.alpha * error
            freq = freq + be
            if freq > self.mx:
                freq = self.mx
                self.hits["om_hi"] += 1
            elif freq < self.mn:
                freq = self.mn
                self.hits["om_lo"] += 1
            phase = phase + (freq + ae)
            seen.extend((be, ae, phase))
            delta = np.floor(phase)
            off += int(delta)
            self.steps.append(int(delta))
            phase = phase - delta
            seen.append(phase)
        self.off, self.phase, self.freq, self.last = off - n, phase, freq, last
        self.fh = work[n:n + T - 1].copy()
        self._seen(seen)
        soft = np.asarray(out_vals, f).astype(np.float32) if out_vals else np.zeros(0, np.float32)
        self.counts.append(len(soft))
        self.softs.append(np.asarray(out_vals, np.float64))
        return soft, (np.asarray(out_vals, f) > 0).astype(np.uint8) if out_vals else np.zeros(0, np.uint8)


def cat(parts):
    return (np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.float32), np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint8))


def cfg_of_pager(baud):
    from sdrplusplus_amd import radio

    d, keep = radio.pager_desc(IF_RATE, baud)
    return dict(inv_dev=np.float32(d.inv_deviation), taps=keep[0].copy(), bank=keep[1].copy(), omega=np.float32(d.omega), mu=np.float32(d.mu_gain), og=np.float32(d.omega_gain),
                mn=np.float32(d.min_omega), mx=np.float32(d.max_omega))


# ---- 1. the restatement against the reference's recorded outputs: no context, no device --------------------------------------------------------
FIXTURE_CASES = ["steady_2400", "steady_1200", "steady_512", "noisy_2400", "cuts", "reset"]
FIXTURE_DISTANCE = 1e-6  # four times the largest |restatement - recorded| / RMS this test's own CPU run shows over the cases (2.43e-7): numpy's arctan2 against atan2f


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_restatement_is_the_reference_per_symbol(name):
    """CPU only.  The float32 restatement over the fixture's input in the fixture's cuts, a fresh chain where the fixture starts one: counts exactly the recorded
    ones, every bit equal where |soft_ref| >= 0.05, soft values within the bar test_pager.py gives the device for that case (numpy's arctan2 need not be glibc's
    atan2f bit for bit)."""
    z = np.load(GOLDEN)
    x, cut, fresh = case_input(z, name), z[name + "_cut"], z[name + "_reset"]
    ref_soft, ref_bits = z[name + "_soft"], z[name + "_bits"]
    cfg = cfg_of_pager(float(z[name + "_baud"]))
    r32, r64 = Restate(cfg, np.float32), Restate(cfg, np.float64)
    parts, pos = [], 0
    for b, n in enumerate(cut):
        if b in fresh:
            r32.fresh()
            r64.fresh()
        parts.append(r32.push(x[pos:pos + int(n)]))
        r64.push(x[pos:pos + int(n)])
        pos += int(n)
    soft, bits = cat(parts)
    assert r32.counts == [int(c) for c in z[name + "_counts"]], (name, r32.counts)
    strong = np.abs(ref_soft) >= 0.05
    assert np.array_equal(bits[strong], ref_bits[strong]) and np.array_equal(bits, (soft > 0).astype(np.uint8))
    err = soft.astype(np.float64) - ref_soft.astype(np.float64)
    R = rms(ref_soft)
    bar_each = np.maximum(1e-5 * R, 4.0 * z[name + "_dev_max"].astype(np.float64))
    bar_rms = max(1e-5 * R, 4.0 * float(z[name + "_dev_rms"]))
    exact = int(np.sum(soft.view(np.uint32) == ref_soft.view(np.uint32)))
    s64 = np.concatenate(r64.softs) if r64.counts == r32.counts else None
    print("\n[pager rows] fixture %s: %d symbols, %d bit-equal to the recorded ones, largest distance %.3g of the RMS (bar %.3g), rms %.3g (bar %.3g); float32 vs float64 restatement %s" % (
        name, len(soft), exact, np.abs(err).max() / R, bar_each.min() / R, rms(err) / R, bar_rms / R, "%.3g" % (np.abs(soft - s64).max() / R) if s64 is not None else "(counts differ)"))
    assert np.all(np.abs(err) <= bar_each), (name, float(np.abs(err).max()))
    assert rms(err) <= bar_rms
    assert np.abs(err).max() / R <= FIXTURE_DISTANCE, (name, np.abs(err).max() / R)
    assert r32.hits["phase"] == 0


# ---- descriptions and inputs --------------------------------------------------------------------------------------------------------------------
_cfgs = {}


def make_cfg(K=10, T=8, P=128, omega=10.0, mu=1.0, og=0.01, rel=0.05, mn=None, mx=None, seed=0):
    """random shaping taps and a random interpolator bank: magnitudes 0.1 .. 1 of the largest, random signs, every entry different"""
    key = (K, T, P, omega, mu, og, rel, mn, mx, seed)
    if key not in _cfgs:
        rng = np.random.default_rng(7000 + 131 * K + 17 * T + P + seed)
        mags = lambda m: 0.1 + 0.9 * (rng.permutation(m) + rng.uniform(0.25, 0.75, m)) / m  # noqa: E731  (a shuffled grid with jitter: no two magnitudes alike)
        taps = (mags(K) * rng.choice([-1.0, 1.0], K) * (2.0 / math.sqrt(K))).astype(np.float32)
        bank = (mags(P * T).reshape(P, T) * rng.choice([-1.0, 1.0], (P, T)) * (1.0 / math.sqrt(T))).astype(np.float32)
        assert len(set(np.abs(taps).tolist())) == K and len(set(np.abs(bank).reshape(-1).tolist())) == P * T
        assert np.min(np.abs(taps)) >= 0.1 * np.max(np.abs(taps)) and np.min(np.abs(bank)) >= 0.1 * np.max(np.abs(bank))
        c = dict(inv_dev=INV_DEV, taps=taps, bank=bank, omega=np.float32(omega), mu=np.float32(mu), og=np.float32(og),
                 mn=np.float32(omega * (1.0 - rel) if mn is None else mn), mx=np.float32(omega * (1.0 + rel) if mx is None else mx))
        assert c["mn"] - abs(c["mu"]) >= 1.0 and c["mx"] + abs(c["mu"]) <= MAX_STEP and c["mn"] < c["mx"]  # what sym_apply takes
        c["key"] = key
        _cfgs[key] = c
    return _cfgs[key]


def sym_desc_of(cfg):
    from sdrplusplus_amd import capi, radio

    s = capi.SymDesc()
    taps, bank = np.ascontiguousarray(cfg["taps"], np.float32), np.ascontiguousarray(cfg["bank"], np.float32)
    s.inv_deviation, s.shape_ntaps, s.shape_taps = float(cfg["inv_dev"]), len(taps), radio._fp(taps)
    s.omega, s.mu_gain, s.omega_gain, s.min_omega, s.max_omega = (float(cfg[k]) for k in ("omega", "mu", "og", "mn", "mx"))
    s.interp_phases, s.interp_ntaps, s.interp_bank = bank.shape[0], bank.shape[1], radio._fp(bank)
    return s, [taps, bank]


def axis_walk(n, seed):
    """a seeded walk over the four axes: quadrant steps of -1, 0, +1 and 2, amplitudes 0.05 .. 0.9, the zero part +0.0"""
    rng = np.random.default_rng(seed)
    q = np.cumsum(rng.integers(0, 4, n)) % 4
    a = rng.uniform(0.05, 0.9, n).astype(np.float32)
    x = np.zeros(n, np.complex64)
    x.real = np.where(q == 0, a, np.where(q == 2, -a, np.float32(0.0)))
    x.imag = np.where(q == 1, a, np.where(q == 3, -a, np.float32(0.0)))
    v = x.view(np.float32)
    assert not np.any((v == 0) & np.signbit(v)) and np.all((x.real == 0) != (x.imag == 0))
    return x


def front_tiles(n, K, T):
    """vfo_sym_front_body, restated: the tiles of a block of n IF samples -> [(cnt, is the tail tile, first tile of a job)]"""
    out = []
    for lo in range(0, n, SEG):
        hi = min(lo + SEG, n)
        for t0 in range(lo, hi, TILE):
            out.append((min(TILE, hi - t0), False, t0 == lo))
    if n > 0:
        out.append((max(1, min(T - 1, n)), True, False))
    return out


def if_counts(cuts, dec):
    """IF samples per push behind a one-tap stage decimating by `dec`: outputs sit at input indices 0, dec, 2 dec .."""
    out, pos = [], 0
    for n in cuts:
        out.append((pos + n + dec - 1) // dec - (pos + dec - 1) // dec)
        pos += n
    return out


def fill(cuts, total=6000, piece=700):
    cuts = list(cuts)
    while sum(cuts) < total:
        cuts.append(min(piece, total - sum(cuts)))
    assert sum(cuts) == total
    return cuts


class Row:
    """build() -> dict(x, vfos [(cfg, dec)], scale, ops, edge (callable(case, restatements per VFO) with the row's own CPU assertions), large (the 6-symbol
    floor)); `why`: the edge the row places; groups: the launch groups the row also runs pipelined in."""

    def __init__(self, rid, family, why, build, groups=()):
        self.id, self.family, self.why, self.build, self.groups = rid, family, why, build, groups


def pushes(cuts):
    return [("push", int(n)) for n in cuts]


DEFAULT_CUTS = fill([997, 7, 1, 1250, 256, 1025, 3])


def tiles_of(case, j=0):
    cfg, dec = case["vfos"][j]
    K, T = len(cfg["taps"]), cfg["bank"].shape[1]
    t = []
    for n in if_counts([o[1] for o in case["ops"] if o[0] == "push"], dec):
        t += front_tiles(n, K, T)
    return K, T, t


def _plain(cfg, cuts=None, edge=None, seed=1, large=False):
    def build():
        c = DEFAULT_CUTS if cuts is None else cuts
        return dict(x=axis_walk(sum(c), seed), vfos=[(cfg(), 1)], ops=pushes(c), edge=edge, large=large)
    return build


def _edge_k(K):
    def edge(case, rs):
        k, T, tiles = tiles_of(case)
        assert k == K and any(c == TILE for c, tail, _ in tiles if not tail) and any(c < TILE for c, tail, _ in tiles if not tail)
        if K == 64:
            assert any(c + K == TILE + 64 for c, tail, _ in tiles)  # the largest window: 320 elements
    return edge


def _edge_t(T):
    def edge(case, rs):
        _k, t, tiles = tiles_of(case)
        assert t == T and rs[0].T == T and {c for c, tail, _ in tiles if tail} >= {max(1, T - 1), 1}  # a full tail tile, and one behind a block of one sample
        if T == 1:
            assert all((T - 1) - c == -1 for c, tail, _ in tiles if tail)  # dst0 = -1: the tail tile stores no output
    return edge


def _edge_p(P):
    def edge(case, rs):
        assert rs[0].P == P
        assert len(rs[0].pidx) >= min(P, 40) and max(rs[0].pidx) >= P - 1 - P // 8, (P, len(rs[0].pidx))  # the walk visits the bank, its far end included
    return edge


def _edge_windows(prop, want):
    def edge(case, rs):
        K, _T, tiles = tiles_of(case)
        got = {prop(c, K) for c, tail, _ in tiles if not tail}
        assert set(want) <= got, (sorted(set(want) - got), K)
    return edge


def _edge_blocks(want, K=None, T=None):
    def edge(case, rs):
        k, t, _ = tiles_of(case)
        ns = [o[1] for o in case["ops"] if o[0] == "push"]
        assert set(want) <= set(ns), ns
        assert (K is None or k == K) and (T is None or t == T)
    return edge


def _edge_hits(*sides):
    def edge(case, rs):
        for s in sides:
            assert rs[0].hits[s] >= 1, (s, rs[0].hits)
    return edge


def _edge_min2(case, rs):
    r = rs[0]
    n = len(case["x"])
    assert 1 in r.steps and sum(r.counts) >= n // 3 and max(r.steps) <= 4, (sum(r.counts), set(r.steps))  # steps of ONE sample; cap_of(n) = n + 1 symbols of room


def _edge_large(job_too):
    def edge(case, rs):
        r = rs[0]
        ns = [o[1] for o in case["ops"] if o[0] == "push"]
        assert sum(1 for n in ns if n < min(r.steps)) >= len(ns) // 2  # steps longer than a push
        if job_too:
            assert min(r.steps) > SEG and max(ns) > SEG                    # ... and than a job
        zero_runs, run_ = 0, 0
        for c in r.counts:
            run_ = run_ + 1 if c == 0 else 0
            zero_runs = max(zero_runs, run_)
        assert zero_runs >= (2 if job_too else 1), r.counts                 # pushes in a row without a symbol
        assert any(a > n for a, n in zip(r.offsets, ns)), r.offsets        # an offset carried down across a whole push
        assert min(r.steps) >= 800 and max(r.steps) <= MAX_STEP + 1
    return edge


def _edge_ones(case, rs):
    ns = [o[1] for o in case["ops"] if o[0] == "push"]
    assert ns.count(1) >= 200 and rs[0].counts.count(0) > 150 and rs[0].counts.count(1) >= 15


def _ctl(kind, seed):
    """the control surface: 3000 samples in pushes of 250, the switch in front of pushes 3, 6 and 9"""
    def build():
        cfg, other = make_cfg(K=10, T=8, P=128), make_cfg(K=7, T=5, P=64, omega=12.0, seed=3)
        x = axis_walk(3750, seed)
        ops = []
        for i in range(12):
            if i in (3, 6, 9):
                if kind == "off":
                    ops += [("off",)] + pushes([235, 1, 14]) + [("on",)]
                elif kind == "other":
                    ops += [("other", other)]
                else:
                    ops += [(kind,)]
            ops += pushes([250 if i != 7 else 249]) + (pushes([1]) if i == 7 else [])

        total = sum(o[1] for o in ops if o[0] == "push")
        x = x[:total].copy()
        pos = 0
        for o in ops:
            if o[0] == "push":
                pos += o[1]
            elif o[0] == "reset":
                x[pos - 1] = np.complex64(0.3j)  # the sample in front of the reset: phase pi / 2

        def edge(case, rs):
            at, nblocks = 0, 0
            for o in case["ops"]:
                if o[0] == "push":
                    at, nblocks = at + o[1], nblocks + 1
                elif o[0] == "reset":
                    assert at > 0 and case["x"][at - 1].imag != 0, "the sample in front of the reset has phase 0"
            assert total == (3750 if kind == "off" else 3000)
        return dict(x=x, vfos=[(cfg, 1)], ops=ops, edge=edge)
    return build


GROUP_CUTS = fill([601] + [1] * 10 + [2049, 1, 1, 5, 1, 3000, 1, 1, 1, 2, 1, 1, 777, 2, 2, 1, 1500, 1, 1, 1, 1, 1, 1, 1, 1, 1, 4], total=12000, piece=900)


def _group(seed):
    def build():
        def edge(case, rs):
            ifn = if_counts(GROUP_CUTS, 2)
            assert 0 in ifn and 1 in ifn and max(ifn) > SEG and GROUP_CUTS.count(1) >= 20
            assert any(n > 0 and c == 0 for n, c in zip(ifn, rs[0].counts))  # a push with samples and without a symbol
        return dict(x=axis_walk(sum(GROUP_CUTS), seed), vfos=[(make_cfg(K=10, T=8, P=128), 2)], scale=2, ops=pushes(GROUP_CUTS), edge=edge)
    return build


def bank_cfgs():
    return [make_cfg(K=10, T=8, P=128, omega=10.0), make_cfg(K=1, T=1, P=2, omega=2.05, mn=2.0, mx=2.1, mu=1.0), make_cfg(K=33, T=5, P=127, omega=7.3, mu=-0.6),
            make_cfg(K=64, T=16, P=1024, omega=15.0, og=0.05, rel=0.01), make_cfg(K=2, T=8, P=128, omega=12.0, seed=9)]


def _bank(nv, n, mixed, cuts, seed):
    def build():
        cfgs = bank_cfgs()
        vfos = [(cfgs[i % 5], 2 if (mixed and i % 2) else 1) for i in range(nv)]

        def edge(case, rs):
            assert {c["bank"].shape[1] for c in cfgs} == {1, 5, 8, 16} and len({c["key"] for c in cfgs}) == 5
            njobs = (nv + PACK - 1) // PACK
            per = (nv + njobs - 1) // njobs
            assert njobs == {5: 1, 65: 2, 130: 3}[nv] and per == {5: 5, 65: 33, 130: 44}[nv]  # plan_vfo.h: the records spread evenly over as few jobs as 64 lanes allow
            if mixed:
                for k in range(0, nv, per):
                    assert {d for _c, d in vfos[k:k + per]} == {1, 2}  # lanes of one job differ in n
        return dict(x=axis_walk(n, seed), vfos=vfos, scale=2 if mixed else 1, ops=pushes(cuts), edge=edge, banks=5)
    return build


def K_(K):
    return Row("k%d" % K, "taps", "K = %d shaping taps (T = 8, 128 phases): full and partial tiles%s" % (K, ", the largest window of 320" if K == 64 else ""),
               _plain(lambda: make_cfg(K=K), edge=_edge_k(K), seed=10 + K))


def T_(T):
    why = {1: "no interpolator history: the tail tile stores nothing, index -1 is reached", 8: "the fast path", 16: "the largest T"}.get(T, "the generic path")
    return Row("t%d" % T, "interp", "T = %d interpolator taps (K = 10): %s" % (T, why), _plain(lambda: make_cfg(T=T), edge=_edge_t(T), seed=30 + T))


def P_(P):
    return Row("p%d" % P, "phases", "%d interpolator phases (K = 10)%s" % (P, ": phase index 0 whatever the phase" if P == 1 else ""), _plain(lambda: make_cfg(P=P, T=8 if P != 127 else 7), edge=_edge_p(P), seed=50 + P % 9))


ROWS = [K_(K) for K in (1, 2, 10, 33, 63, 64)] + [T_(T) for T in (1, 2, 7, 8, 9, 15, 16)] + [P_(P) for P in (1, 2, 127, 128, 1024)] + [
    # ---- front windows ----
    Row("win_round", "front", "the loader's round: tiles of cnt + K = 255, 256, 257 (K = 10)",
        _plain(lambda: make_cfg(K=10), fill([245, 246, 247, 1024 + 245, 1024 + 246, 1024 + 247]), _edge_windows(lambda c, K: c + K, (LOAD_ROUND - 1, LOAD_ROUND, LOAD_ROUND + 1)), seed=61)),
    Row("win_chunk", "front", "the difference chunk: cnt + K - 1 = 63, 64, 65 and 127, 128, 129 (K = 10)",
        _plain(lambda: make_cfg(K=10), fill([54, 55, 56, 118, 119, 120, 1024 + 55, 256 + 119]), _edge_windows(lambda c, K: c + K - 1, (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)), seed=62)),
    Row("win_cnt", "front", "four outputs per lane: cnt = 63, 64, 65, 191, 192, 193, 255, 256 (K = 33)",
        _plain(lambda: make_cfg(K=33), fill([63, 64, 65, 191, 192, 193, 255, 256, 1024 + 65, 512 + 192]), _edge_windows(lambda c, K: c, (63, 64, 65, 191, 192, 193, 255, 256)), seed=63)),
    # ---- block lengths ----
    Row("blk_k64_short", "block", "blocks of 1 and 2 samples with K = 64: the new line is spliced from the old one",
        _plain(lambda: make_cfg(K=64), fill([500] + [1, 2] * 30 + [63, 1, 1, 64, 2]), _edge_blocks((1, 2, 63, 64), K=64), seed=64)),
    Row("blk_t16_fh", "block", "blocks of T - 2, T - 1 and T samples with T = 16: the fh splice",
        _plain(lambda: make_cfg(T=16), fill([500, 14, 15, 16, 14, 14, 3, 15, 1, 16, 2, 2, 2]), _edge_blocks((14, 15, 16, 1, 2, 3), T=16), seed=65)),
    Row("blk_seg", "block", "blocks of SEG - 1, SEG and SEG + 1 samples: one job, and a second of one sample",
        _plain(lambda: make_cfg(), fill([SEG - 1, SEG, SEG + 1]), _edge_blocks((SEG - 1, SEG, SEG + 1)), seed=66)),
    Row("blk_seg1_k64_t16", "block", "SEG + 1 with K = 64, T = 16: the last job owns one sample, its tail tile and window reach back over the job boundary",
        _plain(lambda: make_cfg(K=64, T=16), fill([SEG + 1, 2 * SEG + 1, SEG + 1]), _edge_blocks((SEG + 1, 2 * SEG + 1), K=64, T=16), seed=67)),
    Row("blk_2seg_tile", "block", "2 x SEG + TILE + 1: three jobs, the last of a full tile and a tile of one",
        _plain(lambda: make_cfg(K=33, T=9), fill([2 * SEG + TILE + 1, 2 * SEG + TILE + 1]), _edge_blocks((2 * SEG + TILE + 1,)), seed=68)),
    Row("blk_ones", "block", "a run of 200 one-sample pushes (K = 10, T = 8)",
        _plain(lambda: make_cfg(), fill([300] + [1] * 200), _edge_ones, seed=69)),
    # ---- the loop ----
    Row("loop_err", "loop", "the error clamp, both sides", _plain(lambda: make_cfg(K=10, seed=1), edge=_edge_hits("err_hi", "err_lo"), seed=70)),
    Row("loop_omega", "loop", "omega gain 0.05, relative limit 0.01: both omega limits", _plain(lambda: make_cfg(og=0.05, rel=0.01), edge=_edge_hits("om_hi", "om_lo", "err_hi", "err_lo"), seed=71)),
    Row("loop_min2", "loop", "min_omega = 2, mu_gain = 1: steps of one sample, thousands of symbols", _plain(lambda: make_cfg(omega=2.05, mn=2.0, mx=2.1, mu=1.0), edge=_edge_min2, seed=72)),
    Row("loop_neg_mu", "loop", "a negative mu_gain", _plain(lambda: make_cfg(mu=-0.7, T=7), edge=lambda case, rs: rs[0].alpha < 0, seed=73)),
    Row("loop_om900", "loop", "omega 900: steps longer than a push of 500, pushes without a symbol, the offset carried down",
        _plain(lambda: make_cfg(omega=900.0, og=0.5, mu=1.0), fill([500] * 4 + [2100], piece=500), _edge_large(False), seed=74, large=True)),
    Row("loop_om3900", "loop", "omega 3900 with |mu_gain| = 1: steps longer than a job and than a push, several pushes in a row without a symbol",
        _plain(lambda: make_cfg(omega=3900.0, mn=3800.0, mx=4000.0, og=2.0, mu=-1.0), fill([1500] * 5 + [2000], total=21500, piece=1500), _edge_large(True), seed=75, large=True)),
    # ---- the control surface, absolute ----
    Row("ctl_off_on", "control", "off for three pushes of other samples, then on: the branch, its previous phase included, does not move", _ctl("off", 80)),
    Row("ctl_reset", "control", "sdrpp_vfo_reset in front of a sample of non-zero phase, behind an odd and an even number of blocks: the previous phase alone becomes 0", _ctl("reset", 81)),
    Row("ctl_replace", "control", "sdrpp_vfo_replace with keep & 2: everything moves to the new handle", _ctl("replace", 82)),
    Row("ctl_fresh", "control", "detach and attach: a fresh chain", _ctl("fresh", 83)),
    Row("ctl_other", "control", "another description and back: a fresh chain", _ctl("other", 84)),
    # ---- launch groups and blocks without samples (behind a one-tap decimate-by-2 stage) ----
    Row("groups", "group", "pipelined in launch groups of 1, 3 and 8: pushes of one input sample (IF blocks of 0 and 1 samples), pushes without a symbol inside a group", _group(90), groups=(1, 3, 8)),
    # ---- mixed banks ----
    Row("bank5", "bank", "five VFOs, five descriptions, T = 8, 1, 5, 16, 8: lanes of one wavefront on both paths, five device banks", _bank(5, 6000, False, DEFAULT_CUTS, 91)),
    Row("bank65", "bank", "65 VFOs cycling through them, every second behind the decimate-by-2 stage: two loop jobs of 33 and 32 lanes in one workgroup, lanes that differ in n",
        _bank(65, 2400, True, fill([997, 7, 1, 1, 500], total=2400), 92)),
    Row("bank130", "bank", "130 VFOs: three loop jobs of 44, 44 and 42 lanes", _bank(130, 2000, True, fill([900, 1, 3], total=2000), 93)),
]


# ---- running ----------------------------------------------------------------------------------------------------------------------------------
_cases = {}


def prepare(row):
    if row.id not in _cases:
        case = row.build()
        for k, v in (("scale", 1), ("large", False), ("banks", 1), ("edge", None)):
            case.setdefault(k, v)
        assert sum(o[1] for o in case["ops"] if o[0] == "push") == len(case["x"]), row.id
        _cases[row.id] = case
    return dict(_cases[row.id])


def vfo_desc_of(case, dec):
    from sdrplusplus_amd import radio

    if case["scale"] == 1:
        assert dec == 1
        d, keep = radio.vfo_desc(IF_RATE, IF_RATE, IF_RATE, 0.0, "RAW")  # test_pager.add_transparent's
        return d, keep
    d, keep, _rate = hand_desc(2 * IF_RATE, 0.0, *(([(2, np.ones(1, np.float32))],) if dec == 2 else ()))
    return d, keep


def known_if(case, dec):
    return case["x"] if dec == 1 else np.ascontiguousarray(case["x"][::dec])


def run(case, group=0, watch=None):
    """-> dict(out [per VFO [(soft, bits) per push the branch was on for]], ifs {VFO: the IF stream it delivered}, stats, groups).  group > 0: pipelined in launch
    groups of that many pushes (plain schedules only).  watch: the VFOs whose IF is read (default: the first of each decimation)."""
    from sdrplusplus_amd import capi

    sizes = [o[1] for o in case["ops"] if o[0] == "push"]
    mp = max(sum(sizes[i:i + max(1, group)]) for i in range(len(sizes)))
    ctx = capi.Context(0, max_push=max(mp, 256))
    vids, descs, syms = [], [], []
    for cfg, dec in case["vfos"]:
        d, keep = vfo_desc_of(case, dec)
        vids.append(ctx.vfo_add(d, keep))
        descs.append((d, keep))
        syms.append(sym_desc_of(cfg))
        ctx.vfo_set_symbols(vids[-1], syms[-1][0], True, syms[-1][1])
    if watch is None:
        decs = [d for _c, d in case["vfos"]]
        watch = sorted(decs.index(d) for d in set(decs))
    out, ifs, pending = [[] for _ in vids], {j: [] for j in watch}, []
    on, pos, tickets = True, 0, 0
    if group:
        assert all(o[0] == "push" for o in case["ops"])
        ctx.set_pipelined(True, 1 | capi.RESULT_SYM)
        ctx.set_pipeline_group(group)

    def take():
        tk = pending.pop(0)
        res = ctx.result_wait(tk)
        for k, v in enumerate(vids):
            out[k].append(ctx.result_sym(tk, v))
        for j in watch:
            ifs[j].append(np.ascontiguousarray(res["vfo"][vids[j]]).view(np.complex64).reshape(-1).copy())
        ctx.result_release(tk)

    for op in case["ops"]:
        if op[0] == "push":
            ctx.push(case["x"][pos:pos + op[1]])
            pos += op[1]
            if group:
                tickets += 1
                pending.append(tickets)
                if len(pending) > LAG:
                    take()
                continue
            for k, v in enumerate(vids):
                if on:
                    out[k].append(ctx.vfo_sym_read(v))
                else:
                    assert ctx.vfo_sym_count(v) == 0
            for j in watch:
                ifs[j].append(ctx.vfo_read_if(vids[j]).copy())
        elif op[0] in ("on", "off"):
            on = op[0] == "on"
            for v, (sd, sk) in zip(vids, syms):
                ctx.vfo_set_symbols(v, sd, on, sk)
        elif op[0] == "reset":
            for v in vids:
                ctx.vfo_reset(v)
        elif op[0] == "replace":
            vids = [ctx.vfo_replace(v, d, 3, keep) for v, (d, keep) in zip(vids, descs)]
        elif op[0] == "fresh":
            for v, (sd, sk) in zip(vids, syms):
                ctx.vfo_set_symbols(v, None)
                ctx.vfo_set_symbols(v, sd, True, sk)
        else:
            assert op[0] == "other", op
            od, ok = sym_desc_of(op[1])
            for v, (sd, sk) in zip(vids, syms):
                ctx.vfo_set_symbols(v, od, True, ok)
                ctx.vfo_set_symbols(v, sd, True, sk)
    while pending:
        take()
    banks = ctx.sym_bank_count()
    st = ctx.pipeline_stats()
    gs = ctx.pipeline_group_stats() if group else None
    if group:
        ctx.set_pipelined(False)
    ctx.close()
    return dict(out=out, ifs={j: np.concatenate(v) for j, v in ifs.items()}, stats=st, groups=gs, banks=banks, tickets=tickets)


_restated = {}


def restated(row, case, j):
    """the float32 Restate of VFO j over its IF in the case's schedule and its per-push (soft, bits); computed once per row, description and decimation, then left alone"""
    cfg, dec = case["vfos"][j]
    key = (row.id, cfg["key"], dec)
    if key not in _restated:
        r = Restate(cfg, np.float32)
        parts, pos, on = [], 0, True
        y = known_if(case, dec)
        counts = iter(if_counts([o[1] for o in case["ops"] if o[0] == "push"], dec))
        for op in case["ops"]:
            if op[0] == "push":
                n = next(counts)
                if on:
                    s, b = r.push(y[pos:pos + n])
                    s.setflags(write=False)
                    b.setflags(write=False)
                    parts.append((s, b))
                pos += n
            elif op[0] in ("on", "off"):
                on = op[0] == "on"
            elif op[0] == "reset":
                r.reset()
            elif op[0] in ("fresh", "other"):
                r.fresh()
        assert pos == len(y)
        _restated[key] = (r, parts)
    return _restated[key]


def check_exact(row, case):
    """The CPU conditions of a row, before a device's output is looked at -> [(Restate, parts)] per VFO"""
    res = [restated(row, case, j) for j in range(len(case["vfos"]))]
    for j, (r, parts) in enumerate(res):
        soft = cat(parts)[0]
        assert len(soft) >= (MIN_SYMBOLS_LARGE if case["large"] else MIN_SYMBOLS), (row.id, j, len(soft))
        assert rms(soft) >= MIN_RMS, (row.id, j, rms(soft))
        assert r.tiny >= TINY, (row.id, j, "an intermediate of", r.tiny)
        assert np.all(np.isfinite(soft))
    if case["edge"]:
        assert case["edge"](case, [r for r, _p in res]) is not False, row.id
    return res


def compare(row, what, got, want, j):
    assert [len(p[0]) for p in got] == [len(p[0]) for p in want], (row.id, what, "VFO %d: symbols per push" % j, [len(p[0]) for p in got], [len(p[0]) for p in want])
    gs, gb = cat(got)
    ws, wb = cat(want)
    if not np.array_equal(gs.view(np.uint32), ws.view(np.uint32)):
        at = int(np.argmax(gs.view(np.uint32) != ws.view(np.uint32)))
        raise AssertionError((row.id, what, "VFO %d: soft values differ, first at symbol %d of %d: %r against %r; %d differ" % (j, at, len(ws), gs[at], ws[at], int(np.sum(gs.view(np.uint32) != ws.view(np.uint32))))))
    assert np.array_equal(gb, wb) and np.array_equal(gb, (gs > 0).astype(np.uint8)), (row.id, what, j, "bits")


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_pager_symbol_by_symbol(backend, row):
    case = prepare(row)
    res = check_exact(row, case)
    runs = [("ordinary passes", run(case))] + [("launch groups of %d" % g, run(case, group=g)) for g in row.groups]
    for what, a in runs:
        for j, y in a["ifs"].items():
            assert bits_equal(y.view(np.float32), known_if(case, case["vfos"][j][1]).view(np.float32)), (row.id, what, "VFO %d: the IF is not the input" % j)
        assert a["banks"] == case["banks"], (row.id, a["banks"])
        for j, (_r, parts) in enumerate(res):
            compare(row, what, a["out"][j], parts, j)
        if a["groups"] is not None:
            assert a["stats"]["pass_blocks"] == 0 and a["stats"]["tick_blocks"] == a["tickets"] > 0, (row.id, what, a["stats"])
            g = int(what.split()[-1])
            if g > 1:
                assert a["groups"]["multi_groups"] >= 2 and a["groups"]["largest"] == g, (row.id, what, a["groups"])
    r = res[0][0]
    print("\n[pager rows %s] %s: %d VFOs, %d symbols of VFO 0 bit-equal; clamp hits %s, steps %d .. %d" % (row.id, backend, len(res), sum(r.counts), r.hits, min(r.steps), max(r.steps)))


def test_every_row_states_its_edge_and_the_table_is_complete():
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids) and all(len(r.why) > 8 for r in ROWS)
    assert {r.family for r in ROWS} == {"taps", "interp", "phases", "front", "block", "loop", "control", "group", "bank"}
    Ks, Ts, Ps, hits = set(), set(), set(), dict(err_hi=0, err_lo=0, om_hi=0, om_lo=0)
    for r in ROWS:
        case = prepare(r)
        assert len(case["x"]) // case["scale"] <= 6000 or case["large"], r.id
        for cfg, _d in case["vfos"][:5]:
            Ks.add(len(cfg["taps"]))
            Ts.add(cfg["bank"].shape[1])
            Ps.add(cfg["bank"].shape[0])
    assert {1, 2, 10, 33, 63, 64} <= Ks and {1, 2, 7, 8, 9, 15, 16} <= Ts and {1, 2, 127, 128, 1024} <= Ps
    for rid in ("loop_err", "loop_omega"):
        row = ROWS[ids.index(rid)]
        rr = restated(row, prepare(row), 0)[0]
        for k in hits:
            hits[k] += rr.hits[k]
    assert all(v >= 1 for v in hits.values()), hits  # every clamp side is hit by some row


# ---- 3. signal rows: real FSK behind the real wideband chain ------------------------------------------------------------------------------------
SR, OFFSETS = 240e3, {2400.0: 30e3, 1200.0: -45e3, 512.0: 80e3}
SIGNALS = [  # id, the baud rates of the bank, launch group (0: ordinary passes), seed
    ("sig_chain", (2400.0,), 0, 41),
    ("sig_groups3", (2400.0,), 3, 42),
    ("sig_bank3", (2400.0, 1200.0, 512.0), 0, 43),
]
SIG_CUTS = [9970, 70, 10, 12500, 2500, 5000, 30, 10240, 10250, 9420]  # 60 000 samples: 6 000 at the IF rate


def run_signal(bauds, x, group):
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=max(sum(SIG_CUTS[i:i + max(1, group)]) for i in range(len(SIG_CUTS))))
    vids = []
    for baud in bauds:
        d, keep = radio.vfo_desc(SR, IF_RATE, 12.5e3, OFFSETS[baud], "RAW")
        vids.append(ctx.vfo_add(d, keep))
        sd, sk = radio.pager_desc(IF_RATE, baud)
        ctx.vfo_set_symbols(vids[-1], sd, True, sk)
    out, ifs, pos = [[] for _ in vids], [[] for _ in vids], 0
    if group:
        ctx.set_pipelined(True, 1 | capi.RESULT_SYM)
        ctx.set_pipeline_group(group)
    for n in SIG_CUTS:
        ctx.push(x[pos:pos + n])
        pos += n
        if not group:
            for k, v in enumerate(vids):
                out[k].append(ctx.vfo_sym_read(v))
                ifs[k].append(ctx.vfo_read_if(v).copy())
    if group:
        for t in range(1, len(SIG_CUTS) + 1):
            res = ctx.result_wait(t)
            for k, v in enumerate(vids):
                out[k].append(ctx.result_sym(t, v))
                ifs[k].append(np.ascontiguousarray(res["vfo"][v]).view(np.complex64).reshape(-1).copy())
            ctx.result_release(t)
        st, gs = ctx.pipeline_stats(), ctx.pipeline_group_stats()
        assert st["pass_blocks"] == 0 and gs["multi_groups"] >= 2 and gs["largest"] == group, (st, gs)
        ctx.set_pipelined(False)
    ctx.close()
    return out, ifs


def restate_signal(cfg, blocks, seed):
    """-> (parts of the float32 restatement, per-symbol spread, the spread's RMS) by make_pager_golden.py's recipe; the nine runs must agree in counts and bits"""
    def once(bl):
        r = Restate(cfg, np.float32)
        return [r.push(b) for b in bl], r

    parts, r0 = once(blocks)
    soft, bits = cat(parts)
    rng = np.random.default_rng(1000 + seed)
    dev = np.zeros((8, len(soft)), np.float64)
    for k in range(8):
        pert = []
        for b in blocks:
            v = b.view(np.float32)
            sgn = np.where(rng.integers(0, 2, v.shape) == 1, 1.0, -1.0)
            pert.append((v.astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32).view(np.complex64))
        pk, rk = once(pert)
        assert rk.counts == r0.counts, "run %d differs in its symbol counts: another seed" % k
        sk, bk = cat(pk)
        assert np.array_equal(bk, bits), "run %d differs in a bit: another seed" % k
        dev[k] = sk.astype(np.float64) - soft.astype(np.float64)
    return parts, np.abs(dev).max(axis=0), float(np.sqrt(np.mean(dev * dev)))


@pytest.mark.parametrize("sig", SIGNALS, ids=[s[0] for s in SIGNALS])
def test_pager_signal_rows(backend, sig):
    rid, bauds, group, seed = sig
    x = sum(fsk(sum(SIG_CUTS), seed=seed + i, f0=OFFSETS[b], baud=b) for i, b in enumerate(bauds)).astype(np.complex64)  # a carrier per baud rate, each at its VFO's offset
    out, ifs = run_signal(bauds, x, group)
    for k, baud in enumerate(bauds):
        assert sum(len(b) for b in ifs[k]) == 6000
        parts, dev_max, dev_rms = restate_signal(cfg_of_pager(baud), ifs[k], seed)  # the CPU conditions come first: the device's symbols are looked at below
        ref_soft, ref_bits = cat(parts)
        R = rms(ref_soft)
        strong = np.abs(ref_soft) >= 0.05
        assert len(ref_soft) >= MIN_SYMBOLS and int((~strong).sum()) <= 0.01 * len(ref_soft), (rid, baud, int((~strong).sum()), len(ref_soft))
        bar_each = np.maximum(1e-5 * R, 4.0 * dev_max)
        bar_rms = max(1e-5 * R, 4.0 * dev_rms)
        assert np.mean(bar_each <= 1e-5 * R) >= 0.9, (rid, baud, "the bar leaves its floor for more than 10 % of the symbols", float(np.mean(bar_each <= 1e-5 * R)))
        assert [len(p[0]) for p in out[k]] == [len(p[0]) for p in parts], (rid, baud, "symbols per push")
        soft, bits = cat(out[k])
        err = soft.astype(np.float64) - ref_soft.astype(np.float64)
        print("\n[pager rows %s %g baud] %s: %d symbols, soft error max %.3g rms %.3g of the RMS; largest error / bar %.3g, rms / bar %.3g" % (
            rid, baud, backend, len(soft), np.abs(err).max() / R, rms(err) / R, float(np.max(np.abs(err) / bar_each)), rms(err) / bar_rms))
        assert np.array_equal(bits[strong], ref_bits[strong]) and np.array_equal(bits, (soft > 0).astype(np.uint8)), (rid, baud)
        assert np.all(np.abs(err) <= bar_each), (rid, baud, int(np.argmax(np.abs(err) / bar_each)), float(np.max(np.abs(err) / bar_each)))
        assert rms(err) <= bar_rms, (rid, baud)
