"""The radio's IF chain per sample, at every edge of its two kernel bodies (vfo_nbsq_body in vfo_ifchain_kernels.h, vfo_fmif_body in vfo_fmif_kernels.h) — in the
manner of tests/test_meteor_rows.py and tests/test_rds_demod_rows.py.

tests/test_ifchain.py and tests/test_fmif.py feed the chain through a decimating channeliser, whose output on the device differs from the oracle's by about 1e-7, so they
keep every decision clear of its threshold and meet one geometry.  Here the input is EXACT: a RAW VFO whose input rate, IF rate and bandwidth are equal, at offset 0,
delivers what was pushed, bit for bit (every ordinary run asserts that of `vfo_read_if`), and a reference block is an IF block.  From there on

  * family A (blanker, squelch): every operation of the blanker is one IEEE float32 operation, so device, emulator and the float32 restatement of tests/test_ifchain.py
    agree in every word, compared as uint32 — thresholds met exactly included.  Only the squelch's sum is ordered differently (lane partials): where a squelch decision is
    not exact by construction the row asserts, on the restatement's side, |block level - squelch level| >= 0.05 dB;
  * family B (FMIF): a single non-zero sample makes each output ONE entry of the matrix (every other term of the fmaf chain is a product with an exact zero), so the
    winner on a tie — within a lane, and across the two lane halves through LDS — is visible in the output's bits: it must be the first bin of strictly largest
    float32 sqrtf((re * re) + (im * im)), as the reference's volk index_max gives.  The table is restated here as sdrpp_host::fmifMatrix builds it.  Noise rows stay
    under the rule of tests/test_fmif.py (Tally): 1e-5 x S_i, widened to the near-top set below a clearance of 1e-4;
  * family C: the rows with three pushes or more, pipelined with one block per launch and in launch groups of three, bit-equal to the ordinary passes.

Each row asserts its own edge from the kernels' constants (below) on the CPU before any device output is looked at.  c64 of tests/test_fmif.py is not used for the
[n, 2] blocks: its a + 1j * b loses the sign of a -0.0 and spreads a NaN to both parts; the blocks are viewed as complex64 instead.

N = 2 is left out of family B: its window is two rounding residues of about -2.4e-17 (nuttall(0, 1) and nuttall(1, 1)), nothing a radio would run.

Measured worst |got - want| / S_i over family B's noise rows: 2.8e-7 on the emulator and 2.8e-7 on an MI355X (every row prints its own)."""
import math

import numpy as np
import pytest

from test_fmif import Fmif, Tally, bits_equal
from test_ifchain import Blanker, Chain, squelch

f32 = np.float32
CHUNK = 64    # vfo_nbsq_body: samples per load, one per lane
ROUND = 256   # vfo_nbsq_body, squelch alone: four chunks per round
SEG = 256     # SDRPP_FMIF_SEG: samples per FMIF wave job
TILE = 32     # SDRPP_FMIF_TILE: samples per matrix tile
RATE = 24000.0
LAG = 16      # pipelined results are taken this many pushes behind (SDRPP_RESULT_SLOTS is 24)
NB = (0.25, 3.0)
FLT_MIN = float(np.finfo(np.float32).tiny)


def u32(a):
    return np.ascontiguousarray(np.asarray(a, np.complex64)).view(np.uint32)


def pairs(a):
    """an [n, 2] float32 block as complex64, every bit kept"""
    return np.ascontiguousarray(a, np.float32).view(np.complex64).reshape(-1).copy()


def blocks_of(p, R):
    """how a push of p samples is cut into reference blocks of R (0: the push is one block)"""
    return [p] if R == 0 else [R] * (p // R) + ([p % R] if p % R else [])


class Row:
    def __init__(self, id, x, cuts, edge, nb=None, sq=None, ref_block=0, bins=0, sq_exact=False):
        self.id, self.x, self.cuts, self.edge, self.nb, self.sq, self.ref_block, self.bins, self.sq_exact = id, np.asarray(x, np.complex64), list(cuts), edge, nb, sq, ref_block, bins, sq_exact
        assert sum(self.cuts) == len(self.x) <= 1100, id


# ---- the yardstick and the device -------------------------------------------------------------------------------------------------------
def run_ref(row):
    """-> dict(mid [the blanker / squelch output per push], amps [amp behind each push], closed [per squelch block], min_sq, fm [Fmif.process per push])"""
    ch = Chain(row.nb[0] if row.nb else None, row.nb[1] if row.nb else None, row.sq)
    fm = Fmif(row.bins) if row.bins else None
    ref = dict(mid=[], amps=[], closed=[], fm=[])
    pos = 0
    for p in row.cuts:
        xb = row.x[pos:pos + p]
        pos += p
        cut = blocks_of(p, row.ref_block)
        with np.errstate(all="ignore"):
            mid = ch.process(xb, cut)
        ref["mid"].append(mid)
        ref["amps"].append(ch.nb.amp if ch.nb is not None else None)
        if row.sq is not None:
            q = 0
            for c in cut:
                ref["closed"].append(not np.any(mid[q:q + c] != 0))
                q += c
        if fm is not None:
            ref["fm"].append(fm.process(mid))
    ref["min_sq"] = ch.min_sq
    return ref


def run_device(row, piped=None):
    """piped None: ordinary passes, the IF asserted bit-equal to what was pushed -> the chain's output per push.  piped 0: pipelined, one block per launch; piped n: in
    launch groups of n -> (the results per push, how much roles["ifc"] grew, pass_blocks)."""
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=4096)
    ctx.set_reference_block(row.ref_block)
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    vid = ctx.vfo_add(d, keep)
    if row.nb or row.sq is not None:
        f = capi.IfDesc()
        f.nb_enabled, f.nb_rate, f.nb_level = int(bool(row.nb)), float(row.nb[0]) if row.nb else 0.0, float(row.nb[1]) if row.nb else 0.0
        f.squelch_enabled, f.squelch_level = int(row.sq is not None), float(row.sq) if row.sq is not None else 0.0
        ctx.vfo_set_if(vid, f)
    if row.bins:
        ctx.vfo_set_fmnr(vid, True, row.bins)
    out, pos = [], 0
    if piped is None:
        for p in row.cuts:
            xb = row.x[pos:pos + p]
            pos += p
            ctx.push(xb)
            gi, fin = ctx.vfo_read_if(vid), ~np.isnan(xb)  # (a NaN does not pass RxVFO's rotator bit for bit: it reaches both parts, as in the reference)
            assert len(gi) == p and bits_equal(gi[fin], xb[fin]) and np.all(np.isnan(gi[~fin])), "%s: the IF is not what was pushed" % row.id
            got = ctx.vfo_ifc_read(vid).copy()
            assert bits_equal(pairs(ctx.vfo_read(vid)), got)  # a RAW VFO with a chain delivers the chain's output
            out.append(got)
        ctx.close()
        return out
    ctx.set_pipelined(True, 1)
    if piped:
        ctx.set_pipeline_group(piped, adaptive=False)
    before = ctx.pipeline_stats()["roles"].get("ifc", 0)
    pending = []

    def take():
        tk = pending.pop(0)
        out.append(pairs(ctx.result_wait(tk)["vfo"][vid]))
        ctx.result_release(tk)

    for tk, p in enumerate(row.cuts, start=1):
        ctx.push(row.x[pos:pos + p])
        pos += p
        pending.append(tk)
        if len(pending) > LAG:
            take()
    while pending:
        take()
    st = ctx.pipeline_stats()
    ctx.set_pipelined(False)
    ctx.close()
    return out, st["roles"].get("ifc", 0) - before, st["pass_blocks"]


def same_bits(got, want, what):
    assert [len(g) for g in got] == [len(w) for w in want], what
    g, w = u32(np.concatenate(got)), u32(np.concatenate(want))
    assert np.array_equal(g, w), "%s: %d words differ, first at sample %d" % (what, int((g != w).sum()), int(np.nonzero(g != w)[0][0]) // 2)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def stream(amps, seed, spikes=(), spike=40.0):
    """magnitudes `amps` x (0.8 .. 1.2) at random phases; at `spikes` the local amplitude x `spike` (the tracker at rate 0.25 reaches an excess of about 3.5 there)"""
    r = np.random.default_rng(1000 + seed)
    a = np.asarray(amps, np.float64) * r.uniform(0.8, 1.2, len(amps))
    for i in spikes:
        if 0 <= i < len(a):
            a[i] = amps[i] * spike
    return (a * np.exp(2j * np.pi * r.random(len(a)))).astype(np.complex64)


def alternating(n, stretch, hi, lo, restart=()):
    """stretches of `stretch` samples, alternately hi and lo, starting over with hi at every index of `restart` (where a push starts: so do the reference blocks)"""
    a, k = np.empty(n), 0
    for i in range(n):
        if i in restart:
            k = 0
        a[i] = hi if (k // stretch) % 2 == 0 else lo
        k += 1
    return a


def blanked(row, ref):
    return int(sum(np.sum((m != row.x[lo:lo + len(m)]) & (m != 0)) for m, lo in zip(ref["mid"], np.r_[0, np.cumsum(row.cuts)[:-1]])))


def excesses(x, rate):
    """the float32 excess of every sample as NoiseBlanker computes it (it does not depend on the level); 0 where the sample is zero"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(f32), x.imag.astype(f32)
    a = np.sqrt(re * re + im * im)
    rate = f32(rate)
    inv, amp, ex = f32(1.0) - rate, f32(1.0), np.zeros(len(x), f32)
    for i in range(len(x)):
        if a[i] != 0.0:
            amp = f32(f32(amp * inv) + f32(a[i] * rate))
            ex[i] = f32(a[i] / amp)
    return ex


def blank_without_select(x, rate, level):
    """the blanker with `amp` moving on zero samples too: what a kernel without the `!= 0` select would compute"""
    x = np.asarray(x, np.complex64)
    re, im = x.real.astype(f32), x.imag.astype(f32)
    a = np.sqrt(re * re + im * im)
    rate, level = f32(rate), f32(level)
    inv, amp, out = f32(1.0) - rate, f32(1.0), x.copy()
    for i in range(len(x)):
        amp = f32(f32(amp * inv) + f32(a[i] * rate))
        if a[i] != 0.0 and f32(a[i] / amp) > level:
            g = f32(f32(1.0) / f32(a[i] / amp))
            out[i] = complex(f32(re[i] * g), f32(im[i] * g))
    return out


# ---- A. blanker and squelch rows ---------------------------------------------------------------------------------------------------------
def length_(L, reps):
    """A1: pushes of L samples — below, at and above one and two chunks; with three pushes the second starts from the amp the first left"""
    n = L * reps
    x = stream(np.full(n, 0.3), 10 * L + reps, spikes=list(range(8, n, 8)) + ([L, 2 * L] if reps == 3 else []))

    def edge(row, ref):
        assert set(row.cuts) == {L} and len(row.cuts) == reps and L in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1)
        assert blanked(row, ref) >= (5 if n >= 60 else 0)
        if reps == 3:  # a blanker that started the second push at amp = 1 would give other bits
            assert ref["amps"][0] != f32(1.0)
            fresh, _ = Blanker(*NB).process(row.x[L:2 * L])
            assert not bits_equal(fresh, ref["mid"][1])
    return Row("len%d_x%d" % (L, reps), x, [L] * reps, edge, nb=NB)


def round_(P, R):
    """A2: squelch alone, two pushes of P samples: below, at and above one and two rounds of four chunks.  R = 0: a push is a block, the first loud and the second
    quiet; R = 100: blocks that start in mid-round, alternately loud and quiet"""
    n = 2 * P
    a = alternating(n, 100, 0.5, 0.005, restart=(P,))
    a[P:] *= 0.01
    x = stream(a, P)

    def edge(row, ref):
        assert row.nb is None and P in (ROUND - 1, ROUND, ROUND + 1, 2 * ROUND - 1, 2 * ROUND + 1) and row.cuts == [P, P]
        assert len(ref["closed"]) == 2 * len(blocks_of(P, R)) and True in ref["closed"] and False in ref["closed"]
        if R:
            assert R % CHUNK and ref["closed"][:3] == [False, True, False]
    return Row("round%d_block%d" % (P, R), x, [P, P], edge, sq=-20.0, ref_block=R)


def short_block_(R, cuts, name=None):
    """A3: blanker + squelch with reference blocks below, at and above a chunk; at R = 1 every sample is its own squelch block and its own chunk"""
    n = sum(cuts)
    starts = tuple(np.cumsum(cuts)[:-1])
    a = alternating(n, R, 0.5, 0.02, restart=starts)
    x = stream(a, 300 + R + len(cuts), spikes=range(6, n, 16))

    def edge(row, ref):
        assert row.ref_block == R and R in (1, CHUNK - 1, CHUNK, CHUNK + 1)
        assert len(ref["closed"]) == sum(len(blocks_of(p, R)) for p in cuts) and ref["closed"].count(True) >= 2 and ref["closed"].count(False) >= 2
        assert blanked(row, ref) >= 5
        if R == 1:
            assert len(ref["closed"]) == n
        if name:  # pushes that are no multiple of the block: a shorter last block, and a push shorter than a block
            assert all(p % R for p in cuts) and min(cuts) < R
    return Row(name or "block%d" % R, x, cuts, edge, nb=NB, sq=-10.0, ref_block=R)


ZEROS = [0, CHUNK, 2 * CHUNK - 1] + list(range(2 * CHUNK, 3 * CHUNK))  # the stream's first sample, lane 0, lane 63, a whole chunk
# -0.0 components that RxVFO's rotator, (1, 0) at offset 0, hands on as they are (re = xr * 1 - xi * 0, im = xr * 0 + xi * 1: a (0, -0) or a (0.5, -0) would arrive as +0):
# a zero sample with a sign bit, and two samples that carry a -0.0 beside a value
SIGNED = {70: complex(-0.0, 0.0), 71: complex(-0.0, 0.3), 72: complex(-0.3, -0.0)}


def zeros_blanker():
    """A4: exact zeros under the blanker: amp does not move on them and they pass with their sign bits"""
    x = stream(np.full(260, 0.3), 41, spikes=range(8, 260, 8))
    x[ZEROS] = 0
    for i, v in SIGNED.items():
        x[i] = v

    def edge(row, ref):
        assert row.cuts == [260] and all(row.x[i] == 0 for i in ZEROS + [70])
        assert [int(w) >> 31 for w in u32(row.x[70:73])] == [1, 0, 1, 0, 1, 1]
        assert np.array_equal(u32(ref["mid"][0][ZEROS + list(SIGNED)]), u32(row.x[ZEROS + list(SIGNED)]))
        without = blank_without_select(row.x, *NB)
        assert not bits_equal(without, ref["mid"][0]) and blanked(row, ref) >= 5  # had the select been missing amp would have moved, and the output with it
    return Row("zeros_blanker", x, [260], edge, nb=NB)


def zeros_squelch():
    """A4: an all-zero block (-0.0 components among them) under the squelch: log10f(0) = -inf, the block closes and its output is +0"""
    x = stream(np.full(192, 0.5), 42, spikes=range(8, 192, 8))
    x[CHUNK:2 * CHUNK] = 0
    x[70] = SIGNED[70]

    def edge(row, ref):
        assert row.ref_block == CHUNK and ref["closed"] == [False, True, False]
        assert np.any(u32(row.x[CHUNK:2 * CHUNK]) != 0) and not np.any(u32(ref["mid"][0][CHUNK:2 * CHUNK]) != 0)
    return Row("zeros_squelch", x, [192], edge, nb=NB, sq=-20.0, ref_block=CHUNK)


def threshold_(below):
    """A5: nb_level equal to an excess that occurs: that sample is not blanked (strict >); one ulp below it is"""
    x = stream(np.full(200, 0.3), 51, spikes=range(8, 200, 8))
    ex = excesses(x, NB[0])
    i = int(np.argmin(np.abs(ex.astype(np.float64) - 3.0)))
    at = ex[i]
    lower = np.nextafter(at, f32(0.0))
    level = lower if below else at

    def edge(row, ref):
        assert f32(row.nb[1]) == level and at > 1.0
        a, _ = Blanker(NB[0], at).process(row.x)
        b, _ = Blanker(NB[0], lower).process(row.x)
        assert a[i] == row.x[i] and b[i] != row.x[i] and not bits_equal(a, b)  # the two yardstick outputs differ in that sample
        assert bits_equal(ref["mid"][0], b if below else a)
    return Row("threshold_" + ("one_ulp_below" if below else "exact"), x, [200], edge, nb=(NB[0], float(level)))


def unit_block_(level, name, closes):
    """A6: samples from {1, -1, j, -j}: every magnitude is exactly 1, every order of summation gives exactly n, the mean is exactly 1 and log10f(1.0f) exactly 0.
    Levels 0.0 and -0.0 open the block (dB >= level), 1e-30 closes it."""
    r = np.random.default_rng(60)
    x = np.array([1, -1, 1j, complex(0.0, -1.0)], np.complex64)[r.integers(0, 4, 357)]  # (+0 beside the -1: -1j is (-0, -1), whose -0 the rotator does not hand on)

    def edge(row, ref):
        assert set(np.abs(row.x).astype(np.float64)) == {1.0} and float(np.log10(f32(1.0), dtype=f32)) == 0.0
        assert ref["closed"] == [closes, closes]
    return Row("squelch_level_" + name, x, [100, ROUND + 1], edge, sq=level, sq_exact=True)


def nan_block():
    """A7: one NaN component in a loud block closes it (power_squelch.h:42: `if (dB >= level) copy else zero`); the blocks behind it are unaffected"""
    x = stream(np.full(400, 0.5), 70)
    x[150] = complex(float("nan"), 0.5)

    def edge(row, ref):
        assert row.nb is None and ref["closed"] == [False, True, False, False] and np.isnan(row.x[100:200]).sum() == 1
        with np.errstate(all="ignore"):
            _, dbs = squelch(row.x, [100] * 4, row.sq)
        assert np.isnan(dbs[1]) and np.all(np.abs(np.delete(dbs, 1) - row.sq) >= 0.05)  # (the loud blocks keep the clearance; the NaN block needs none)
    return Row("nan_closes_its_block", x, [300, 100], edge, sq=-20.0, ref_block=100, sq_exact=True)


def tiny():
    """A8: magnitudes around 1e-20: the squares are denormal or underflow to 0, and a sample whose re * re + im * im is 0 counts as zero"""
    r = np.random.default_rng(80)
    mag = 10.0 ** r.uniform(-24.0, -19.0, 400)
    mag[::8] *= 40.0
    x = (mag * np.exp(2j * np.pi * r.random(400))).astype(np.complex64)

    def edge(row, ref):
        re, im = row.x.real.astype(f32), row.x.imag.astype(f32)
        sq = re * re + im * im
        assert ((sq > 0) & (sq < FLT_MIN)).sum() >= 50 and ((sq == 0) & (row.x != 0)).sum() >= 50
        _, ratio = Blanker(*NB).process(row.x)
        assert not np.any(ratio[sq == 0]) and np.array_equal(u32(ref["mid"][0][sq == 0]), u32(row.x[sq == 0]))
        assert blanked(row, ref) >= 5
    return Row("tiny_amplitudes", x, [400], edge, nb=NB)


A_ROWS = ([length_(L, reps) for reps in (1, 3) for L in (1, 2, 63, 64, 65, 127, 128, 129)] + [round_(P, R) for R in (0, 100) for P in (255, 256, 257, 511, 513)] +
          [short_block_(R, [130, 257]) for R in (1, 63, 64, 65)] + [short_block_(64, [100, 1, 191], "ragged_block64"), zeros_blanker(), zeros_squelch(), threshold_(False),
           threshold_(True), unit_block_(0.0, "plus0", False), unit_block_(-0.0, "minus0", False), unit_block_(1e-30, "1e-30", True), nan_block(), tiny()])


@pytest.mark.parametrize("row", A_ROWS, ids=[r.id for r in A_ROWS])
def test_blanker_squelch_row(backend, row):
    """Device (or emulator) and the float32 restatement agree in every word of the chain's output, as uint32."""
    ref = run_ref(row)
    row.edge(row, ref)
    if row.sq is not None and not row.sq_exact:
        assert ref["min_sq"] >= 0.05, "TEST BUG: a block within 0.05 dB of the squelch level (%.3g dB)" % ref["min_sq"]
    same_bits(run_device(row), ref["mid"], row.id)


# ---- B. FMIF rows -------------------------------------------------------------------------------------------------------------------------
def fmif_table(N):
    """sdrpp_host::fmifMatrix restated: -> (re, im)[n][k], float32.  The window in double as window/cosine.h sums it, stored as float; the angle reduced exactly."""
    a4 = (0.355768, 0.487396, 0.144232, 0.012604)
    re, im = np.zeros((N, N), f32), np.zeros((N, N), f32)
    for n in range(N):
        acc, sign = 0.0, 1.0
        for i in range(4):
            acc += sign * a4[i] * math.cos(float(i) * 2.0 * math.pi * float(n) / float(N - 1))
            sign = -sign
        w = float(f32(acc))
        for k in range(N):
            a = -2.0 * math.pi * float((k * (n - N // 2)) % N) / float(N)
            re[n, k], im[n, k] = f32(w * math.cos(a)), f32(w * math.sin(a))
    return re, im


# (the third one carries a -0.0 into the products; it is -0.5 - 0j because RxVFO's rotator hands a 0.5 - 0j on as 0.5 + 0j: see SIGNED)
IMPULSES = {"1": complex(1.0, 0.0), "j": complex(0.0, 1.0), "minus_half": complex(-0.5, -0.0)}
IMPULSE_CASES = [(N, "1") for N in range(3, 33)] + [(N, v) for v in ("j", "minus_half") for N in (31, 32)]


def impulse_bins(N, v):
    """Every bin's output for the N windows a lone sample v passes through, d = 0 .. N - 1 samples behind it: the kernel's accumulators start at +0 and take
    re += Ar * xr, im += Ai * xr, re += Ai * (-xi), im += Ar * xi; with one non-zero component each sum has one non-zero term, and a -0 never survives +0 + (-0).
    -> (re, im, mag)[d][k], float32"""
    tr, ti = fmif_table(N)
    xr, xi = f32(IMPULSES[v].real), f32(IMPULSES[v].imag)
    cols = np.arange(N - 1, -1, -1)  # the sample sits at column n = N - 1 - d
    re = (f32(0.0) + tr[cols] * xr) + ti[cols] * (-xi)
    im = (f32(0.0) + ti[cols] * xr) + tr[cols] * xi
    return re, im, np.sqrt(re * re + im * im)


def impulse_want(N, v, n, at):
    re, im, mag = impulse_bins(N, v)
    want = np.zeros((n, 2), f32)
    k = np.argmax(mag, axis=1)  # the first bin of strictly largest float32 magnitude
    want[at:at + N, 0], want[at:at + N, 1] = re[np.arange(N), k], im[np.arange(N), k]
    return pairs(want)


def impulse_row(N, v, single):
    n, at = 3 * N + 7, N + 5
    x = np.zeros(n, np.complex64)
    x[at] = IMPULSES[v]

    def edge(row, ref):
        assert at >= N and n - at >= 2 * N and np.count_nonzero(row.x) == 1 and row.bins == N
        assert (at // TILE != (at + N - 1) // TILE) == (14 <= N <= 26 or N >= 30)  # there the sample's outputs lie in two tiles
    return Row("impulse_%s_N%d_%s" % (v, N, "pushes_of_1" if single else "one_push"), x, [1] * n if single else [n], edge, bins=N)


def half_of(k):
    return (k >> 2) & 1  # the lane half that holds bin k's accumulator (vfo_fmif_body: k = (r & 3) + 8 * (r >> 2) + 4 * h)


def test_impulses_tie_in_every_class():
    """CPU only.  Over all impulse rows the float32 maximum is shared by several bins (a) within one lane half, (b) across the halves with the lowest k in half 0,
    (c) across the halves with the lowest k in half 1 — and in at least 10 cases of each the bin a flipped comparison would take differs in bits."""
    seen, visible = [0, 0, 0], [0, 0, 0]
    for N, v in IMPULSE_CASES:
        re, im, mag = impulse_bins(N, v)
        for d in range(N):
            tied = [int(k) for k in np.nonzero(mag[d] == mag[d].max())[0]]
            if len(tied) < 2:
                continue
            k0 = tied[0]
            bits = lambda k: (re[d, k].view(np.uint32), im[d, k].view(np.uint32))
            near = [k for k in tied[1:] if half_of(k) == half_of(k0)]
            far = [k for k in tied[1:] if half_of(k) != half_of(k0)]
            if near:  # `>=` within the lane takes the last one
                seen[0] += 1
                visible[0] += int(bits(near[-1]) != bits(k0))
            if far:  # the other half's own winner is its first
                c = 1 + half_of(k0)
                seen[c] += 1
                visible[c] += int(bits(far[0]) != bits(k0))
    print("[ifchain rows] tied impulse windows: same half %d (%d visible), lowest k in half 0 %d (%d), in half 1 %d (%d)" % (seen[0], visible[0], seen[1], visible[1], seen[2], visible[2]))
    assert min(visible) >= 10, (seen, visible)


@pytest.mark.parametrize("N,v", IMPULSE_CASES, ids=["%s_N%d" % (v, N) for N, v in IMPULSE_CASES])
def test_impulse_row(backend, N, v):
    """A lone sample in a stream of zeros, in one push and in pushes of 1: every output bit-equal to the matrix entry of the first maximal bin; +0 elsewhere."""
    for single in (False, True):
        row = impulse_row(N, v, single)
        row.edge(row, None)
        want = impulse_want(N, v, len(row.x), int(np.nonzero(row.x)[0][0]))
        got = np.concatenate(run_device(row))
        bad = np.nonzero((u32(got) != u32(want)).reshape(-1, 2).any(axis=1))[0]
        assert not len(bad), "%s: %d outputs differ, first %d samples behind the impulse: got %r, want %r" % (row.id, len(bad), bad[0] - np.nonzero(row.x)[0][0], got[bad[0]], want[bad[0]])


def noise(n, seed, sigma=0.3):
    r = np.random.default_rng(seed)
    return (sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64)


WORST = {}


def tally(row, ref, got, cap=0):
    """Tally.check over every sample.  cap: the 1 % cap of Tally.done over the samples from `cap` on (None: no cap)"""
    t, tc = Tally(), Tally()
    assert len(got) == len(ref["fm"])
    pos = 0
    for i, (g, r) in enumerate(zip(got, ref["fm"])):
        t.check(g, r, "%s push %d" % (row.id, i))
        if cap is not None and pos + len(g) > cap:
            s = max(cap - pos, 0)
            tc.check(g[s:], {k: v[s:] for k, v in r.items()}, row.id)
        pos += len(g)
    if cap is not None:
        tc.done(row.id)
    WORST[row.id] = t.worst
    print("[ifchain rows] %s: worst |got - want| / S %.3g; over family B so far %.3g" % (row.id, t.worst, max(WORST.values())))
    return t


def bins_row(N):
    def edge(row, ref):
        assert row.bins == N and 3 <= N <= TILE and row.cuts == [300, 300] and 300 > SEG  # two segments a push, the second one 44 samples: a tile of 12
    return Row("bins%d" % N, noise(600, 3000 + N), [300, 300], edge, bins=N)


@pytest.mark.parametrize("N", range(3, 33))
def test_every_bin_count(backend, N):
    """Every bin count the C-ABI admits but 2 (see the module's docstring), against the float64 yardstick under the Tally rule; at most 1 % of the samples decided by
    rounding.  N = 3: the window is (~0, 1, ~0), every bin has the same magnitude in exact arithmetic and every bin's output is x[i - 1] — the 1 % cap does not
    apply, the output must also lie within the bound of x[i - 1]."""
    row = bins_row(N)
    ref = run_ref(row)
    row.edge(row, ref)
    got = run_device(row)
    tally(row, ref, got, cap=0 if N != 3 else None)
    if N == 3:  # (the window's two residues w[0], w[2] of about -2.4e-17 times their samples are what the output holds beside x[i - 1])
        g = np.concatenate(got).astype(np.complex128)
        S = np.concatenate([r["S"] for r in ref["fm"]])
        xx = np.abs(np.r_[0.0, 0.0, row.x.astype(np.complex128)])
        w = np.abs(Fmif(3).w)
        prev = np.r_[0.0, row.x[:-1].astype(np.complex128)]
        assert np.all(np.abs(g - prev) <= 1e-5 * S + w[0] * xx[:-2] + w[2] * xx[2:])


def cut_row(N, first, name=None):
    if first == 1:
        cuts = [1] * 100

        def edge(row, ref):
            assert len(row.cuts) == 100 and N - 1 > 2  # a window reaches across N - 1 pushes
    else:
        cuts = [first, 40]

        def edge(row, ref):
            assert first in (5, TILE - 1, TILE, TILE + 1, SEG - 1, SEG, SEG + 1, 2 * SEG + 1) and (first != 5 or first < N - 1)  # 5: a window longer than everything seen so far
    return Row(name or "N%d_first%d" % (N, first), noise(sum(cuts), 4000 + 40 * N + first), cuts, edge, bins=N)


CUT_ROWS = [cut_row(N, first) for N in (32, 9) for first in (31, 32, 33, 255, 256, 257, 513)] + [cut_row(32, 1, "N32_pushes_of_1"), cut_row(9, 1, "N9_pushes_of_1"), cut_row(32, 5)]


@pytest.mark.parametrize("row", CUT_ROWS, ids=[r.id for r in CUT_ROWS])
def test_cut_edges(backend, row):
    """First pushes that end below, at and above a tile, a segment and two segments, pushes of one sample, and a first push shorter than the window: under the Tally
    rule, and bit-equal to the same stream pushed at once.  The 1 % cap counts from the first full window on: behind the empty line a window holds one sample, then
    two, ... — every bin ties on the first, and rows of 71 samples cannot keep that one below 1 %."""
    ref = run_ref(row)
    row.edge(row, ref)
    got = run_device(row)
    tally(row, ref, got, cap=row.bins - 1)
    once = run_device(Row(row.id + "_at_once", row.x, [len(row.x)], row.edge, bins=row.bins))
    assert bits_equal(np.concatenate(got), once[0])


def behind_squelch():
    """B4: closed blocks reach FMIF as zeros, and the N - 1 samples behind them see those zeros"""
    x = stream(alternating(600, 50, 0.5, 0.005), 90)

    def edge(row, ref):
        c = ref["closed"]
        assert row.bins == 16 and row.nb is None and row.ref_block == 50 and len(c) == 12
        assert c.count(True) >= 2 and sum(1 for a, b in zip(c, c[1:]) if a and not b) >= 2
        mid = np.concatenate(ref["mid"])
        assert not np.any(mid[50:100] != 0) and np.all(mid[100:150] != 0)
    return Row("fmif_behind_squelch", x, [200, 200, 200], edge, sq=-20.0, ref_block=50, bins=16)


def test_fmif_behind_the_squelch(backend):
    row = behind_squelch()
    ref = run_ref(row)
    row.edge(row, ref)
    assert ref["min_sq"] >= 0.05, "TEST BUG: a block within 0.05 dB of the squelch level (%.3g dB)" % ref["min_sq"]
    tally(row, ref, run_device(row), cap=None)  # (no cap: the windows at the six edges of a closed block hold one sample, two, ... and tie as those behind an empty line do)


def test_nothing_behind_the_push_is_read(backend):
    """A segment job that took SDRPP_FMIF_SEG samples whatever the push holds would read the stream's buffer behind the push.  For the outputs themselves that only
    matters with an odd bin count: the last matrix step pairs column N - 1 with a zero column, and what that one multiplies is the window entry behind the push's
    last sample — zero by the kernel's load predicate, else whatever an earlier, longer push left there.  So: N = 9, a push of 40 samples with a NaN at index 20, then a
    push of 20, whose last sample would meet 0 x NaN.  (The NaN has left the delay line by then.  The first push is compared up to two samples in front of the NaN:
    for the same reason — and this is the kernel as it is, stated in its header: "what it multiplies must be finite" — an odd bin count lets a NaN or an infinity
    reach the output ONE sample early, N + 1 outputs where the reference spoils N.)"""
    N, first, second = 9, 40, 20
    x = noise(first + second, 5000)
    x[second] = complex(float("nan"), float("nan"))
    row = Row("stale_behind_the_push", x, [first, second], None, bins=N)
    assert N % 2 == 1 and second + (N - 1) < first - (N - 1) and second < first < SEG
    ref = run_ref(row)
    assert not np.any(np.isnan(ref["fm"][1]["out"])) and np.isnan(ref["fm"][0]["out"]).sum() == N
    got = run_device(row)
    t = Tally()
    t.check(got[0][:second - 1], {k: v[:second - 1] for k, v in ref["fm"][0].items()}, row.id + ", in front of the NaN")
    t.check(got[1], ref["fm"][1], row.id + ", second push")


def test_nothing_behind_the_push_is_written(backend):
    """... and it would store a whole segment.  A push of 300 samples, then one of 20 into the same buffer: what the first left behind sample 20 is still there."""
    from sdrplusplus_amd import capi, radio

    def held(ptr, n):
        ctx.sync()
        a = np.empty(n, np.complex64)
        capi._copy_from_device(ctx.L, a.ctypes.data, ptr, n * 8)
        return a

    first, second = 300, 20
    x = noise(first + second, 5001)
    ctx = capi.Context(0, max_push=4096)
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_fmnr(vid, True, 9)
    ctx.push(x[:first])
    ptr, n = ctx.vfo_ifc_device_buffer(vid)
    a = held(ptr, first)
    assert n == first > SEG and bits_equal(a, ctx.vfo_ifc_read(vid)) and np.all(a != 0)
    ctx.push(x[first:])
    ptr2, n2 = ctx.vfo_ifc_device_buffer(vid)
    assert (ptr2, n2) == (ptr, second) and second < TILE  # (the same buffer: else this test sees nothing)
    b = held(ptr, first)
    assert bits_equal(b[:second], ctx.vfo_ifc_read(vid)) and not bits_equal(b[:second], a[:second])
    assert bits_equal(b[second:], a[second:])
    ctx.close()


# ---- C. the same rows as ticks-----------------------------------------------------------------------------------------------------------
TICK_ROWS = ([r for r in A_ROWS if len(r.cuts) >= 3] + [impulse_row(N, v, True) for N, v in IMPULSE_CASES] + [r for r in CUT_ROWS if len(r.cuts) >= 3] + [behind_squelch()])


@pytest.mark.parametrize("group", [0, 3], ids=["block_per_launch", "groups_of_3"])
@pytest.mark.parametrize("row", TICK_ROWS, ids=[r.id for r in TICK_ROWS])
def test_row_as_ticks(backend, row, group):
    """Pipelined, one block per launch and in launch groups of three: the results of every push bit-equal to the ordinary passes' vfo_read; the blocks ran as ticks
    with the chain as a role, none as an ordinary pass."""
    assert len(row.cuts) >= 3
    want = run_device(row)
    got, grew, passes = run_device(row, piped=group)
    same_bits(got, want, "%s, group %d" % (row.id, group))
    assert grew >= 1 and passes == 0, (grew, passes)
