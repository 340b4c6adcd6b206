"""The WFM stereo decoder (vfo_stereo_kernels.h: the pilot, loop and matrix jobs of the IF chain's role), sample by sample.

test_stereo.py compares whole streams by RMS (bar 1e-5) at ONE geometry — 317 pilot taps, delay 159, 250 kS/s — and everything else there is one device path
against another.  A wrong frame per tile moves an RMS over 12 000 frames by less than that bar.  Here every edge of the three bodies and of the planner's packing
is placed on purpose — ROWS below, one row per edge, each stating what it is there for — and every output frame is compared, from the first one on.

THE RESTATEMENT (restate) is broadcast_fm.h:147-191 written in numpy over a `dtype`: float64 is the yardstick, float32 the sequential baseline (one rounding per
operation, no fused multiply-add, the reference's order): discriminator (atan2, normalizePhase, * invDeviation) -> complex pilot FIR on (m + 0j), taps k-ascending
-> loop::PLL (error, freq += beta * err, clamp, phase += freq + alpha * err, the two wrap loops with FL_PI = 3.1415926535f) -> the delay D -> the two complex
products -> l = m_D + lmr, r = m_D - lmr -> the audio FIR per channel.  It takes the stream's state and resumes across pushes, and besides the audio returns the
indices where the clamp held (signed by the limit), the number of phase wraps, the loop's wrap margin min | |ang - phase| - pi |, the discriminator's margin
min | |dphase| - pi | and min |p| behind the first K samples.  test_restatement_is_the_reference_per_sample pins it, without a device, to the reference's recorded
frames of tests/golden/stereo_ref*.npz in the fixture's block schedule.

ISOLATION.  The restatement's input is the product's own IF for the same pushes, delivered by a RAW twin on the same chain (test_af_chain.py's trick; behind an IF
chain the twin carries the same chain, so its output is what the chain delivered).  Identity-chain rows (offset 0, no stage, no resampler, no channel filter)
first assert that this IF equals the input bit for bit.

THE BAR, per row, job and quantity (l, r, l - r): dist(device, ref64) <= MARGIN x dist(float32 restatement, ref64), dist = max-abs over every frame / rms(ref64)
(test_kernel_forms.py's; MARGIN, BASELINE_MAX and the 1.25 rule are imported); the baselines are recorded in BASELINES from this file's own CPU run.

CONDITIONS BEFORE A DEVICE RUNS (check_row): clamp lists and wrap counts identical in float32 and float64; both wrap margins >= 0.1 rad; min |p| >= 1e-3; and
the row's own edge asserted on the restatement and the schedule, from the kernel's constants restated below.  A row whose input no longer hits its edge fails there.
(Frozen-loop rows: alpha = beta = 0 multiply the error by zero, so the loop's wrap margin and |p| do not enter and are not demanded.  K = 1 is such a row and only
such a row: one complex tap on a real stream gives an angle of two values pi apart, which no loop at the reference's constants can follow with a wrap margin.)

RUNS PER ROW: (a) ordinary passes in the row's blocks; (b) one push of the whole stream; and on the rows of PIPED — about a third, every job kind's edge rows
among them: the pilot's full window alone and in a bank of five (k575, k575_bank5), segment and tile ends (blocks_b), the matrix's full windows and the delay
longer than a segment (a289, d1500), the loop's sparse packing and rows of unequal length (bank5, uneq4), the clamp entered and left (clamp_inout), and everything
in front (front, ifc_nb, fmif) — (c) pipelined over the blocks of (a) and (d) pipelined with launch groups of 3 or 4.  (b), (c), (d) equal (a) bit for bit; (c)
and (d) never fall back to an ordinary pass and run the `ifc` role; (a) meets the bar.  Rows of a bank additionally equal, VFO by VFO and bit for bit, the same
VFO alone in its context.  (The library has no statistic that shows that two loop records shared a job: the unequal rows rely on equal chain depth — one stage each,
hence one level — and on the planner packing a level's records in order; mutations of the packing, listed in DESIGN.md 8g, are what showed that they do.)"""
import math
import os

import numpy as np
import pytest

from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_kernel_forms import BASELINE_MAX, MARGIN, _bits_equal, _lp, dist, hand_desc
from test_stereo import case_x, gold

RATE = 250e3
UNSUPPORTED = -5
# the kernel's constants (vfo_stereo_kernels.h), checked against the library's own refusals in test_constants_are_the_headers
LDS_WAVE = 832       # SDRPP_ST_LDS_WAVE (= SDRPP_FMIF_LDS_WAVE)
SEG = 1024           # SDRPP_ST_SEG
PILOT_TILE = 256     # SDRPP_ST_PILOT_TILE
MATRIX_TILE = 128    # SDRPP_ST_MATRIX_TILE
PACK = 8             # SDRPP_ST_PACK
LOOP_CHUNK = 256     # SDRPP_ST_LOOP_CHUNK
PILOT_MAX_TAPS = LDS_WAVE - PILOT_TILE                 # SDRPP_ST_PILOT_MAX_TAPS = 576
AUDIO_MAX_TAPS = LDS_WAVE // 2 - MATRIX_TILE + 1       # SDRPP_ST_AUDIO_MAX_TAPS = 289
MIN_WRAP_MARGIN, MIN_PILOT = 0.1, 1e-3
INF = float("inf")
FL_PI = np.float32(3.1415926535)


def rads(hz, rate=RATE):
    return np.float32(2.0 * math.pi * (hz / rate))  # dsp/math/hz_to_rads.h:6-8, stored as a float


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def _fir(hist, x, taps, f):
    """fir.h: out[i] = sum_k taps[k] * buf[i + k], buf = hist (K - 1 values) ++ x; k ascending, product and sum rounded on their own -> (out, new hist)"""
    K, n = len(taps), len(x)
    buf = np.concatenate([hist, x]).astype(f)
    acc = np.zeros(n, f)
    for k in range(K):
        acc = acc + (buf[k:k + n] * f(taps[k]))
    return acc, buf[len(buf) - (K - 1):] if K > 1 else buf[:0]


def fresh(cfg, f):
    """BroadcastFM::reset(): discriminator, pilot filter, loop, delay and audio filters at their initial state"""
    K, D, A = len(cfg["ptaps"]), cfg["D"], (len(cfg["ataps"]) if cfg["ataps"] is not None else 1)
    return dict(prev=f(0), m=np.zeros(max(K - 1, D), f), l=np.zeros(A - 1, f), r=np.zeros(A - 1, f), phase=f(0), freq=f(np.float32(cfg["init"])), pos=0, since=0)


def restate(y, cfg, f, state=None, stereo=True):
    """broadcast_fm.h:147-191 (stereo) / :192-212 (mono) over the IF samples y (complex64) in dtype f, from `state` (None: fresh) -> (frames [n, 2], info, state).
    cfg: ptaps float32 [K, 2], D, alpha, beta, init, lo, hi (float32 values), inv_dev (float32), ataps (float32 or None: low-pass off)."""
    n = len(y)
    st = dict(fresh(cfg, f) if state is None else state)
    K, D, at = len(cfg["ptaps"]), cfg["D"], cfg["ataps"]
    PI = f(FL_PI)
    TWO = f(2) * PI
    info = dict(clamps=[], wraps=0, margin=INF, qmargin=INF, pmin=INF)
    # quadrature.h:39-46
    ph = np.arctan2(y.imag.astype(f), y.real.astype(f)).astype(f)
    d = (ph - np.concatenate([[st["prev"]], ph[:-1]]).astype(f)).astype(f)
    if n:
        info["qmargin"] = float(np.min(np.abs(np.abs(d.astype(np.float64)) - math.pi)))
        st["prev"] = ph[-1]
    d = np.where(d > PI, d - TWO, np.where(d <= -PI, d + TWO, d)).astype(f)
    m = (d * f(np.float32(cfg["inv_dev"]))).astype(f)
    H = len(st["m"])
    mm = np.concatenate([st["m"], m]).astype(f)  # mm[H + i] = m[i]
    st["m"] = mm[len(mm) - H:]
    if not stereo:  # alFir on the discriminator's values, two copies
        v = m
        if at is not None:
            v, st["l"] = _fir(st["l"], m, at, f)
        st["pos"], st["since"] = st["pos"] + n, st["since"] + n
        return np.stack([v, v], 1), info, st
    # FIR<complex_t, complex_t> on (m + 0j): re = m * h.re - 0 * h.im, im = m * h.im + 0 * h.re
    re, _ = _fir(mm[H - (K - 1):H], m, cfg["ptaps"][:, 0], f)
    im, _ = _fir(mm[H - (K - 1):H], m, cfg["ptaps"][:, 1], f)
    ang = np.arctan2(im, re).astype(f)
    behind = max(0, K - st["since"])
    if n > behind:
        info["pmin"] = float(np.min(np.hypot(re[behind:].astype(np.float64), im[behind:].astype(np.float64))))
    # loop::PLL (pll.h:64-70, phase_control_loop.h:58-85)
    al, be, mn, mx = (f(np.float32(cfg[k])) for k in ("alpha", "beta", "lo", "hi"))
    phase, freq, pos = st["phase"], st["freq"], st["pos"]
    pl = np.empty(n, f)
    for i in range(n):
        pl[i] = phase
        e = ang[i] - phase
        info["margin"] = min(info["margin"], abs(abs(float(e)) - math.pi))
        if e > PI:
            e = e - TWO
        elif e <= -PI:
            e = e + TWO
        freq = freq + (be * e)
        if freq > mx:
            freq = mx
            info["clamps"].append(pos + i + 1)
        elif freq < mn:
            freq = mn
            info["clamps"].append(-(pos + i + 1))
        phase = phase + (freq + (al * e))
        while phase > PI:
            phase = phase - TWO
            info["wraps"] += 1
        while phase < -PI:
            phase = phase + TWO
            info["wraps"] += 1
    st["phase"], st["freq"], st["pos"], st["since"] = phase, freq, pos + n, st["since"] + n
    # delay, conj(v) twice, real part x 2, sum and difference, alFir / arFir
    md = mm[H - D:H - D + n]
    vr, vi = np.cos(pl).astype(f), (-np.sin(pl)).astype(f)
    ar, ai = (md * vr), (md * vi)
    qr = (ar * vr) - (ai * vi)
    lmr = qr * f(2)
    l, r = (md + lmr).astype(f), (md - lmr).astype(f)
    if at is not None:
        l, st["l"] = _fir(st["l"], l, at, f)
        r, st["r"] = _fir(st["r"], r, at, f)
    return np.stack([l, r], 1), info, st


def merge(infos):
    out = dict(clamps=[], wraps=0, margin=INF, qmargin=INF, pmin=INF)
    for i in infos:
        out["clamps"] += i["clamps"]
        out["wraps"] += i["wraps"]
        for k in ("margin", "qmargin", "pmin"):
            out[k] = min(out[k], i[k])
    return out


def clamp_idx(info, sign):
    """0-based sample indices where the limit `sign` (+1 upper, -1 lower) held"""
    return [abs(c) - 1 for c in info["clamps"] if (c > 0) == (sign > 0)]


def three(frames):
    """(l, r, l - r) of frames, in float64 (a float32 difference of two float32 values is rounded: the device's frames are compared as what they are)"""
    a = np.asarray(frames).astype(np.float64)
    return a[:, 0], a[:, 1], a[:, 0] - a[:, 1]


# ---- 1. the restatement against the reference's recorded frames, no device --------------------------------------------------------------------
def fixture_cfg(lowpass=True):
    from sdrplusplus_amd import capi

    z = gold()
    at = capi.design_low_pass(15000.0, 4000.0, RATE) if lowpass else None  # broadcast_fm.h:49
    return dict(ptaps=z["pilot_taps"].astype(np.float32), D=int(z["delay"]), alpha=np.float32(z["alpha"]), beta=np.float32(z["beta"]), init=rads(19000.0), lo=rads(18750.0),
                hi=rads(19250.0), inv_dev=np.float32(1.0 / (2.0 * math.pi * (75000.0 / RATE))), ataps=at)


def restate_fixture(name, f):
    """the fixture's case in the fixture's blocks with its operations: 1 setStereo(false), 2 setStereo(true), 3 reset() — each starts over"""
    z = gold()
    cfg, x = fixture_cfg(bool(z[name + "_lp"])), case_x(name)
    out, infos, st, on, pos = [], [], None, True, 0
    for b, n in enumerate(z[name + "_cut"]):
        op = int(z[name + "_ops"][b])
        if op:
            st, on = dict(fresh(cfg, f), pos=pos), (on if op == 3 else op == 2)  # (clamp indices count from the stream's start, |p| from K behind every start over)
        assert on == bool(z[name + "_stereo"][b])
        o, i, st = restate(x[pos:pos + int(n)], cfg, f, st, stereo=on)
        out.append(o)
        infos.append(i)
        pos += int(n)
    return np.concatenate(out), merge(infos)


@pytest.mark.parametrize("name", ["steady", "cuts", "nolp", "toggle"])
def test_restatement_is_the_reference_per_sample(name):
    """CPU only.  The reference's recorded frames lie within BASELINE_MAX of the float64 restatement per sample, for l, r and l - r; the float32 restatement's own
    distance lies within a factor 2 of the reference's (both are float32 evaluations of the same operations; numpy's arctan2 / cos / sin need not be glibc's bits).
    The float32 and float64 loops clamp at the same samples and wrap equally often."""
    want = gold()[name + "_audio"]
    r64, i64 = restate_fixture(name, np.float64)
    r32, i32 = restate_fixture(name, np.float32)
    assert i64["clamps"] == i32["clamps"] and i64["wraps"] == i32["wraps"] and i64["wraps"] > 100, (i64["wraps"], i32["wraps"])
    figs = [(q, dist(g, r), dist(b, r)) for q, g, b, r in zip(("l", "r", "l-r"), three(want), three(r32), three(r64))]
    for q, dg, db in figs:
        print("\n[stereo rows] fixture %s %s: reference %.3g, float32 restatement %.3g of the float64 restatement's RMS" % (name, q, dg, db), end="")
        if os.environ.get("SDRPP_STEREO_FIGURES"):
            with open(os.environ["SDRPP_STEREO_FIGURES"], "a") as fh:
                fh.write("golden %s %s %.3g %.3g\n" % (name, q, dg, db))
    for q, dg, db in figs:
        assert dg < BASELINE_MAX, (name, q, dg)
        assert 0.5 * dg <= db <= 2.0 * dg, (name, q, dg, db)
        rec = GOLDEN_FIGURES[name][q]
        assert dg <= 1.25 * rec[0] and db <= 1.25 * rec[1], (name, q, dg, db, rec)
    print()


# ---- descriptions -----------------------------------------------------------------------------------------------------------------------------
_ptaps = {}


def pilot_taps(K, rate=RATE, lo=18750.0, hi=19250.0):
    """K complex band-pass taps around the pilot from capi.design_band_pass_complex: the transition width is searched -> float32 [K, 2]"""
    from sdrplusplus_amd import capi

    key = (K, rate, lo, hi)
    if key not in _ptaps:
        a, b = 20.0, rate
        for _ in range(200):
            w = math.sqrt(a * b)
            t = capi.design_band_pass_complex(lo, hi, w, rate, True)
            if len(t) == K:
                break
            a, b = (w, b) if len(t) > K else (a, w)
        assert len(t) == K, (K, len(t))
        _ptaps[key] = np.ascontiguousarray(t.view(np.float32).reshape(-1, 2))
    return _ptaps[key]


def hand_taps(K):
    """K = 1: the tap j (frozen-loop rows only).  K = 3: a window times exp(-j w k) at the pilot's frequency — of a pilot a sin(w i) it leaves a phasor of 3 a / 2
    turning at +w and one of 1.07 a turning at -w: an angle that advances by w per sample on average, which the loop follows with an error below one radian."""
    if K == 1:
        return np.float32([[0.0, 1.0]])
    k = np.arange(K)
    t = np.exp(-1j * float(rads(19000.0)) * k)
    return np.ascontiguousarray(np.stack([t.real, t.imag], 1).astype(np.float32))


_ataps = {}


def audio_taps(A, rate=RATE):
    from sdrplusplus_amd import capi

    if (A, rate) not in _ataps:
        if A == "std":
            t = capi.design_low_pass(15000.0, 4000.0, rate)  # broadcast_fm.h:49
        elif A == 1:
            t = np.ones(1, np.float32)
        elif A == 2:
            t = np.float32([0.625, 0.375])
        else:
            t = _lp(A, 15000.0, rate)
        _ataps[(A, rate)] = np.ascontiguousarray(t, np.float32)
    return _ataps[(A, rate)]


def make_cfg(K=317, D=None, A="std", bw=25000.0, init=19000.0, lo=18750.0, hi=19250.0, frozen=False, rate=RATE, dev=75000.0, scale=1.0):
    """A description of the branch at `rate`; scale: the pilot and the loop's frequencies are those of a stream read at every scale-th sample (the unequal rows)"""
    from sdrplusplus_amd import capi

    pt = hand_taps(K) if K <= 3 else pilot_taps(K, rate / scale)
    a, b = capi.design_pll(bw / rate)
    c = dict(ptaps=pt, D=(K - 1) // 2 + 1 if D is None else D, alpha=np.float32(a), beta=np.float32(b), init=rads(init, rate / scale), lo=rads(lo, rate / scale),
             hi=rads(hi, rate / scale), inv_dev=np.float32(1.0 / (2.0 * math.pi * (dev / rate))), ataps=audio_taps(A, rate), frozen=frozen)
    if frozen:  # the phasor stays (1, 0): l = 3 m_D, r = -m_D through the audio filter
        c.update(alpha=np.float32(0), beta=np.float32(0), init=np.float32(0), lo=np.float32(-0.5), hi=np.float32(0.5))
    c["key"] = (K, c["D"], len(c["ataps"]), float(c["alpha"]), float(c["beta"]), float(c["init"]), float(c["lo"]), float(c["hi"]), float(c["inv_dev"]))
    return c


def stereo_desc_of(cfg):
    from sdrplusplus_amd import capi, radio

    s = capi.StereoDesc()
    taps = np.ascontiguousarray(cfg["ptaps"], np.float32)
    s.pilot_taps, s.pilot_ntaps, s.delay = radio._fp(taps), len(taps), cfg["D"]
    s.alpha, s.beta, s.init_freq, s.min_freq, s.max_freq, s.enabled = cfg["alpha"], cfg["beta"], cfg["init"], cfg["lo"], cfg["hi"], 1
    return s, [taps]


def job(cfg, twin=0, ifd=None, if_first=False, fmnr=False, chain=None):
    """One stereo VFO: its description, the chain in front (hand_desc arguments behind the rate; None: the identity), the IF chain and its order, its twin's index"""
    return dict(cfg=cfg, twin=twin, ifd=ifd, if_first=if_first, fmnr=fmnr, chain=chain)


def wfm_desc(j, sr, raw=False):
    from sdrplusplus_amd import radio

    d, keep, rate = hand_desc(sr, 0.0, *(j["chain"] or ()))
    if not raw:
        d.demod = radio.DEMOD_CODES["WFM"]
        d.inv_deviation = j["cfg"]["inv_dev"]
        at = j["cfg"]["ataps"]
        keep.append(at)
        d.audio_ntaps, d.audio_taps = len(at), radio._fp(at)
    return d, keep


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def signal(n, seed=1, noise=0.0005, fp=19000.0, step=None, rate=RATE, dev=75000.0, audio=1.0, spikes=()):
    """The fixture's recipe (make_stereo_golden.py): a carrier of 0.06, 75 kHz deviation, L = 1 kHz and R = 2.3 kHz, L - R on twice the pilot's phase, the pilot at 9 %,
    noise, int16 / 16384.  fp / step: the pilot's frequency, and (index, frequency) of a step; audio: the tones' level; spikes: (index, value) added."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    left, right = audio * 0.5 * np.sin(2 * np.pi * 1000.0 * t), audio * 0.3 * np.sin(2 * np.pi * 2300.0 * t + 0.4)
    fpil = np.full(n, fp)
    if step:
        fpil[step[0]:] = step[1]
    pph = 2 * np.pi * np.cumsum(fpil) / rate
    msg = 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * pph) + 0.09 * np.sin(pph)
    x = 0.06 * np.exp(1j * 2 * np.pi * np.cumsum(dev * msg) / rate) + noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    for i, v in spikes:
        x[i] += v
    q = np.rint(np.stack([x.real, x.imag], 1) * 16384.0).astype(np.int16)
    return (q.astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)


S1 = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 187]  # 3 196: every tile and segment end but the two-segment block
S2 = [64, 1024, 2049, 1, 863]                         # 4 001: a whole segment, two segments and one sample
S3 = [60, 740, 1, 650, 449, 600, 500]                # 3 000: no block reaches a segment
ALL_BLOCKS = {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049}
assert ALL_BLOCKS <= set(S1) | set(S2)


class Row:
    """build() -> dict(x, blocks, jobs [job], twins [twin's job], sr, edge (callable(case, infos64, counts) with the row's own CPU assertions), alone (every VFO also
    runs alone in its context and must give the same bits)); `why`: the edge the row places."""

    def __init__(self, rid, why, build, identity=True, group=3):
        self.id, self.why, self.build, self.identity, self.group = rid, why, build, identity, group


def _first_short(case):
    for j in case["jobs"]:
        K, D = len(j["cfg"]["ptaps"]), j["cfg"]["D"]
        assert (case["first_if"] < K or K <= 3) and (case["first_if"] < D or D <= 2), (case["first_if"], K, D)  # (no block is shorter than one sample)


def _simple(cfg_kw, blocks, edge=None, sig_kw=None, nv=1):
    def build():
        cfg = make_cfg(**cfg_kw)
        return dict(x=signal(sum(blocks), **(sig_kw or {})), blocks=blocks, jobs=[job(cfg) for _ in range(nv)], twins=[job(cfg)], edge=edge, alone=nv > 1)
    return build


def _edge_blocks(want):
    def edge(case, infos, counts):
        assert set(want) <= set(case["blocks"]), case["blocks"]
        # tiles of every kind: a pilot tile with a fourth group of 1 .. 63 outputs, a matrix tile with a second group of 1 .. 63, both full, both of one sample
        pt = {min(PILOT_TILE, min(SEG, n - s) - t) for n in case["blocks"] for s in range(0, n, SEG) for t in range(0, min(SEG, n - s), PILOT_TILE)}
        mt = {min(MATRIX_TILE, min(SEG, n - s) - t) for n in case["blocks"] for s in range(0, n, SEG) for t in range(0, min(SEG, n - s), MATRIX_TILE)}
        assert {1, PILOT_TILE} <= pt and {1, MATRIX_TILE} <= mt, (pt, mt)
        if 255 in want:
            assert {63, 64, 65, 255} <= pt and any(193 <= c <= 255 for c in pt) and {63, 64, 65, 127} <= mt, (pt, mt)
    return edge


def _edge_k575(case, infos, counts):
    K = len(case["jobs"][0]["cfg"]["ptaps"])
    assert K == PILOT_MAX_TAPS - 1 and PILOT_TILE + K == LDS_WAVE - 1  # phases 0 .. tile + K - 1: 831 of the wavefront's 832 floats
    assert any(n >= PILOT_TILE for n in case["blocks"])  # a full tile: the whole window is written
    if len(case["jobs"]) > 1:
        assert len(case["jobs"]) >= 5  # five pilot jobs per level: the four wavefronts of a workgroup all hold full windows next to each other


def _edge_a(A):
    def edge(case, infos, counts):
        assert len(case["jobs"][0]["cfg"]["ataps"]) == A
        if A == AUDIO_MAX_TAPS:
            assert MATRIX_TILE + A - 1 == LDS_WAVE // 2 and any(n >= MATRIX_TILE for n in case["blocks"])  # both halves of the share are full
    return edge


def _edge_d(D):
    def edge(case, infos, counts):
        c = case["jobs"][0]["cfg"]
        assert c["D"] == D
        if D == 160:
            assert D != (len(c["ptaps"]) - 1) // 2 + 1
        if D == 1500:
            assert D > SEG and D > max(case["blocks"])
    return edge


def _edge_frozen(case, infos, counts):
    for j, i in zip(case["jobs"], infos):
        assert j["cfg"]["frozen"] and i["clamps"] == [] and i["wraps"] == 0


def _edge_clamp(sign, hold=1000, leave=False):
    def edge(case, infos, counts):
        K = len(case["jobs"][0]["cfg"]["ptaps"])
        idx = clamp_idx(infos[0], sign)
        behind = [i for i in idx if i >= K]
        assert len(behind) >= hold, ("the clamp is not held", sign, len(behind))
        if leave:  # entered, held, and left for good inside a block, not at its start; the loop is free behind it
            last, n = max(idx), len(case["x"])
            starts = set(np.cumsum([0] + case["blocks"]).tolist())
            assert leave[0] < last + 1 < leave[1] and (last + 1) not in starts and n - last > 500, (last, leave)
            assert not [i for i in clamp_idx(infos[0], -sign) if i > last]
    return edge


def _edge_init_min(case, infos, counts):
    c = case["jobs"][0]["cfg"]
    lower = clamp_idx(infos[0], -1)
    assert c["init"] == c["lo"] and c["D"] == 1 and len(lower) >= 10 and min(lower) < 8, lower[:20]


# the loop job's packing: four descriptions — two pilot lengths, two alpha / beta pairs, two limit sets — dealt round the bank
def bank_cfgs():
    return [make_cfg(), make_cfg(K=161, bw=40000.0, lo=18900.0, hi=19100.0), make_cfg(bw=40000.0), make_cfg(K=161, lo=18900.0, hi=19100.0)]


def _bank(nv):
    def build():
        cfgs = bank_cfgs()
        x = signal(sum(S3), seed=5)

        def edge(case, infos, counts):
            C = LOOP_CHUNK // nv
            empty = [e for e in range(LOOP_CHUNK) if e >= nv * C]  # elements of a lane's four that belong to no row
            assert (C, C | 1) == {2: (128, 129), 4: (64, 65), 5: (51, 51), 6: (42, 43), 7: (36, 37), 8: (32, 33)}[nv]
            assert nv <= PACK and bool(empty) == (nv in (5, 6, 7)) and max(case["blocks"]) > 2 * C  # (one job: at most SDRPP_ST_PACK records)
        return dict(x=x, blocks=S3, jobs=[job(cfgs[k % 4]) for k in range(nv)], twins=[job(cfgs[0])], edge=edge, alone=True, alone_key="bank")
    return build


def _uneq(nv, short_first=False):
    """VFO k reads every 2nd (even k; with short_first odd k) or 4th input sample through a one-tap stage: one level, one loop job, rows of n and n / 2.  The input is the fixture's
    recipe at the /2 VFOs' rate with 30 kHz deviation (at every 4th sample a phase step is twice as large, and 75 kHz would carry it past pi), the other samples
    of the input are something else."""
    def build():
        C = LOOP_CHUNK // nv
        blocks = [1, 2, 3, 2, 160, 4 * C, 1, 1, 1, 1, 640, 2048, 3, 5, 1200, 4 * C, 2000]
        blocks.append(12000 - sum(blocks))
        n = sum(blocks)
        s = signal(n // 2, seed=6, dev=30000.0)
        x = np.empty(n, np.complex64)
        x[0::2], x[1::2] = s, np.roll(s, 5) * np.complex64(-2.0 + 1.0j) + np.complex64(0.125)
        c2 = [make_cfg(dev=30000.0), make_cfg(dev=30000.0, bw=40000.0, lo=18900.0, hi=19100.0)]
        c4 = [make_cfg(K=161, dev=15000.0, scale=2.0), make_cfg(K=161, dev=15000.0, scale=2.0, bw=40000.0)]
        one = np.ones(1, np.float32)
        jobs = []
        is_short = lambda k: (k % 2 == 1) != short_first  # noqa: E731
        for k in range(nv):
            jobs.append(job((c4 if is_short(k) else c2)[(k // 2) % 2], twin=int(is_short(k)), chain=([(4 if is_short(k) else 2, one)],)))
        twins = [job(None, chain=([(2, one)],)), job(None, chain=([(4, one)],))]

        def edge(case, infos, counts):
            long_, short = np.asarray(counts[0]), np.asarray(counts[1])
            assert sum(long_) == n // 2 and sum(short) == n // 4
            assert np.any((short == 0) & (long_ > 0)) and np.any((short == 0) & (long_ == 0))  # pushes that give a row, or every row, no record
            assert np.any((short > 0) & (short < long_) & (long_ <= C))  # the short row ends inside the long row's first chunk
            assert np.any((short == C) & (long_ == 2 * C))  # the short row ends exactly at a chunk end
            assert np.any(long_ > 3 * C)  # several chunks, the short row out of them before the long one
            assert is_short(0) == short_first  # (the job's first record is the short row: a walk sized by it would stop early)
            for t, dec in enumerate((2, 4)):
                _bits_equal(case["ifs"][t].view(np.float32), np.ascontiguousarray(case["x"][::dec]).view(np.float32), "one-tap stage: IF = every %d-th sample" % dec)
        return dict(x=x, blocks=blocks, jobs=jobs, twins=twins, edge=edge, alone=True, sr=2 * RATE)
    return build


def _front():
    """750 kS/s -> /2 (7 taps) -> 2/3 polyphase (a 3/2 decimating resampler, 8 taps) -> channel filter (5 taps) -> 250 kS/s.  Short triangles of positive taps: from
    a zeroed line every output is a positive mixture of the first inputs, so the start-up has phase steps like the stream's (a long low-pass starts with taps of
    1e-12 and both signs, and its first outputs step by nearly pi: ill-conditioned for any discriminator, and for nothing that is checked here)."""
    def build():
        sr = 3 * RATE
        tri = lambda n: np.bartlett(n + 2)[1:-1].astype(np.float32) / np.float32(np.bartlett(n + 2).sum())  # noqa: E731
        chain = ([(2, tri(7))], 2, 3, tri(8) * np.float32(2), tri(5))
        blocks = [90, 3072, 1, 7, 2999, 768, 3000, 1500, 563]
        cfg = make_cfg()
        return dict(x=signal(sum(blocks), seed=7, rate=sr, audio=0.5), blocks=blocks, jobs=[job(cfg, chain=chain)], twins=[job(None, chain=chain)], sr=sr,
                    edge=lambda case, infos, counts: _first_short(dict(case, first_if=counts[0][0])))
    return build


def _ifc(first, nb=False, fmnr=False):
    def build():
        from sdrplusplus_amd import radio

        blocks = [120, 1024, 700, 1, 1155]
        spikes = [(i, 0.9 + 0.3j) for i in (500, 1500, 1501, 2400)] if nb else ()
        ifd = radio.if_desc(RATE, nb=nb, nb_level=10.0, squelch=-150.0)  # (the squelch enabled and open)
        cfg = make_cfg()

        def edge(case, infos, counts):
            _first_short(dict(case, first_if=counts[0][0]))
            same = np.array_equal(case["ifs"][0].view(np.uint32), case["x"].view(np.uint32))
            assert same == (not (nb or fmnr)), "the IF chain must change the stream exactly where a block of it is switched on"
        return dict(x=signal(sum(blocks), seed=9 if fmnr else 8, spikes=spikes, audio=0.2 if fmnr else 1.0), blocks=blocks, jobs=[job(cfg, ifd=ifd, if_first=first, fmnr=fmnr)], twins=[job(None, ifd=ifd, fmnr=fmnr)], edge=edge)
    return build


N_CLAMP, STEP = 6000, 3000
CLAMP_BLOCKS = [100, 1400, 1000, 1100, 1400, 1000]  # (the step at 3 000 and everything within 500 samples behind it lie inside the fifth block)

ROWS = [
    # ---- pilot geometry ----
    Row("k1_frozen", "K = 1 pilot tap, D = 1, frozen loop (one tap gives no angle a loop can follow): window of tile + 1 phases", _simple(dict(K=1, D=1, A=1, frozen=True), S1, _edge_frozen)),
    Row("k3", "K = 3 hand-made pilot taps, D = 2, the tones at 2 % so that three taps see the pilot", _simple(dict(K=3, A=1), S1, None, dict(audio=0.02))),
    Row("k317", "K = 317, the reference's geometry, in blocks that end on every tile and segment edge; the first block shorter than K and D", _simple(dict(), S1, _edge_blocks(ALL_BLOCKS - {1024, 2049}))),
    Row("k575", "K = 575 with D = 288: the pilot window takes 831 of the wavefront's 832 LDS floats", _simple(dict(K=575), S2, _edge_k575, dict(seed=2))),
    Row("k575_bank5", "five VFOs of K = 575: the four wavefronts of a workgroup hold full windows next to each other", _simple(dict(K=575), S2, _edge_k575, dict(seed=2), nv=5), group=4),
    # ---- block lengths ----
    Row("blocks_b", "blocks of 64, 1024, 2049, 1, 863: a whole segment, two segments and a sample; the first block shorter than K and D", _simple(dict(), S2, _edge_blocks({64, 1024, 2049, 1}), dict(seed=3)), group=4),
    # ---- matrix geometry ----
    Row("a1", "one audio tap: the matrix window is the tile", _simple(dict(A=1), S3, _edge_a(1))),
    Row("a2", "two audio taps", _simple(dict(A=2), S3, _edge_a(2))),
    Row("a129", "129 audio taps: the window is two tiles long", _simple(dict(A=129), S1, _edge_a(129))),
    Row("a289", "289 audio taps, the most: both halves of the wavefront's share are full", _simple(dict(A=AUDIO_MAX_TAPS), S2, _edge_a(AUDIO_MAX_TAPS), dict(seed=4))),
    Row("d1", "a delay of one sample", _simple(dict(D=1), S1, _edge_d(1))),
    Row("d160", "delay 160 behind 317 pilot taps: not the filter's centre", _simple(dict(D=160), S1, _edge_d(160))),
    Row("d1500", "delay 1 500: longer than a segment and than every block", _simple(dict(D=1500), S3, _edge_d(1500)), group=4),
    # ---- frozen loop: discriminator, delay and audio filter alone ----
    Row("frozen_k317_a129", "alpha = beta = 0, phase 0: l = 3 m_D, r = -m_D through 129 audio taps", _simple(dict(A=129, frozen=True), S1, _edge_frozen)),
    Row("frozen_k575_a289", "the frozen loop at both maxima", _simple(dict(K=575, A=AUDIO_MAX_TAPS, frozen=True), S2, _edge_frozen)),
    # ---- the frequency clamp ----
    Row("clamp_hi", "pilot at 19 300 Hz: the upper limit held in steady state", _simple(dict(), CLAMP_BLOCKS, _edge_clamp(+1, 5000), dict(fp=19300.0))),
    Row("clamp_lo", "pilot at 18 700 Hz: the lower limit held in steady state", _simple(dict(), CLAMP_BLOCKS, _edge_clamp(-1, 5000), dict(fp=18700.0))),
    Row("clamp_inout", "pilot at 19 300 Hz, 19 100 Hz from sample 3 000: the clamp is left inside a block", _simple(dict(), CLAMP_BLOCKS, _edge_clamp(+1, 2000, leave=(STEP, STEP + 500)), dict(fp=19300.0, step=(STEP, 19100.0)))),
    Row("clamp_init_min", "init_freq = min_freq with D = 1: the lower limit in the first samples, seen at once (behind a longer delay the first frames are zeros)", _simple(dict(init=18750.0, D=1), S1, _edge_init_min)),
    Row("clamp_narrow", "limits 19 005 +- 10 Hz, pilot at 19 020 Hz: a description's own limits, held", _simple(dict(lo=18995.0, hi=19015.0, init=19005.0), CLAMP_BLOCKS[:3], _edge_clamp(+1, 1000), dict(fp=19020.0))),
    # ---- the loop job's packing ----
    Row("bank2", "two loops in a job: chunk 128, pitch 129", _bank(2)),
    Row("bank4", "four: chunk 64, pitch 65", _bank(4)),
    Row("bank5", "five: chunk 51 (odd: pitch 51), 255 of a lane's 256 elements belong to a row", _bank(5), group=4),
    Row("bank6", "six: chunk 42, pitch 43, 252 elements", _bank(6)),
    Row("bank7", "seven: chunk 36, pitch 37, 252 elements", _bank(7)),
    Row("bank8", "eight, a full job: chunk 32, pitch 33", _bank(8)),
    Row("uneq2", "two loops of unequal length in one job (/2 and /4 one-tap stages): rows without a record, a row that ends inside the other's first chunk and at a chunk end", _uneq(2), identity=False),
    Row("uneq4", "four loops of two lengths in one job, the SHORT row first (the longest row is not the job's first)", _uneq(4, short_first=True), identity=False, group=4),
    # ---- what sits in front ----
    Row("front", "behind a decimator, a 3/2 resampler and a channel filter; the first block shorter than K", _front(), identity=False),
    Row("ifc_after", "behind the IF chain (squelch open, blanker off) attached AFTER the branch", _ifc(False)),
    Row("ifc_before", "behind the IF chain attached BEFORE the branch", _ifc(True)),
    Row("ifc_nb", "behind the IF chain with the noise blanker on, over spikes: the IF is what the chain delivered", _ifc(True, nb=True), identity=False),
    Row("fmif", "behind FMIF (32 bins), the IF chain's last block", _ifc(True, fmnr=True), identity=False),
]
PIPED = ("k575", "k575_bank5", "blocks_b", "a289", "d1500", "bank5", "uneq4", "clamp_inout", "front", "ifc_nb", "fmif")

# The reference's recorded frames and the float32 restatement against the float64 restatement per fixture case: {case: {quantity: (reference, float32 restatement)}}
GOLDEN_FIGURES = {
    "steady": {"l": (1.21e-06, 1.18e-06), "r": (1.63e-06, 1.89e-06), "l-r": (1.36e-06, 1.57e-06)},
    "cuts": {"l": (1.15e-06, 1.35e-06), "r": (1.73e-06, 1.88e-06), "l-r": (1.47e-06, 1.41e-06)},
    "nolp": {"l": (1.45e-06, 2.31e-06), "r": (2.29e-06, 2.73e-06), "l-r": (1.76e-06, 2.33e-06)},
    "toggle": {"l": (2.02e-06, 2.31e-06), "r": (1.92e-06, 1.77e-06), "l-r": (2.04e-06, 2.24e-06)},
}

# float32 sequential baselines per row, job and quantity (l, r, l - r), measured by this file's own CPU run of the restatement: {row: [per job ((emulator leg), (device
# leg))]}.  Identity rows' IF is the input on both legs: one figure.  A job's bar is MARGIN x the baseline of the run, which may not exceed 1.25 x the figure here.
BASELINES = {
    "k1_frozen": [((1.32e-06, 1.37e-06, 1.33e-06), (1.32e-06, 1.37e-06, 1.33e-06))],
    "k3": [((1.83e-06, 4.69e-06, 1.94e-06), (1.83e-06, 4.69e-06, 1.94e-06))],
    "k317": [((1.08e-06, 1.56e-06, 1.49e-06), (1.08e-06, 1.56e-06, 1.49e-06))],
    "k575": [((2.32e-06, 1.42e-06, 1.64e-06), (2.32e-06, 1.42e-06, 1.64e-06))],
    "k575_bank5": [((2.32e-06, 1.42e-06, 1.64e-06), (2.32e-06, 1.42e-06, 1.64e-06))],
    "blocks_b": [((1.04e-06, 1.67e-06, 1.59e-06), (1.04e-06, 1.67e-06, 1.59e-06))],
    "a1": [((1.78e-06, 2.94e-06, 1.9e-06), (1.78e-06, 2.94e-06, 1.9e-06))],
    "a2": [((1.32e-06, 2.01e-06, 1.55e-06), (1.32e-06, 2.01e-06, 1.55e-06))],
    "a129": [((8.88e-07, 1.17e-06, 1.09e-06), (8.88e-07, 1.17e-06, 1.09e-06))],
    "a289": [((1.16e-06, 1.8e-06, 1.31e-06), (1.16e-06, 1.8e-06, 1.31e-06))],
    "d1": [((1.2e-06, 1.64e-06, 1.42e-06), (1.2e-06, 1.64e-06, 1.42e-06))],
    "d160": [((1.77e-06, 2.09e-06, 2.76e-06), (1.77e-06, 2.09e-06, 2.76e-06))],
    "d1500": [((1.77e-06, 2.92e-06, 4.36e-06), (1.77e-06, 2.92e-06, 4.36e-06))],
    "frozen_k317_a129": [((1.16e-06, 1.24e-06, 1e-06), (1.16e-06, 1.24e-06, 1e-06))],
    "frozen_k575_a289": [((2.21e-06, 1.95e-06, 1.61e-06), (2.21e-06, 1.95e-06, 1.61e-06))],
    "clamp_hi": [((1.1e-06, 1.63e-06, 1.34e-06), (1.1e-06, 1.63e-06, 1.34e-06))],
    "clamp_lo": [((1.11e-06, 1.72e-06, 1.32e-06), (1.11e-06, 1.72e-06, 1.32e-06))],
    "clamp_inout": [((1.13e-06, 2.17e-06, 1.34e-06), (1.13e-06, 2.17e-06, 1.34e-06))],
    "clamp_init_min": [((1.2e-06, 1.64e-06, 1.42e-06), (1.2e-06, 1.64e-06, 1.42e-06))],
    "clamp_narrow": [((1.39e-06, 1.69e-06, 1.35e-06), (1.39e-06, 1.69e-06, 1.35e-06))],
    "bank2": [((1.15e-06, 1.89e-06, 1.16e-06), (1.15e-06, 1.89e-06, 1.16e-06)), ((1.64e-06, 1.97e-06, 2.72e-06), (1.64e-06, 1.97e-06, 2.72e-06))],
    "bank4": [((1.15e-06, 1.89e-06, 1.16e-06), (1.15e-06, 1.89e-06, 1.16e-06)), ((1.64e-06, 1.97e-06, 2.72e-06), (1.64e-06, 1.97e-06, 2.72e-06)), ((1.13e-06, 1.86e-06, 1.38e-06), (1.13e-06, 1.86e-06, 1.38e-06)), ((1.23e-06, 1.74e-06, 2.19e-06), (1.23e-06, 1.74e-06, 2.19e-06))],
    "bank5": [((1.15e-06, 1.89e-06, 1.16e-06), (1.15e-06, 1.89e-06, 1.16e-06)), ((1.64e-06, 1.97e-06, 2.72e-06), (1.64e-06, 1.97e-06, 2.72e-06)), ((1.13e-06, 1.86e-06, 1.38e-06), (1.13e-06, 1.86e-06, 1.38e-06)), ((1.23e-06, 1.74e-06, 2.19e-06), (1.23e-06, 1.74e-06, 2.19e-06))],
    "bank6": [((1.15e-06, 1.89e-06, 1.16e-06), (1.15e-06, 1.89e-06, 1.16e-06)), ((1.64e-06, 1.97e-06, 2.72e-06), (1.64e-06, 1.97e-06, 2.72e-06)), ((1.13e-06, 1.86e-06, 1.38e-06), (1.13e-06, 1.86e-06, 1.38e-06)), ((1.23e-06, 1.74e-06, 2.19e-06), (1.23e-06, 1.74e-06, 2.19e-06))],
    "bank7": [((1.15e-06, 1.89e-06, 1.16e-06), (1.15e-06, 1.89e-06, 1.16e-06)), ((1.64e-06, 1.97e-06, 2.72e-06), (1.64e-06, 1.97e-06, 2.72e-06)), ((1.13e-06, 1.86e-06, 1.38e-06), (1.13e-06, 1.86e-06, 1.38e-06)), ((1.23e-06, 1.74e-06, 2.19e-06), (1.23e-06, 1.74e-06, 2.19e-06))],
    "bank8": [((1.15e-06, 1.89e-06, 1.16e-06), (1.15e-06, 1.89e-06, 1.16e-06)), ((1.64e-06, 1.97e-06, 2.72e-06), (1.64e-06, 1.97e-06, 2.72e-06)), ((1.13e-06, 1.86e-06, 1.38e-06), (1.13e-06, 1.86e-06, 1.38e-06)), ((1.23e-06, 1.74e-06, 2.19e-06), (1.23e-06, 1.74e-06, 2.19e-06))],
    "uneq2": [((1.42e-06, 2.05e-06, 2.03e-06), (1.42e-06, 2.05e-06, 2.03e-06)), ((1.92e-06, 1.31e-06, 1.83e-06), (1.92e-06, 1.31e-06, 1.83e-06))],
    "uneq4": [((1.92e-06, 1.31e-06, 1.83e-06), (1.92e-06, 1.31e-06, 1.83e-06)), ((1.42e-06, 2.05e-06, 2.03e-06), (1.42e-06, 2.05e-06, 2.03e-06)), ((1.66e-06, 1.16e-06, 1.6e-06), (1.66e-06, 1.16e-06, 1.6e-06)), ((1.59e-06, 2.08e-06, 2.14e-06), (1.59e-06, 2.08e-06, 2.14e-06))],
    "front": [((1.59e-06, 2.45e-06, 3.86e-06), (1.59e-06, 2.45e-06, 3.86e-06))],
    "ifc_after": [((1.31e-06, 1.94e-06, 1.59e-06), (1.31e-06, 1.94e-06, 1.59e-06))],
    "ifc_before": [((1.31e-06, 1.94e-06, 1.59e-06), (1.31e-06, 1.94e-06, 1.59e-06))],
    "ifc_nb": [((1.31e-06, 1.94e-06, 1.59e-06), (1.31e-06, 1.94e-06, 1.59e-06))],
    "fmif": [((3.91e-06, 8.12e-06, 1.87e-05), (3.91e-06, 8.12e-06, 1.87e-05))],
}


# ---- running ----------------------------------------------------------------------------------------------------------------------------------
_cases = {}


def prepare(row):
    if row.id not in _cases:
        case = row.build()
        case.setdefault("sr", RATE)
        case.setdefault("alone", False)
        assert sum(case["blocks"]) == len(case["x"])
        _cases[row.id] = case
    return dict(_cases[row.id])


LAG = 16  # results are taken this many pushes behind (SDRPP_RESULT_SLOTS is 24)


def run(case, pushes, pipelined=False, group=0, only=None):
    """-> dict(audio=[per job [n, 2]], ifs=[per twin complex64], counts=[per twin [IF samples per push]], forms, stats, groups); only: that job alone"""
    from sdrplusplus_amd import capi

    mp = max(sum(pushes[i:i + max(1, group)]) for i in range(len(pushes)))
    ctx = capi.Context(0, max_push=mp)
    jobs = case["jobs"] if only is None else [case["jobs"][only]]
    vids, tids = [], []
    for j in jobs:
        d, keep = wfm_desc(j, case["sr"])
        vid = ctx.vfo_add(d, keep)
        sd, skeep = stereo_desc_of(j["cfg"])
        if j["ifd"] is not None and j["if_first"]:
            ctx.vfo_set_if(vid, j["ifd"])
        if j["fmnr"] and j["if_first"]:
            ctx.vfo_set_fmnr(vid, True, 32)
        ctx.vfo_set_stereo(vid, sd, skeep)
        if j["ifd"] is not None and not j["if_first"]:
            ctx.vfo_set_if(vid, j["ifd"])
        vids.append(vid)
    for t in case["twins"]:
        d, keep = wfm_desc(t, case["sr"], raw=True)
        tid = ctx.vfo_add(d, keep)
        if t["ifd"] is not None:
            ctx.vfo_set_if(tid, t["ifd"])
        if t["fmnr"]:
            ctx.vfo_set_fmnr(tid, True, 32)
        tids.append(tid)
    if pipelined:
        ctx.set_pipelined(True, 1)
        if group:
            ctx.set_pipeline_group(group)
    audio, ifs = [[] for _ in vids], [[] for _ in tids]
    as_if = lambda a: np.ascontiguousarray(a).copy().view(np.complex64).reshape(-1)  # noqa: E731

    def take(tk):
        got = ctx.result_wait(tk)
        for k, v in enumerate(vids):
            audio[k].append(got["vfo"][v].copy())
        for k, t in enumerate(tids):
            ifs[k].append(as_if(got["vfo"][t]))
        ctx.result_release(tk)

    pos = 0
    for k, c in enumerate(pushes, start=1):
        ctx.push(case["x"][pos:pos + c])
        pos += c
        if pipelined:
            if k > LAG:
                take(k - LAG)
        else:
            for q, v in enumerate(vids):
                audio[q].append(ctx.vfo_read(v).copy())
            for q, t in enumerate(tids):
                ifs[q].append(as_if(ctx.vfo_read(t)))
    if pipelined:
        for k in range(max(1, len(pushes) - LAG + 1), len(pushes) + 1):
            take(k)
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    gs = ctx.pipeline_group_stats() if (pipelined and group) else None
    if pipelined:
        ctx.set_pipelined(False)
    ctx.close()
    return dict(audio=[np.concatenate(a) for a in audio], ifs=[np.concatenate(q) for q in ifs], counts=[[len(q) for q in qq] for qq in ifs], forms=forms, stats=st, groups=gs)


_restated = {}


def restated(row, case, j, y, leg):
    """(ref64, info64, base32, info32) of job j over its IF y; computed once per row, description and leg and left unchanged"""
    cfg = case["jobs"][j]["cfg"]
    key = (case.get("alone_key", row.id), cfg["key"], case["jobs"][j]["twin"], "cpu" if row.identity else leg)
    if key not in _restated:
        o64, i64, _ = restate(y, cfg, np.float64)
        o32, i32, _ = restate(y, cfg, np.float32)
        for a in (o64, o32):
            a.setflags(write=False)
        _restated[key] = (o64, i64, o32, i32)
    return _restated[key]


def check_row(row, case, leg):
    """The CPU check of a row, before its outputs are looked at -> [(ref64, info64, base32, info32)] per job"""
    out = []
    for j, jb in enumerate(case["jobs"]):
        o64, i64, o32, i32 = restated(row, case, j, case["ifs"][jb["twin"]], leg)
        assert i32["clamps"] == i64["clamps"], (row.id, j, "float32 and float64 loops clamp at different samples", len(i32["clamps"]), len(i64["clamps"]))
        assert i32["wraps"] == i64["wraps"], (row.id, j, "float32 and float64 loops wrap differently", i32["wraps"], i64["wraps"])
        assert i64["qmargin"] >= MIN_WRAP_MARGIN and i32["qmargin"] >= MIN_WRAP_MARGIN, (row.id, j, "a phase step comes too close to pi", i64["qmargin"])
        if not jb["cfg"]["frozen"]:
            assert i64["margin"] >= MIN_WRAP_MARGIN and i32["margin"] >= MIN_WRAP_MARGIN, (row.id, j, "the loop's error comes too close to pi", i64["margin"])
            assert i64["pmin"] >= MIN_PILOT, (row.id, j, "the pilot filter's output comes too close to zero", i64["pmin"])
            assert i64["wraps"] > len(o64) // 20, (row.id, j, i64["wraps"])
        out.append((o64, i64, o32, i32))
    if case.get("edge"):
        case["edge"](case, [o[1] for o in out], case["counts"])
    return out


_alone = {}


def alone(backend, row, case, j):
    """job j alone in its context, over the row's blocks -> frames; one run per backend and description, shared"""
    jb = case["jobs"][j]
    key = (backend, case.get("alone_key", row.id), jb["cfg"]["key"], jb["twin"])
    if key not in _alone:
        one = dict(case, twins=[case["twins"][jb["twin"]]], jobs=[dict(jb, twin=0)])
        _alone[key] = run(one, case["blocks"])["audio"][0]
        _alone[key].setflags(write=False)
    return _alone[key]


def _same(a, b, what):
    for j, (p, q) in enumerate(zip(a["audio"], b["audio"])):
        _bits_equal(p, q, "%s, job %d audio" % (what, j))
    for j, (p, q) in enumerate(zip(a["ifs"], b["ifs"])):
        _bits_equal(p.view(np.float32), q.view(np.float32), "%s, twin %d IF" % (what, j))


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_stereo_sample_by_sample(backend, row):
    case = prepare(row)
    x = case["x"]
    if row.identity:  # the row's edge on the CPU before anything runs on a device: the IF of an identity chain is the input
        case["ifs"], case["counts"] = [x] * len(case["twins"]), [case["blocks"]] * len(case["twins"])
        _first_short(dict(case, first_if=case["blocks"][0]))
        checked = check_row(row, case, backend)
    a = run(case, case["blocks"])
    if row.identity:
        for t in a["ifs"]:
            _bits_equal(t.view(np.float32), x.view(np.float32), "%s: the identity chain's IF is the input" % row.id)
    else:
        case["ifs"], case["counts"] = a["ifs"], a["counts"]
        checked = check_row(row, case, backend)
    for j, jb in enumerate(case["jobs"]):
        assert len(a["audio"][j]) == len(a["ifs"][jb["twin"]]), (row.id, j)
    assert a["forms"].get("ifc", 0) > 0, a["forms"]
    b = run(case, [len(x)])
    _same(a, b, "%s: one push vs the row's blocks" % row.id)
    if row.id in PIPED:
        c = run(case, case["blocks"], pipelined=True)
        d = run(case, case["blocks"], pipelined=True, group=row.group)
        _same(a, c, "%s: pipelined vs ordinary passes" % row.id)
        _same(a, d, "%s: launch groups of %d vs ordinary passes" % (row.id, row.group))
        for r, what in ((c, "pipelined"), (d, "grouped")):
            st = r["stats"]
            assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(case["blocks"]) and not r["forms"], (row.id, what, st, r["forms"])
            assert st["roles"].get("ifc", 0) > 0, (row.id, what, st["roles"])
        if any(jb["chain"] and jb["chain"][0] for jb in case["jobs"]):  # (a chain without a decimator stage goes out one push per launch)
            assert d["groups"]["multi_groups"] >= 2 and d["groups"]["largest"] == row.group, d["groups"]
    if case["alone"]:
        for j in range(len(case["jobs"])):
            _bits_equal(a["audio"][j], alone(backend, row, case, j), "%s: VFO %d in the bank vs alone in its context" % (row.id, j))
    figures, seen = [], {}
    for j, jb in enumerate(case["jobs"]):
        o64, i64, o32, i32 = checked[j]
        k = (jb["cfg"]["key"], jb["twin"])
        if k in seen:  # (a copy of a VFO of this bank, bit-identical to it by the comparison with the VFO alone)
            _bits_equal(a["audio"][j], a["audio"][seen[k]], "%s: VFO %d vs its copy %d" % (row.id, j, seen[k]))
            continue
        seen[k] = j
        fig = []
        for q, g, b32, r in zip(("l", "r", "l-r"), three(a["audio"][j]), three(o32), three(o64)):
            base, e = dist(b32, r), dist(g, r)
            fig.append((base, e))
            print("\n[stereo rows %s job %d %s] %s per-sample max-abs / rms: baseline %.3g library %.3g (bar %.3g) | clamps %d wraps %d margins %.3g %.3g |p| %.3g" % (
                row.id, j, q, backend, base, e, MARGIN * base, len(i64["clamps"]), i64["wraps"], i64["margin"], i64["qmargin"], i64["pmin"]), end="")
        figures.append((j, fig))
    print()
    if os.environ.get("SDRPP_STEREO_FIGURES"):  # (refilling BASELINES: one line per row and leg, baseline:library per job and quantity, appended to the named file)
        with open(os.environ["SDRPP_STEREO_FIGURES"], "a") as fh:
            fh.write("%s %s %s\n" % (row.id, backend, " | ".join(" ".join("%.3g:%.3g" % be for be in fig) for _, fig in figures)))
    for n, (j, fig) in enumerate(figures):
        for q, (base, e) in zip(("l", "r", "l-r"), fig):
            assert base < BASELINE_MAX, ("ill-conditioned input: float32 sequential baseline", row.id, j, q, base)
            at = int(np.argmax(np.abs(three(a["audio"][j])[("l", "r", "l-r").index(q)] - three(checked[j][0])[("l", "r", "l-r").index(q)])))
            assert e <= MARGIN * base, (row.id, "job %d %s: %.3g against a float32 sequential baseline of %.3g" % (j, q, e, base), "worst frame", at)
            rec = BASELINES[row.id][n][backend == "gpu"][("l", "r", "l-r").index(q)]
            assert base <= 1.25 * rec, ("the float32 sequential baseline moved up: the bar may not loosen unseen", row.id, j, q, backend, base, rec)


def test_every_row_states_its_edge_and_the_table_is_complete():
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids) and all(len(r.why) > 8 for r in ROWS) and set(PIPED) <= set(ids)
    assert sorted(BASELINES) == sorted(ids), (set(ids) ^ set(BASELINES))
    assert len(ROWS) // 3 <= len(PIPED)
    for r in ROWS:
        case = prepare(r)
        nif = len(case["x"]) * RATE / case["sr"] if r.id != "front" else len(case["x"]) // 3
        assert nif <= 6000 + 66, (r.id, nif)
        distinct = len({(j["cfg"]["key"], j["twin"]) for j in case["jobs"]})
        assert len(BASELINES[r.id]) == distinct, (r.id, len(BASELINES[r.id]), distinct)


def test_constants_are_the_headers(backend):
    """SDRPP_ST_PILOT_MAX_TAPS and SDRPP_ST_AUDIO_MAX_TAPS as the library enforces them: 575 pilot taps (the largest odd count) and 289 audio taps are taken, 577 and
    290 refused as unsupported.  The tile, segment, pack and chunk sizes have no such surface: they are restated above under their macros' names."""
    import ctypes as C

    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=4096)
    call = lambda v, d: ctx.L.sdrpp_vfo_set_stereo(ctx.h, v, C.byref(d))  # noqa: E731
    for A, want in ((AUDIO_MAX_TAPS, 0), (AUDIO_MAX_TAPS + 1, UNSUPPORTED)):
        cfg = dict(make_cfg(K=PILOT_MAX_TAPS - 1), ataps=np.ones(A, np.float32) / np.float32(A))
        d, keep = wfm_desc(job(cfg), RATE)
        vid = ctx.vfo_add(d, keep)
        sd, skeep = stereo_desc_of(cfg)
        assert call(vid, sd) == want, (A, want)
    long_taps = np.zeros((PILOT_MAX_TAPS + 1, 2), np.float32)
    sd, skeep = stereo_desc_of(dict(make_cfg(), ptaps=long_taps))
    d, keep = wfm_desc(job(make_cfg()), RATE)
    assert call(ctx.vfo_add(d, keep), sd) == UNSUPPORTED
    ctx.close()
