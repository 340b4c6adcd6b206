"""The AM and SSB / CW demodulator tails (vfo_sequential_body: DC blocker, loop::AGC with its look-ahead), sample by sample.

test_kernel_forms.py checks every channeliser form per sample with the AGC pinned to unit gain, test_af_chain.py the AF chain behind the demodulator; the
tail between them was only checked by test_parity_vfo.py::test_agc_look_ahead_follows_reference_blocks, an RMS over whole pushes of one burst pattern.  Here
every edge of the tail is placed on purpose — ROWS below, one row per edge, each stating what it is there for — and every output frame is compared.

THE RESTATEMENTS (agc_real, agc_complex, dc_block, tail) are written in numpy scalars over a `dtype`: float64 is the yardstick, float32 the sequential baseline
(one rounding per operation, the reference's order).  They take the demodulator's parameters explicitly (PRM: the oracle fixes them, the descriptor does not),
the state, and the reference's block ends as cumulative IF sample counts; they return the clip indices and the decision margin
min |inAmp * gain / max_output_amp - 1| as well.  test_float32_restatement_is_the_oracle_bit_for_bit pins the float32 one to the compiled oracle (DSB, AM with
both AGC placements, default parameters, bursts, blocks that are no multiples of 64) without a device.

ISOLATION.  The restatement's input is the product's own IF for the same pushes (test_af_chain.py's trick).  Rows that place clips on exact lanes use a
hand descriptor whose chain is the identity (offset 0, no stage, no resampler, no channel filter, second translation (1, 0), a one-tap audio filter) and assert
first that the IF equals the input bit for bit; the two `dec_*` rows carry block ends through bounds_decim / bounds_poly and take the IF block ends from the
per-push IF counts of the block-by-block run.  One context holds one VFO per mode (DSB, AM with the audio AGC, AM with the carrier AGC) over the same
input, each with a RAW twin on the same chain that delivers the IF in pipelined mode.

FOUR RUNS PER ROW: (a) ordinary passes, one push per reference block; (b) ordinary passes over the row's ragged / large pushes with
sdrpp_set_reference_block(B); (c) pipelined over the pushes of (b); (d) pipelined with launch groups of 3 or 4 over the pushes of (a).  (b), (c), (d) equal
(a) bit for bit, audio and IF; (c) and (d) never fall back to an ordinary pass and run the tick's `seq` role.  (a) meets test_kernel_forms.py's per-sample
bar (MARGIN, BASELINE_MAX and the 1.25 rule are imported): max |got - ref64| / rms(ref64) over every frame within MARGIN x the same distance of the float32
restatement, whose figure is recorded per leg in BASELINES.

WHAT MAKES THE BAR MEANINGFUL.  The clip test is a discontinuity: every row's input keeps the float64 decision margin >= MIN_MARGIN at every sample and
the float32 and float64 clip lists identical, and every row's edge (clip indices, lanes, block ends, clamp, zeros) is asserted on the restatement before a
device runs (check_row).  A row whose input no longer hits its edge fails there."""
import bisect
import os

import numpy as np
import pytest

import support as S
from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_kernel_forms import BASELINE_MAX, MARGIN, _bits_equal, _fir64, _lp, _orc_fir, _parts, dist, hand_desc, ragged

MIN_MARGIN = 1e-3
MODES = ("DSB", "AMA", "AMC")  # SSB family with an identity second translation; AM with the audio AGC; AM with the carrier AGC
INF = float("inf")
# the demodulator's parameters; the descriptor takes them as float32 (sdrpp_vfo_desc), so do the restatements
PRM = dict(set_point=1.0, attack=0.01, decay=0.002, max_gain=10e6, max_output_amp=10.0, init_gain=INF, dc_rate=1e-4)
FAST = dict(attack=0.05, decay=0.5)  # amp falls by half per sample: a second clip inside one chunk


def prm(**kw):
    p = dict(PRM)
    p.update(kw)
    return p


# ---- restatements ----------------------------------------------------------------------------------------------------------------------------
def _agc(x, inamp, p, amp, ends, f, scan=None):
    """loop::AGC::process (agc.h:70-109) over consecutive blocks ending at `ends`; inamp = |x| per sample in dtype f; `scan`: the values the look-ahead takes
    its maximum of (None: inamp — anything else restates a DEFECT, for the checks that a row can tell it from the operation)."""
    g32 = lambda k: np.float32(p[k])
    sp, att, dec, mg, mo = (f(g32(k)) for k in ("set_point", "attack", "decay", "max_gain", "max_output_amp"))
    iatt, idec = f(np.float32(1.0) - g32("attack")), f(np.float32(1.0) - g32("decay"))  # agc.h:16-18: float values of 1.0f - rate
    if amp is None:
        amp = f(g32("set_point") / g32("init_gain"))  # agc.h:22
    amp = f(amp)
    scan = inamp if scan is None else scan
    gain = np.empty(len(inamp), f)
    clips, margin, one, lo = [], INF, f(1.0), 0
    for hi in ends:
        for i in range(lo, hi):
            a = inamp[i]
            if a != 0:
                amp = (amp * iatt) + (a * att) if a > amp else (amp * idec) + (a * dec)
                g = sp / amp
                g = mg if mg < g else g
            else:
                g = one
            margin = min(margin, abs(float(a) * float(g) / float(mo) - 1.0))
            if a * g > mo:
                clips.append(i)
                amp = scan[i:hi].max()
                g = sp / amp
                g = mg if mg < g else g
            gain[i] = g
        lo = hi
    assert lo == len(inamp), (lo, len(inamp))
    return gain, dict(clips=clips, margin=margin, amp=amp, gain=gain)


def agc_real(x, p, amp, ends, dtype, scan=None):
    """agc.h:70-109, T = float -> (out, info)"""
    x = np.asarray(x, dtype)
    gain, info = _agc(x, np.abs(x), p, amp, ends, dtype, scan)
    return (x * gain).astype(dtype), info


def _mag(re, im, f):
    return np.sqrt(((re * re).astype(f) + (im * im).astype(f)).astype(f)).astype(f)


def agc_complex(x, p, amp, ends, dtype):
    """agc.h:70-109, T = complex_t (amplitude(): types.h:81-83) -> (re, im, info)"""
    re, im = np.asarray(x.real, dtype), np.asarray(x.imag, dtype)
    gain, info = _agc(x, _mag(re, im, dtype), p, amp, ends, dtype)
    return (re * gain).astype(dtype), (im * gain).astype(dtype), info


def dc_block(x, rate, offset, dtype):
    """dc_blocker.h:54-60: out = in - offset; offset += out * rate -> (out, offset)"""
    f = dtype
    rate, off = f(np.float32(rate)), f(offset)
    out = np.empty(len(x), f)
    for i, v in enumerate(np.asarray(x, f)):
        o = v - off
        out[i] = o
        off = off + (o * rate)
    return out, off


def tail(mode, y, p, ends, dtype, ataps=None, defect=None):
    """The demodulator tail of `mode` behind the IF stream y (complex64) from cleared state -> (audio, info).  DSB: Re(IF) -> AGC -> {v, v} (ssb.h:77-92
    with an identity translation).  AMA: |x| -> DC blocker -> AGC -> audio FIR; AMC: AGC on the complex IF -> |x| -> DC blocker -> audio FIR
    (demod/am.h:101-131).  defect = "raw_scan" (AMA): the look-ahead takes the raw envelope instead of the DC blocker's output."""
    f = dtype
    re, im = y.real.astype(f), y.imag.astype(f)
    if mode == "DSB":
        return agc_real(re, p, None, ends, f)
    if mode == "AMA":
        m = _mag(re, im, f)
        v, _ = dc_block(m, p["dc_rate"], 0.0, f)
        out, info = agc_real(v, p, None, ends, f, scan=m if defect == "raw_scan" else None)
    else:
        gr, gi, info = agc_complex(y, p, None, ends, f)
        out, _ = dc_block(_mag(gr, gi, f), p["dc_rate"], 0.0, f)
    if ataps is not None:
        out = _fir64(out, ataps) if f == np.float64 else _orc_fir(out, ataps, 1, width=1)
    return out, info


# ---- geometry of a sample inside the kernel's walk ---------------------------------------------------------------------------------------------
def blocks_of(pushes, B):
    """Reference-block ends (cumulative) of `pushes` with sdrpp_set_reference_block(B): every push is cut into blocks of B and a remainder."""
    ends, pos = [], 0
    for p in pushes:
        left = p
        while left > 0:
            c = min(B, left) if B else left
            pos += c
            left -= c
            ends.append(pos)
    return ends


def geom(i, ends):
    """Where sample i stands: its block, and its lane / chunk length in the kernel's walk (chunks of 64 from the block's start)."""
    k = bisect.bisect_right(ends, i)
    lo, hi = (ends[k - 1] if k else 0), ends[k]
    lane = (i - lo) % 64
    return dict(block=k, lo=lo, hi=hi, lane=lane, cnt=min(64, hi - (i - lane)), first=i == lo, last=i == hi - 1, size=hi - lo)


def block_at(ends, after, min_size, nth=0):
    """(lo, hi) of the nth block of at least min_size samples that starts at or behind `after`"""
    lo = 0
    for hi in ends:
        if lo >= after and hi - lo >= min_size:
            if nth == 0:
                return lo, hi
            nth -= 1
        lo = hi
    raise AssertionError("no such block")


# ---- descriptors -----------------------------------------------------------------------------------------------------------------------------
def set_tail(d, keep, mode, p):
    """The demodulator fields of a descriptor for `mode` with parameters p; AM gets a one-tap audio filter [1.0] unless it has one."""
    from sdrplusplus_amd import radio

    d.demod = radio.DEMOD_CODES["DSB" if mode == "DSB" else "AM"]
    d.agc_set_point, d.agc_attack, d.agc_decay = p["set_point"], p["attack"], p["decay"]
    d.agc_max_gain, d.agc_max_output_amp, d.agc_init_gain = p["max_gain"], p["max_output_amp"], p["init_gain"]
    d.am_carrier_agc = int(mode == "AMC")
    d.dc_block_rate = p["dc_rate"]
    d.ssb_phase_delta_re, d.ssb_phase_delta_im = 1.0, 0.0
    if mode != "DSB" and d.audio_ntaps == 0:
        one = np.ones(1, np.float32)
        keep.append(one)
        d.audio_ntaps, d.audio_taps = 1, radio._fp(one)
    return d


def desc_params(d):
    """The tail's parameters as a descriptor holds them (radio.vfo_desc rows)."""
    return dict(set_point=d.agc_set_point, attack=d.agc_attack, decay=d.agc_decay, max_gain=d.agc_max_gain, max_output_amp=d.agc_max_output_amp,
                init_gain=d.agc_init_gain, dc_rate=d.dc_block_rate)


def identity_jobs(jobs, half=False, sr=48000.0):
    """[(mode, p)] -> [(mode, p, desc, keep, raw twin desc, twin keep, audio taps)] on the identity chain; half: behind ONE decimator stage, /2 with the
    single tap 1.0 (IF[m] = input[2 m] exactly) — a chain that only rotates never shares a launch (group_eligible), this one does."""
    out = []
    stages = [(2, np.ones(1, np.float32))] if half else []
    for mode, p in jobs:
        d, keep, _ = hand_desc(sr, 0.0, stages)
        t, tkeep, _ = hand_desc(sr, 0.0, stages)
        set_tail(d, keep, mode, p)
        out.append((mode, p, d, keep, t, tkeep, None if mode == "DSB" else np.ones(1, np.float32)))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def floor(n, level=0.01):
    return level * (1.0 + 0.2 * np.sin(2 * np.pi * np.arange(n) / 23.7))


def carrier(u):
    """u >= 0 -> complex64 with |x| = u and Re(x) = u cos(phi), phi between 0.1 and 0.7 rad: every mode's AGC sees the shape of u."""
    i = np.arange(len(u))
    return (u * np.exp(1j * (0.4 + 0.3 * np.sin(2 * np.pi * i / 41.0)))).astype(np.complex64)


THREE = lambda **kw: [(m, prm(**kw)) for m in MODES]


class Row:
    """build() -> dict(x, pushes (run b), B, jobs [(mode, p)] or prepared jobs, clips (list, {job index: list} or None = count rule), geometry
    [(index, {property: value})], extra (callable(case, infos64) with further CPU assertions)); `why`: what the row is there for."""

    def __init__(self, rid, why, build, identity=True, group=3, half=False, grouping=True):
        self.id, self.why, self.build, self.identity, self.group, self.half = rid, why, build, identity, group, half
        self.grouping = grouping and (half or not identity)  # (a chain without a decimator stage goes out one push per launch: run (d) is then run (c) over the pushes of (a))


N0, B0 = 2400, 200


def _pushes(n=N0):
    return ragged(n, 64)  # 1, 7, a prime, 63, 65, two uneven parts: blocks of B inside the long pushes start in mid-chunk of the push


def _spike_row(lane, chunk=1, **kw):
    """One 40 dB spike on `lane` of chunk `chunk` (full) of a 200-sample block; slow AGC: the stream's first sample and the spike clip, nothing else."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        pos = lo + 64 * chunk + lane
        u = floor(N0)
        u[pos] = 1.0
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=THREE(**kw), clips=[0, pos], geometry=[(pos, dict(lane=lane, cnt=64, lo=lo))])
    return build


def _at_row(where, **kw):
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        u = floor(N0)
        g = {}
        if where == "block_last_short_chunk":  # the look-ahead covers one sample; lane 7 of a chunk of 8
            lo, hi = block_at(ends, 400, B0, 1)
            pos, g = hi - 1, dict(last=True, cnt=8, lane=7)
        elif where == "block_last_full_chunk":  # a push of 128 samples: its last sample is lane 63 of a full chunk AND the block's last
            pushes = [700, 128, 1, 900, N0 - 1729]
            ends = blocks_of(pushes, B0)
            pos, g = 827, dict(last=True, cnt=64, lane=63, size=128)
        elif where == "block_first_midchunk":  # the second block of a long push: blk_lo = 200 inside the push, no multiple of 64
            lo, hi = block_at(ends, 400, B0, 1)
            pos, g = lo, dict(first=True, lane=0)
            start = max(e for e in np.cumsum([0] + pushes) if e <= lo)
            assert (lo - start) % 64 != 0 and lo > start, (lo, start)
        elif where == "short_chunk_mid":  # a lane in the middle of a final short chunk
            lo, hi = block_at(ends, 400, B0, 1)
            pos, g = hi - 5, dict(cnt=8, lane=3)
        u[pos] = 1.0
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=THREE(**kw), clips=[0, pos], geometry=[(pos, g)])
    return build


def _first_nonzero():
    """Five zero samples, then the stream: with init_gain = inf the first non-zero sample clips (amp = 0 + a * attack).  DSB and the carrier AGC (complex
    zeros); behind AM's DC blocker the zeros are zeros too while the offset is still 0."""
    def build():
        u = floor(N0)
        u[:5] = 0.0
        return dict(x=carrier(u), pushes=_pushes(), B=B0, jobs=THREE(), clips=[5], geometry=[(5, dict(lane=4, block=1))], extra=_zero_extra([(0, 5)], all_modes=True))
    return build


def _multi_row(offsets, heights, **kw):
    """Spikes at chunk start + offsets (one full chunk of a block), fast decay: every one clips, and the scan restarts behind each."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        u = floor(N0)
        pos = [lo + 64 + o for o in offsets]
        for q, h in zip(pos, heights):
            u[q] = h
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=THREE(**dict(FAST, **kw)), clips=[0] + pos, geometry=[(q, dict(lo=lo, cnt=64, lane=o)) for q, o in zip(pos, offsets)])
    return build


def _adjacent():
    """Clips at f and f + 1 inside one chunk: only possible with max_output_amp below set_point (behind a clip amp >= every later sample of the block, so the
    next sample's output is at most set_point); f + 1 holds the block's maximum."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        f = lo + 64 + 20
        u = np.zeros(N0)  # (below set_point EVERY sample of a steady signal clips: zeros, which never do, around a short stretch of signal)
        u[f - 50:f + 60] = 0.01
        u[f], u[f + 1] = 0.5, 1.0
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=[(m, prm(max_output_amp=0.8, attack=0.05, decay=0.2, dc_rate=0.0)) for m in MODES], clips=None, must_clip=[f, f + 1],
                    geometry=[(f, dict(lane=20, cnt=64)), (f + 1, dict(lane=21, cnt=64))], min_clips=20)
    return build


def _noise(seed, nudges=()):
    """Seeded noise with max_output_amp close to set_point: a dense-clip regime, at least a tenth of the samples clip in every mode."""
    def build():
        r = np.random.default_rng(seed)
        x = ((r.standard_normal(N0) + 1j * r.standard_normal(N0)) * 0.05 + 0.02)
        for i in nudges:  # (samples moved off the decision threshold: the margin condition is a property of the input)
            x[i] *= 1.03
        return dict(x=x.astype(np.complex64), pushes=_pushes(), B=B0, jobs=THREE(max_output_amp=1.05, dc_rate=0.01, **FAST), clips=None, min_clips=N0 // 10)
    return build


def _max_row(where):
    """A clip at f (lane 20 of a full chunk, 0.5 over a floor of 0.01) and the largest sample of the neighbourhood, 20.0 = 32 dB above it, at `where`."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        assert ends[ends.index(hi) + 1] - hi == B0
        u = floor(N0)
        f = lo + 64 + 20
        u[f] = 0.5
        big = dict(earlier=f - 18, later_lane=f + 30, later_chunk=f + 70, block_last=hi - 1, next_block=hi)[where]
        u[big] = 20.0
        clips = [0] + sorted([f, big])
        g = [(f, dict(lane=20, cnt=64, lo=lo))]
        if where == "earlier":
            g.append((big, dict(lo=lo, lane=2, cnt=64)))
        elif where == "later_lane":
            g.append((big, dict(lo=lo, lane=50, cnt=64)))
        elif where == "later_chunk":
            g.append((big, dict(lo=lo, lane=26)))
        elif where == "block_last":
            g.append((big, dict(lo=lo, last=True)))
        else:
            g.append((big, dict(lo=hi, first=True)))

        def extra(case, infos):
            for (mode, p, *_), info in zip(case["jobs"], infos):
                gf = float(info["gain"][f])
                seen = where in ("later_lane", "later_chunk", "block_last")  # the look-ahead from f sees the large sample
                assert (gf < 0.1) == seen, (where, mode, gf)  # amp = 20 x cos(phi) or 0.5 x cos(phi): gain ~0.05 or ~2
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=THREE(**FAST), clips=clips, geometry=g, extra=extra)
    return build


def _clamp_tiny():
    """An input so small that set_point / amp > max_gain for thousands of samples (gain = max_gain = 1e7, output 0.1: not even the first sample clips), then a
    40 dB burst that clips."""
    def build():
        u = floor(N0, 1e-8)
        u[1500:1600] = 3e-6 * (1.0 + 0.2 * np.sin(np.arange(100) / 5.0))

        def extra(case, infos):
            for (mode, p, *_), info in zip(case["jobs"], infos):
                assert np.all(info["gain"][:1500] == np.float32(10e6)) and info["gain"][1500] < 10e6, (mode, info["gain"][:3])
        return dict(x=carrier(u), pushes=_pushes(), B=B0, jobs=THREE(dc_rate=0.0), clips=[1500], geometry=[], extra=extra)
    return build


def _clamp_50():
    """max_gain = 50 with a floor of 0.01 (set_point / amp = 100): the clamp decides every gain up to the spike, and again behind it once amp has fallen."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        u = floor(N0)
        pos = lo + 64 + 33
        u[pos] = 1.0

        def extra(case, infos):
            for (mode, p, *_), info in zip(case["jobs"], infos):
                g = info["gain"]
                assert g[pos - 1] == 50.0 and g[pos] < 50.0 and g[pos + 1] < 50.0 and g[pos + 20] == 50.0, (mode, g[pos - 1:pos + 21])
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=THREE(max_gain=50.0, dc_rate=0.0, **FAST), clips=[pos], geometry=[(pos, dict(lane=33, cnt=64))], extra=extra)
    return build


def _zero_extra(runs, all_modes=False):
    def extra(case, infos):
        for (mode, p, *_), info in zip(case["jobs"], infos):
            assert mode != "AMA" or all_modes
            for a, b in runs:
                assert np.all(info["gain"][a:b] == 1.0), (mode, a, b)  # inAmp == 0: gain 1, amp untouched
    return extra


def _zeros_runs():
    """Runs of exact zeros (complex zeros) inside a chunk, across a chunk boundary and across a block end, fast decay: amp must stand still over them (a tracker
    that took the zeros in would fall to nothing within ten samples and the sample behind the run would clip)."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        u = floor(N0)
        runs = [(lo + 10, lo + 30), (lo + 120, lo + 140), (hi - 12, hi + 15)]
        for a, b in runs:
            u[a:b] = 0.0
        g = [(runs[0][0], dict(lane=10)), (runs[0][1] - 1, dict(lane=29)), (runs[1][0], dict(lane=56)), (runs[1][1] - 1, dict(lane=11)), (runs[2][0], dict(lo=lo)), (runs[2][1] - 1, dict(lo=hi))]
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=[(m, prm(**FAST)) for m in ("DSB", "AMC")], clips=[0], geometry=g, extra=_zero_extra(runs))
    return build


def _zero_block():
    """A whole reference block of zeros between two bursts: gain 1 and amp frozen for the block (the reference's behaviour); the second burst, as large as
    the first, finds amp where the first left it and does not clip."""
    def build():
        pushes = _pushes()
        ends = blocks_of(pushes, B0)
        lo, hi = block_at(ends, 400, B0, 1)
        u = floor(N0)
        u[lo - 40:lo] = 0.3
        u[lo:hi] = 0.0
        u[hi:hi + 40] = 0.3
        return dict(x=carrier(u), pushes=pushes, B=B0, jobs=[(m, prm()) for m in ("DSB", "AMC")], clips=[0, lo - 40], geometry=[(lo, dict(first=True)), (hi - 1, dict(last=True))],
                    extra=_zero_extra([(lo, hi)]))
    return build


def _am_dc(jobs_kw):
    """AM with the audio AGC and a DC blocker far from settled (dc_rate 0.05, offset 0 at the start): a carrier of 0.003 steps to 0.3 at sample 10 and swells to
    0.45 later in the block.  The look-ahead at the clip must take the DC blocker's FUTURE output (at most 0.3: the offset has followed the carrier by
    then), not the envelope (0.45); the samples behind the clip check the offset carried from behind it."""
    def build():
        n = 2000
        i = np.arange(n)
        u = 0.3 * (1.0 + 0.5 * np.exp(-((i - 60) / 15.0) ** 2) + 0.1 * np.sin(2 * np.pi * i / 31.0))
        u[:10] = 0.003
        p = prm(dc_rate=0.05, **jobs_kw)

        def extra(case, infos):
            y = case["if"]
            ends = case["ends"]
            good, _ = tail("AMA", y, p, ends, np.float64)
            bad, ib = tail("AMA", y, p, ends, np.float64, defect="raw_scan")
            assert abs(good[10] - bad[10]) > 1e-2, ("a look-ahead over the raw envelope must show at the clip", good[10], bad[10])
        return dict(x=carrier(u), pushes=[1, 7, 150, 64, 778, 1000], B=100, jobs=[("AMA", p), ("AMA", prm(dc_rate=0.05, **dict(jobs_kw, max_output_amp=5.0)))], clips=None,
                    must_clip=[0, 10], geometry=[(10, dict(lane=2, block=2))], extra=extra)
    return build


def _shape_row(B, n, pushes):
    """Spikes of five heights every 37 samples, fast decay: every one clips and amp behind it is the maximum over the REST OF ITS BLOCK, which depends on where
    the block ends."""
    def build():
        assert sum(pushes) == n
        u = floor(n)
        pos = list(range(20, n, 37))
        for k, q in enumerate(pos):
            u[q] = (1.0, 0.5, 2.0, 0.7, 1.5)[k % 5]
        return dict(x=carrier(u), pushes=pushes, B=B, jobs=THREE(dc_rate=2e-5, **FAST), clips=[0] + pos, geometry=[])  # (a DC rate at which the offset stays below the floor: no zero crossing behind the blocker)
    return build


def _many_jobs():
    """Five VFOs with different modes and AGC parameters in one context: one wavefront per job, every one with its own state."""
    def build():
        n = N0
        u = floor(n)
        for k, q in enumerate(range(30, n, 53)):
            u[q] = (1.0, 0.4, 2.5)[k % 3]
        jobs = [("DSB", prm(**FAST)), ("AMA", prm(dc_rate=0.02, attack=0.03, decay=0.3)), ("AMC", prm(max_gain=50.0, **FAST)), ("DSB", prm(max_output_amp=3.0, attack=0.02, decay=0.05, init_gain=1.0)),
                ("AMC", prm(set_point=0.5, max_output_amp=4.0, attack=0.02, decay=0.4)), ("AMA", prm(dc_rate=1e-3, **FAST))]
        return dict(x=carrier(u), pushes=_pushes(n), B=B0, jobs=jobs, clips=None, min_clips=10, geometry=[])
    return build


def _burst_input(n, seed, period, level=0.02, low=0.0005, on=(2,)):
    """Bursts 32 dB above the floor that start and end inside blocks, each 15 times the one before (a slow decay has not let go of the last one yet)."""
    r = np.random.default_rng(seed)
    i = np.arange(n)
    env = np.where(np.isin((i // period) % 3, on), level * 15.0 ** (i // (3 * period)), low)
    x = env * (1.0 + 0.4 * np.sin(2 * np.pi * i / 211.0)) * np.exp(1j * 0.5) + (r.standard_normal(n) + 1j * r.standard_normal(n)) * 1e-5
    return x.astype(np.complex64)


def _dec_hand():
    """Block ends through bounds_decim and bounds_poly: a /4 first stage, then a polyphase 3/5 resampler; 1 000-sample reference blocks give 150 IF samples
    each, with stage offsets and phases that differ from block to block."""
    def build():
        sr, n = 96000.0, 30000
        st = [(4, _lp(27, 0.4 * sr / 4, sr))]
        rt = _lp(61, 0.45 * (sr / 4) * 3 / 5, sr / 4 * 3) * np.float32(3)
        jobs = []
        for mode in MODES:
            p = prm(attack=0.02, decay=0.01, dc_rate=0.002)
            d, keep, rate = hand_desc(sr, 0.0, st, 3, 5, rt, None)
            t, tkeep, _ = hand_desc(sr, 0.0, st, 3, 5, rt, None)
            set_tail(d, keep, mode, p)
            jobs.append((mode, p, d, keep, t, tkeep, None if mode == "DSB" else np.ones(1, np.float32)))
        return dict(x=_burst_input(n, 5, 2300), pushes=[1, 7, 4999, 1000, 3001, 20992], B=1000, jobs=jobs, clips=None, min_clips=4, geometry=[])
    return build


def _dec_radio():
    """radio.vfo_desc's own plans and default AGC / DC parameters at 20 kS/s, offset 0: DSB through an INTERPOLATING 6/5 resampler, AM (audio and carrier AGC)
    through 3/4, each behind its channel filter; 1 000-sample reference blocks."""
    def build():
        from sdrplusplus_amd import radio

        sr, n = 20000.0, 12000
        jobs = []
        for mode in MODES:
            rmode = "DSB" if mode == "DSB" else "AM"
            if_rate, bw = radio.RADIO_DEFAULTS[rmode]
            d, keep = radio.vfo_desc(sr, if_rate, bw, 0.0, rmode, carrier_agc=(mode == "AMC"))
            t, tkeep = radio.vfo_desc(sr, if_rate, bw, 0.0, "RAW")
            assert (d.interp > d.decim) == (mode == "DSB") and d.interp != d.decim, (mode, d.interp, d.decim)
            jobs.append((mode, desc_params(d), d, keep, t, tkeep, _parts(d)["ataps"]))
        return dict(x=_burst_input(n, 6, 1900, on=(1, 2)), pushes=[1, 7, 2999, 1000, 4001, 3992], B=1000, jobs=jobs, clips=None, min_clips=3, geometry=[])
    return build


ROWS = [
    # ---- where in a chunk the clip stands ----
    Row("lane0", "a clip on lane 0 of a full chunk", _spike_row(0)),
    Row("lane1", "a clip on lane 1 of a full chunk", _spike_row(1)),
    Row("lane62", "a clip on lane 62 of a full chunk: the restart finds one lane left", _spike_row(62)),
    Row("lane63", "a clip on lane 63 of a full chunk: the restart finds nothing left", _spike_row(63)),
    Row("first_nonzero", "the first non-zero sample of the stream clips (init_gain = inf) behind leading zeros", _first_nonzero()),
    Row("block_last_short_chunk", "a clip on the last sample of a block, last lane of a short chunk: the look-ahead covers one sample", _at_row("block_last_short_chunk")),
    Row("block_last_full_chunk", "a clip on the last sample of a 128-sample block: lane 63 and the block's end at once", _at_row("block_last_full_chunk")),
    Row("short_chunk_mid", "a clip inside a final chunk of 8 lanes", _at_row("short_chunk_mid")),
    Row("block_first_midchunk", "a clip on the first sample of a block that starts in mid-chunk of its push", _at_row("block_first_midchunk")),
    # ---- several clips per chunk ----
    Row("two_clips", "two clips in one chunk: the restart path twice", _multi_row([5, 40], [1.0, 0.6])),
    Row("three_clips", "three clips in one chunk", _multi_row([0, 31, 63], [0.7, 1.3, 0.9])),
    Row("ten_clips", "ten clips in one chunk (decay 0.8)", _multi_row([1, 8, 14, 20, 27, 33, 40, 46, 53, 60], [1.0, 0.5, 2.0, 0.7, 1.5, 0.6, 1.1, 0.8, 2.2, 0.9], decay=0.8)),
    Row("adjacent_clips", "clips at f and f + 1 in one chunk (max_output_amp below set_point)", _adjacent()),
    Row("dense_noise", "seeded noise, max_output_amp = 1.05 set_point: at least a tenth of the samples clip", _noise(7, (103, 204, 300, 865, 956, 1394, 1183, 1394, 1790, 1993))),
    # ---- where the look-ahead's maximum lies ----
    Row("max_earlier_lane", "the largest sample on an EARLIER lane of the clip's chunk: ignored", _max_row("earlier")),
    Row("max_at_f", "the clip itself is the largest sample of its block", _spike_row(10, chunk=2, **FAST)),
    Row("max_later_lane", "the largest sample on a later lane of the same chunk", _max_row("later_lane")),
    Row("max_later_chunk", "the largest sample in a later chunk of the block", _max_row("later_chunk")),
    Row("max_block_last", "the largest sample is the block's last", _max_row("block_last")),
    Row("max_next_block", "the largest sample is the first of the NEXT block: ignored — the block-end semantics", _max_row("next_block")),
    # ---- the gain clamp ----
    Row("clamp_tiny_input", "set_point / amp > max_gain: the clamp gives every gain", _clamp_tiny()),
    Row("clamp_50", "max_gain = 50: the clamp is active next to a clip", _clamp_50()),
    # ---- exact zeros ----
    Row("zeros_runs", "runs of exact zeros inside a chunk, across a chunk boundary, across a block end", _zeros_runs()),
    Row("zero_block", "a whole block of zeros between two bursts: gain 1, amp frozen", _zero_block()),
    # ---- AM, audio AGC: the look-ahead re-runs the DC blocker ----
    Row("am_dc_unsettled", "AM audio AGC, dc_rate 0.05, a clip at sample 10: the look-ahead over the DC blocker's future output", _am_dc(dict(attack=0.05, decay=0.1))),
    # ---- block and push shapes ----
    Row("blk1", "reference blocks of 1 sample", _shape_row(1, 2000, [1, 1, 700, 1, 1297]), group=4),
    Row("blk63", "reference blocks of 63", _shape_row(63, 2000, [31, 63, 3 * 63 + 17, 1, 1, 1000, 698])),
    Row("blk64", "reference blocks of 64", _shape_row(64, 2000, [32, 64, 3 * 64 + 17, 1, 1, 1000, 693]), group=4),
    Row("blk65", "reference blocks of 65", _shape_row(65, 2000, [33, 65, 3 * 65 + 17, 1, 1, 1000, 688])),
    Row("blk100", "reference blocks of 100", _shape_row(100, 2000, [50, 100, 317, 1, 1, 1000, 531]), group=4),
    Row("blk1000", "reference blocks of 1 000", _shape_row(1000, 5000, [500, 1000, 3017, 1, 1, 481])),
    # ---- more than one job per launch ----
    Row("six_jobs", "six VFOs, different modes and AGC parameters, one context", _many_jobs(), group=4),
    # ---- block ends through the decimators ----
    Row("dec_hand_4_3over5", "block ends through bounds_decim (/4) and bounds_poly (3/5)", _dec_hand(), identity=False),
    Row("dec_radio_interp", "radio.vfo_desc defaults: block ends through an interpolating 6/5 and a 3/4 resampler (no stage: no launch groups)", _dec_radio(), identity=False, grouping=False),
]

# Some of the rows above a second time behind a /2 stage of one tap, where pushes share launches: run (d) in groups of 3 or 4.
HALF = ("lane0", "lane63", "block_last_full_chunk", "block_first_midchunk", "ten_clips", "dense_noise", "max_later_chunk", "max_next_block", "zeros_runs", "am_dc_unsettled", "blk64", "blk65",
        "six_jobs")
ROWS += [Row(r.id + "_half", r.why + "; behind a one-tap /2 stage, in launch groups", r.build, group=7 - r.group, half=True) for r in ROWS if r.id in HALF]

# Measured float32-sequential baselines per row and job (the float32 restatement against the float64 one, max-abs / rms): {row: [(emulator leg, device leg)
# per job]}.  The identity rows' IF is the input itself on both legs, so their two figures are one.  The bar of a job is MARGIN x the baseline measured at run
# time, which may not exceed 1.25 x the figure recorded here for its leg.
BASELINES = {
    "lane0": [(1.45e-06, 1.45e-06), (2.21e-06, 2.21e-06), (1.33e-06, 1.33e-06)],
    "lane1": [(1.71e-06, 1.71e-06), (2.21e-06, 2.21e-06), (1.33e-06, 1.33e-06)],
    "lane62": [(1.37e-06, 1.37e-06), (2.13e-06, 2.13e-06), (1.29e-06, 1.29e-06)],
    "lane63": [(1.37e-06, 1.37e-06), (2.13e-06, 2.13e-06), (1.29e-06, 1.29e-06)],
    "first_nonzero": [(1.1e-06, 1.1e-06), (9.73e-07, 9.73e-07), (1.07e-06, 1.07e-06)],
    "block_last_short_chunk": [(1.31e-06, 1.31e-06), (2.05e-06, 2.05e-06), (1.24e-06, 1.24e-06)],
    "block_last_full_chunk": [(2.16e-06, 2.16e-06), (1.91e-06, 1.91e-06), (1.17e-06, 1.17e-06)],
    "short_chunk_mid": [(1.32e-06, 1.32e-06), (2.06e-06, 2.06e-06), (1.25e-06, 1.25e-06)],
    "block_first_midchunk": [(1.48e-06, 1.48e-06), (2.3e-06, 2.3e-06), (1.39e-06, 1.39e-06)],
    "two_clips": [(3.62e-07, 3.62e-07), (4.39e-07, 4.39e-07), (4.88e-07, 4.88e-07)],
    "three_clips": [(3.62e-07, 3.62e-07), (3.85e-07, 3.85e-07), (3.82e-07, 3.82e-07)],
    "ten_clips": [(3.08e-07, 3.08e-07), (5.49e-07, 5.49e-07), (5.45e-07, 5.45e-07)],
    "adjacent_clips": [(6.08e-07, 6.08e-07), (6.75e-07, 6.75e-07), (7.23e-07, 7.23e-07)],
    "dense_noise": [(3.14e-07, 3.14e-07), (4.28e-06, 4.28e-06), (1.7e-06, 1.7e-06)],
    "max_earlier_lane": [(3.62e-07, 3.62e-07), (6.97e-07, 6.97e-07), (3.81e-07, 3.81e-07)],
    "max_at_f": [(3.61e-07, 3.61e-07), (3.84e-07, 3.84e-07), (4.45e-07, 4.45e-07)],
    "max_later_lane": [(3.62e-07, 3.62e-07), (7.38e-07, 7.38e-07), (4.12e-07, 4.12e-07)],
    "max_later_chunk": [(3.62e-07, 3.62e-07), (4.31e-07, 4.31e-07), (4.55e-07, 4.55e-07)],
    "max_block_last": [(3.62e-07, 3.62e-07), (7.8e-07, 7.8e-07), (4.17e-07, 4.17e-07)],
    "max_next_block": [(3.62e-07, 3.62e-07), (6.94e-07, 6.94e-07), (3.81e-07, 3.81e-07)],
    "clamp_tiny_input": [(1.41e-06, 1.41e-06), (1.1e-06, 1.1e-06), (1.09e-06, 1.09e-06)],
    "clamp_50": [(6.53e-08, 6.53e-08), (1.32e-07, 1.32e-07), (1.46e-07, 1.46e-07)],
    "zeros_runs": [(3.66e-07, 3.66e-07), (5.21e-07, 5.21e-07)],
    "zero_block": [(1.4e-06, 1.4e-06), (7.28e-06, 7.28e-06)],
    "am_dc_unsettled": [(3.46e-06, 3.46e-06), (3.46e-06, 3.46e-06)],
    "blk1": [(4.49e-07, 4.49e-07), (4.49e-07, 4.49e-07), (4.25e-07, 4.25e-07)],
    "blk63": [(4.51e-07, 4.51e-07), (4.52e-07, 4.52e-07), (4.98e-07, 4.98e-07)],
    "blk64": [(4.52e-07, 4.52e-07), (4.52e-07, 4.52e-07), (4.86e-07, 4.86e-07)],
    "blk65": [(4.21e-07, 4.21e-07), (4.28e-07, 4.28e-07), (4.81e-07, 4.81e-07)],
    "blk100": [(4.55e-07, 4.55e-07), (4.56e-07, 4.56e-07), (4.99e-07, 4.99e-07)],
    "blk1000": [(3.77e-07, 3.77e-07), (1.06e-06, 1.06e-06), (5.85e-07, 5.85e-07)],
    "six_jobs": [(3.92e-07, 3.92e-07), (7.12e-07, 7.12e-07), (4.23e-07, 4.23e-07), (2.49e-06, 2.49e-06), (5.35e-07, 5.35e-07), (5.37e-06, 5.37e-06)],
    "dec_hand_4_3over5": [(2.4e-06, 2.4e-06), (5.46e-06, 5.46e-06), (2.79e-06, 2.79e-06)],
    "dec_radio_interp": [(1.3e-05, 1.3e-05), (3.39e-05, 3.39e-05), (1.02e-05, 1.02e-05)],
    "lane0_half": [(1.45e-06, 1.45e-06), (2.21e-06, 2.21e-06), (1.33e-06, 1.33e-06)],
    "lane63_half": [(1.37e-06, 1.37e-06), (2.13e-06, 2.13e-06), (1.29e-06, 1.29e-06)],
    "block_last_full_chunk_half": [(2.16e-06, 2.16e-06), (1.91e-06, 1.91e-06), (1.17e-06, 1.17e-06)],
    "block_first_midchunk_half": [(1.48e-06, 1.48e-06), (2.3e-06, 2.3e-06), (1.39e-06, 1.39e-06)],
    "ten_clips_half": [(3.08e-07, 3.08e-07), (5.49e-07, 5.49e-07), (5.45e-07, 5.45e-07)],
    "dense_noise_half": [(3.14e-07, 3.14e-07), (4.28e-06, 4.28e-06), (1.7e-06, 1.7e-06)],
    "max_later_chunk_half": [(3.62e-07, 3.62e-07), (4.31e-07, 4.31e-07), (4.55e-07, 4.55e-07)],
    "max_next_block_half": [(3.62e-07, 3.62e-07), (6.94e-07, 6.94e-07), (3.81e-07, 3.81e-07)],
    "zeros_runs_half": [(3.66e-07, 3.66e-07), (5.21e-07, 5.21e-07)],
    "am_dc_unsettled_half": [(3.46e-06, 3.46e-06), (3.46e-06, 3.46e-06)],
    "blk64_half": [(4.52e-07, 4.52e-07), (4.52e-07, 4.52e-07), (4.86e-07, 4.86e-07)],
    "blk65_half": [(4.21e-07, 4.21e-07), (4.28e-07, 4.28e-07), (4.81e-07, 4.81e-07)],
    "six_jobs_half": [(3.92e-07, 3.92e-07), (7.12e-07, 7.12e-07), (4.23e-07, 4.23e-07), (2.49e-06, 2.49e-06), (5.35e-07, 5.35e-07), (5.37e-06, 5.37e-06)],
}


# ---- running -------------------------------------------------------------------------------------------------------------------------------
def prepare(row):
    case = row.build()
    case["if"] = case["x"]
    if row.identity:
        case["jobs"] = identity_jobs(case["jobs"], row.half)
    if row.half:  # the designed IF on the even input samples, something else on the odd ones; every push and block twice as long
        xin = np.empty(2 * len(case["x"]), np.complex64)
        xin[0::2], xin[1::2] = case["x"], np.roll(case["x"], 7) * np.complex64(-3.0 + 1.0j) + np.complex64(0.25)
        case["x"], case["pushes"], case["B"] = xin, [2 * q for q in case["pushes"]], 2 * case["B"]
    case["ends_in"] = blocks_of(case["pushes"], case["B"])
    case["blocks"] = list(np.diff([0] + case["ends_in"]))
    assert sum(case["pushes"]) == len(case["x"]) == case["ends_in"][-1]
    return case


def check_row(row, case, ifs, ends_if):
    """The CPU check of a row's edge, before its outputs are looked at: float64 and float32 restatements over the IF clip at the indices the row names, on the
    lanes it names, with the decision margin kept.  -> ([(ref64, info64)], [(base32, info32)]) per job"""
    r64, r32 = [], []
    for j, (mode, p, d, keep, t, tkeep, ataps) in enumerate(case["jobs"]):
        o64, i64 = tail(mode, ifs[j], p, ends_if[j], np.float64, ataps)
        o32, i32 = tail(mode, ifs[j], p, ends_if[j], np.float32, ataps)
        assert i64["margin"] >= MIN_MARGIN, (row.id, j, mode, "the input comes too close to the clip decision", i64["margin"])
        assert i32["clips"] == i64["clips"], (row.id, j, mode, "float32 and float64 restatements clip at different samples", i32["clips"][:20], i64["clips"][:20])
        named = case["clips"][j] if isinstance(case["clips"], dict) else case["clips"]
        if named is not None:
            assert i64["clips"] == named, (row.id, j, mode, "the row no longer clips where it says", i64["clips"][:40], named[:40])
        else:
            assert len(i64["clips"]) >= case.get("min_clips", 1), (row.id, j, mode, len(i64["clips"]))
            for q in case.get("must_clip", []):
                assert q in i64["clips"], (row.id, j, mode, q, i64["clips"][:40])
        if row.identity and row.id != "clamp_tiny_input" and np.float32(p["init_gain"]) == np.float32(INF) and np.float32(p["max_gain"]) >= 1e6:
            nz = np.flatnonzero(ifs[j] != 0)
            assert len(nz) and i64["clips"][0] == nz[0], (row.id, j, "the first non-zero sample must clip", i64["clips"][:3])
        r64.append((o64, i64))
        r32.append((o32, i32))
    for q, props in case.get("geometry", []):
        g = geom(q, ends_if[0])
        for k, v in props.items():
            assert g[k] == v, (row.id, "sample %d is not where the row says" % q, k, g)
    if case.get("extra"):
        case["ends"] = ends_if[0]
        case["extra"](case, [i for _, i in r64])
    return r64, r32


LAG = 16  # results are taken this many pushes behind: SDRPP_RESULT_SLOTS is 24, and a held push of a group of <= 4 is never asked for


def run(case, pushes, ref_block=0, pipelined=False, group=0):
    """-> dict(audio=[per job [n, 2]], ifs=[per job complex64], counts=[per job [IF samples per push]], forms, stats)"""
    from sdrplusplus_amd import capi

    mp = max(sum(pushes[i:i + max(1, group)]) for i in range(len(pushes)))
    ctx = capi.Context(0, max_push=mp)
    ctx.set_reference_block(ref_block)
    vids, tids = [], []
    for mode, p, d, keep, t, tkeep, ataps in case["jobs"]:
        vids.append(ctx.vfo_add(d, keep))
        tids.append(ctx.vfo_add(t, tkeep))
    if pipelined:
        ctx.set_pipelined(True, 1)
        if group:
            ctx.set_pipeline_group(group)
    nj = len(vids)
    audio, ifs = [[] for _ in range(nj)], [[] for _ in range(nj)]

    def take(tk):
        got = ctx.result_wait(tk)
        for j in range(nj):
            audio[j].append(got["vfo"][vids[j]])
            ifs[j].append(got["vfo"][tids[j]].copy().view(np.complex64).reshape(-1))
        ctx.result_release(tk)

    pos = 0
    for k, c in enumerate(pushes, start=1):
        ctx.push(case["x"][pos:pos + c])
        pos += c
        if pipelined:
            if k > LAG:
                take(k - LAG)
        else:
            for j in range(nj):
                audio[j].append(ctx.vfo_read(vids[j]).copy())
                ifs[j].append(ctx.vfo_read_if(vids[j]).copy())
                twin = ctx.vfo_read_if(tids[j])
                assert np.array_equal(twin.view(np.uint32), ifs[j][-1].view(np.uint32)), "the RAW twin's IF is the demodulating VFO's"
    if pipelined:
        for k in range(max(1, len(pushes) - LAG + 1), len(pushes) + 1):
            take(k)
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    gs = ctx.pipeline_group_stats() if (pipelined and group) else None
    ctx.close()
    return dict(audio=[np.concatenate(a) for a in audio], ifs=[np.concatenate(q) for q in ifs], counts=[[len(q) for q in qq] for qq in ifs], forms=forms, stats=st, groups=gs)


def _same(a, b, what):
    for j, (p, q) in enumerate(zip(a["audio"], b["audio"])):
        _bits_equal(p, q, "%s, job %d audio" % (what, j))
    for j, (p, q) in enumerate(zip(a["ifs"], b["ifs"])):
        _bits_equal(p.view(np.float32), q.view(np.float32), "%s, job %d IF" % (what, j))


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_tail_sample_by_sample(backend, row):
    case = prepare(row)
    x, nj = case["if"], len(case["jobs"])
    if row.identity:  # the row's edge, on the CPU, before anything runs on a device: the IF of an identity chain is the input
        pre = check_row(row, case, [x] * nj, [[e // 2 for e in case["ends_in"]] if row.half else case["ends_in"]] * nj)
    a = run(case, case["blocks"])
    # reference-block ends at the IF rate: the per-push IF counts of the block-by-block run
    ends_if = [list(np.cumsum(c)) for c in a["counts"]]
    if row.identity:
        for j in range(nj):
            _bits_equal(a["ifs"][j].view(np.float32), x.view(np.float32), "%s: the identity chain's IF is the input" % row.id)
        r64, r32 = pre
    else:
        r64, r32 = check_row(row, case, a["ifs"], ends_if)
    b = run(case, case["pushes"], ref_block=case["B"])
    c = run(case, case["pushes"], ref_block=case["B"], pipelined=True)
    d = run(case, case["blocks"], pipelined=True, group=row.group)
    _same(a, b, "%s: pushes with a reference block size vs one push per block" % row.id)
    _same(a, c, "%s: pipelined vs one push per block" % row.id)
    _same(a, d, "%s: launch groups of %d vs one push per block" % (row.id, row.group))
    for r, npush, what in ((c, len(case["pushes"]), "pipelined"), (d, len(case["blocks"]), "grouped")):
        st = r["stats"]
        assert st["pass_blocks"] == 0 and st["tick_blocks"] == npush and not r["forms"], (row.id, what, st, r["forms"])
        assert st["roles"].get("seq", 0) > 0, (row.id, what, st["roles"])
    assert a["forms"].get("seq", 0) > 0 and b["forms"].get("seq", 0) > 0, (a["forms"], b["forms"])
    if row.grouping:
        assert d["groups"]["multi_groups"] >= 2 and d["groups"]["largest"] == row.group, d["groups"]
    figures = []
    for j, (mode, p, *_rest) in enumerate(case["jobs"]):
        got = a["audio"][j]
        assert np.array_equal(got[:, 0], got[:, 1])
        ref, base32 = r64[j][0], r32[j][0]
        base, e = dist(base32, ref), dist(got[:, 0], ref)
        figures.append((base, e))
        print("\n[tails %s job %d %s] %s per-sample max-abs / rms: baseline %.3g library %.3g (bar %.3g) | clips %d | margin %.3g" % (
            row.id, j, mode, backend, base, e, MARGIN * base, len(r64[j][1]["clips"]), r64[j][1]["margin"]), end="")
    print()
    if os.environ.get("SDRPP_TAILS_FIGURES"):  # (refilling BASELINES: one line per row and leg, baseline:library per job, appended to the named file)
        with open(os.environ["SDRPP_TAILS_FIGURES"], "a") as fh:
            fh.write("%s %s %s\n" % (row.id, backend, " ".join("%.3g:%.3g" % be for be in figures)))
    for j, (base, e) in enumerate(figures):
        mode = case["jobs"][j][0]
        assert base < BASELINE_MAX, ("ill-conditioned input: float32 sequential baseline", row.id, j, mode, base)
        at = int(np.argmax(np.abs(a["audio"][j][:, 0].astype(np.float64) - r64[j][0])))
        assert e <= MARGIN * base, (row.id, "job %d %s: %.3g against a float32 sequential baseline of %.3g" % (j, mode, e, base), at, geom(at, ends_if[j]))
        rec = BASELINES[row.id][j][backend == "gpu"]
        assert base <= 1.25 * rec, ("the float32 sequential baseline moved up: the bar may not loosen unseen", row.id, j, mode, backend, base, rec)


def test_every_row_states_its_purpose_and_the_table_is_complete():
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids) and all(len(r.why) > 15 for r in ROWS)
    assert sorted(BASELINES) == sorted(ids), (set(ids) ^ set(BASELINES))
    for r in ROWS:
        case = prepare(r)
        assert len(BASELINES[r.id]) == len(case["jobs"]), r.id
        assert 2000 <= len(case["x"]) <= 30000 and all(1 <= b <= 1000 * (2 if r.half else 1) for b in case["blocks"]), r.id


# ---- the float32 restatement is the oracle's arithmetic ------------------------------------------------------------------------------------------
def oracle_burst_if(n, seed=3):
    """A bursty IF: 30 dB bursts of uneven length over seeded noise and a carrier, which clip several times at the radio's default parameters."""
    r = np.random.default_rng(seed)
    i = np.arange(n)
    env = np.where((i // 700) % 4 == 3, 15.0 ** (i // 2800), 0.03)  # (each burst 15 times the last: the default decay lets go slowly)
    x = env * (0.3 * (1 + 0.5 * np.cos(2 * np.pi * i / 57.0)) * np.exp(1j * (0.3 + 2 * np.pi * i / 480.0)) + 0.1 * np.exp(-2j * np.pi * i / 33.0))
    x += (r.standard_normal(n) + 1j * r.standard_normal(n)) * 1e-3
    return x.astype(np.complex64)


ORACLE_BLOCKS = [1, 63, 65, 100, 517, 1000, 3, 777, 129, 350]


@pytest.mark.parametrize("mode", MODES)
def test_float32_restatement_is_the_oracle_bit_for_bit(mode):
    """CPU only.  orc_demod_process in DSB mode has an identity second translation and is exactly agc_real(Re(IF)); AM with and without the carrier AGC is compared
    behind its audio FIR, applied to the restatement with the oracle's own FIR.  Default parameters (attack 50 / rate, decay 5 / rate, max gain 1e7, max output 10,
    initial gain inf, DC rate 100 / rate), a bursty input that clips several times, the oracle driven block by block with blocks that are no multiples of 64."""
    o = S.oracle()
    rate, bw = (24000.0, 4600.0) if mode == "DSB" else (15000.0, 10000.0)
    blocks = ORACLE_BLOCKS * 3
    n = sum(blocks)
    y = oracle_burst_if(n)
    h = o.orc_demod_create(S.MODES["DSB" if mode == "DSB" else "AM"], bw, rate, 1, 50.0, 5.0, int(mode == "AMC"))
    outs, pos = [], 0
    for bsz in blocks:
        blk = np.ascontiguousarray(y[pos:pos + bsz])
        out = np.empty((bsz + 1, 2), np.float32)
        assert o.orc_demod_process(h, bsz, S._fp(blk.view(np.float32)), S._fp(out)) == bsz
        outs.append(out[:bsz].copy())
        pos += bsz
    o.orc_demod_destroy(h)
    orc = np.concatenate(outs)
    assert np.array_equal(orc[:, 0], orc[:, 1])
    p = prm(attack=np.float32(50.0 / rate), decay=np.float32(5.0 / rate), dc_rate=np.float32(100.0 / rate))
    ataps = None if mode == "DSB" else S.oracle_low_pass(bw / 2.0, (bw / 2.0) * 0.1, rate)
    got, info = tail(mode, y, p, list(np.cumsum(blocks)), np.float32, ataps)
    assert len(info["clips"]) >= 4 and len({geom(q, list(np.cumsum(blocks)))["block"] for q in info["clips"]}) >= 3, info["clips"]
    _bits_equal(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(orc[:, 0]), "float32 restatement of %s vs the oracle" % mode)
