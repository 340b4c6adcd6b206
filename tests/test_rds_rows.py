"""The WFM demodulator's RDS branch (vfo_rds_kernels.h: the front, line and rotator jobs of the wavefront-job role), sample by sample.

test_rds.py compares whole runs by RMS (bar 1e-5) at ONE description — radio.rds_desc(250e3), whose first stage of 44 taps decimating by 8 makes rds_tile_geometry
answer tile 29, pitch 34, a window of 268 samples — and a wrong sample per tile moves such an RMS by less than that bar.  Here every edge of the three bodies and of
the planner's job cutting is placed on purpose — ROWS below, one row per edge, each stating what it is there for — and every output is compared, from the first on.

THE RESTATEMENT (Restate) is the `_rdsOut` path of broadcast_fm.h:144-215 in numpy over a `dtype`, resuming across pushes from its state: the discriminator
(arctan2, difference, normalizePhase with FL_PI = 3.1415926535f, * invDeviation) over EVERY sample the VFO saw, previous phase 0 at the start and after
sdrpp_vfo_reset; the samples pushed while the branch is on are the fed ones; the translation in two forms — closed form: turns atan2(pd_im, pd_re) / 2 pi of the float32
increments times the count of fed samples; rotator form: frequency_xlator.h around volk's generic rotator, (d + 0j) * phase, phase *= delta, phase /= |phase| after every
512 samples of a call and once more at the end of a call whose count is no multiple of 512, one call per reference block — and the decimating FIRs over the fed
stream from a zeroed line (float64: test_kernel_forms._fir64; float32: k ascending, product and sum rounded on their own), the polyphase stage from _poly.  float64
is the yardstick (ref64), float32 the sequential baseline (base32): one rounding per operation, no fused multiply-add; the rotator form in float32 is the reference's
own arithmetic.  test_restatement_is_the_reference_per_sample pins it, without a context, a device or the oracle (the library's host-side design functions alone build the
description), to the reference's recorded outputs of tests/golden/rds_ref.npz in the fixture's blocks, `on` flags and resets: counts exactly, samples at the bar's level.

ISOLATION.  Rows use the identity chain (hand_desc(250e3, 0.0): offset 0, no stage, no channel filter) and first assert that vfo_read_if is the input bit for bit; the
push-structure rows sit behind a one-tap /2 stage (a launch group needs a decimator in front) whose RAW twin must deliver every second input sample bit for bit; the
row behind the IF chain feeds the restatement what vfo_ifc_read delivered (test_af_chain.py's trick).

THE BAR, per row and VFO, over every output: dist(device, ref64) <= MARGIN x dist(base32, ref64), dist = max |.| / rms(ref64) on the complex samples (test_kernel_forms.py's;
MARGIN, BASELINE_MAX and the 1.25 rule are imported).  BASELINES holds the baselines of this file's own CPU run.

CONDITIONS BEFORE A DEVICE'S OUTPUT IS LOOKED AT (check_row): the discriminator's margin min | |dphase| - pi | >= 0.1 rad, min |x| >= 0.1, at least one phase wrap,
rms(ref64) >= 1e-3, for geometry rows |h[0]| and |h[K-1]| >= 0.1 max |h| (a windowed low-pass has end taps of 1e-5: a phase loader one element short goes unseen
behind them), the frozen path (RdsJob::dline) and the history path (in.hist) both producing outputs, and the row's own edge from the kernel's constants restated
below (plan: the planner's job cutting and rds_freeze's bookkeeping in Python).  A row whose input no longer hits its edge fails there.

RUNS PER ROW: (a) ordinary passes in the row's cuts; (b) one push of the whole stream where the schedule has no switch; on the rows of PIPED (c) pipelined over (a)'s
cuts and (d) pipelined in launch groups of 3 or 4.  (a) meets the bar; (b) is within 1e-6 of (a)'s RMS in closed form (the NCO is anchored per push: test_rds.py's
bound) and bit-equal in rotator mode, whose cuts are whole reference blocks; (c) and (d) equal (a) bit for bit, never fall back to an ordinary pass and run the `ifc`
role.  VFOs of the bank equal, bit for bit, the same VFO alone in its context."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_kernel_forms import BASELINE_MAX, MARGIN, _bits_equal, _fir64, _lp, _poly, dist, hand_desc, rms
from test_rds import GOLDEN, broadcast

RATE = 250e3
NOT_FOUND, UNSUPPORTED = -6, -5
# the kernel's constants (vfo_ifchain_kernels.h, host_util.h, plan_vfo.h, vfo_rds_kernels.h), checked against the library's refusals in test_constants_are_the_headers
LDS_WAVE = 832     # SDRPP_WAVE_LDS_FLOATS
SEG_TILES = 4      # kRdsSegTiles: tiles per front job
LOAD_ROUND = 256   # the phase loader's round: 64 lanes x U = 4 loads in flight
CHUNK = 64         # the difference pass, the line body and the rotator walk 64 elements per round
RENORM = 512       # the rotator's renormalisation period
KMAX = {2: 272, 8: 272, 32: 255, 64: 192, 128: 128}  # the largest K with a tile, per D
FL_PI = np.float32(3.1415926535)
INV_DEV = np.float32(1.0 / (2.0 * math.pi * (75000.0 / RATE)))
MIN_WRAP_MARGIN, MIN_X, MIN_RMS, END_TAPS = 0.1, 0.1, 1e-3, 0.1
INF = float("inf")


def rds_tile_geometry(K, D):
    """host_util.h: (tile, pitch) for K taps decimating by D, or None where no tile's window and phases fit the wavefront's share of LDS"""
    lg = D.bit_length() - 1
    for t in range(64, 0, -1):
        P = t + ((K - 1) >> lg)
        if D >= 16:
            P |= 1
        elif D >= 2:
            g = 16 // D
            while P % (2 * g) != g:
                P += 1
        if 2 * D * P + (t - 1) * D + K + 1 <= LDS_WAVE:
            return t, P
    return None


def kmax(D):
    K = 1
    while rds_tile_geometry(K + 1, D):
        K += 1
    return K


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def _fir32(re, im, taps, D):
    """decimating_fir.h in float32: out[m] = sum_k taps[k] * buf[m * D + k], buf = (K - 1 zeros) ++ x; k ascending, product and sum rounded on their own"""
    f = np.float32
    K, n = len(taps), len(re)
    idx = np.arange((n + D - 1) // D) * D
    br, bi = np.concatenate([np.zeros(K - 1, f), re]), np.concatenate([np.zeros(K - 1, f), im])
    ar, ai = np.zeros(len(idx), f), np.zeros(len(idx), f)
    for k in range(K):
        h = f(taps[k])
        ar = ar + (br[idx + k] * h)
        ai = ai + (bi[idx + k] * h)
    return ar, ai


class Restate:
    """cfg: stages [(D, float32 taps)], interp, decim, rtaps (float32 or None), pd (float32 re, im), inv_dev; form: "closed" or "rotator".
    push(y, on, blocks) per push, reset() for sdrpp_vfo_reset; outputs() -> the branch's samples over everything fed, counts: outputs per push."""

    def __init__(self, cfg, f, form):
        self.cfg, self.f, self.form = cfg, f, form
        self.prev, self.fed, self.rot = f(0), 0, (f(1), f(0))  # quadrature.h's phase, samples fed, FrequencyXlator::phase (frequency_xlator.h:21)
        self.cr, self.ci, self.counts = [], [], []
        self.qmargin, self.xmin, self.wraps = INF, INF, 0
        self.theta = math.atan2(float(np.float32(cfg["pd"][1])), float(np.float32(cfg["pd"][0]))) / (2.0 * math.pi)

    def reset(self):
        self.prev = self.f(0)

    def nout(self, n):
        for D, _t in self.cfg["stages"]:
            n = (n + D - 1) // D
        if self.cfg["rtaps"] is not None:
            n = (n * self.cfg["interp"] + self.cfg["decim"] - 1) // self.cfg["decim"]
        return n

    def _norm(self, pr, pi):
        f = self.f
        h = f(np.sqrt(np.float64(pr) * np.float64(pr) + np.float64(pi) * np.float64(pi)))  # hypotf: the exact squares' sum, rounded once
        return pr / h, pi / h

    def push(self, y, on=True, blocks=None):
        f, n = self.f, len(y)
        PI = f(FL_PI)
        TWO = f(2) * PI
        # quadrature.h:39-46
        ph = np.arctan2(y.imag.astype(f), y.real.astype(f)).astype(f)
        d = (ph - np.concatenate([[self.prev], ph[:-1]]).astype(f)).astype(f)
        if n:
            a = np.abs(d.astype(np.float64))
            self.qmargin = min(self.qmargin, float(np.min(np.abs(a - math.pi))))
            self.wraps += int(np.sum(a > math.pi))
            self.xmin = min(self.xmin, float(np.min(np.abs(y.astype(np.complex128)))))
            self.prev = ph[-1]
        d = np.where(d > PI, d - TWO, np.where(d <= -PI, d + TWO, d)).astype(f)
        d = (d * f(np.float32(self.cfg["inv_dev"]))).astype(f)
        if not on:
            self.counts.append(0)
            return
        if self.form == "closed":
            t = self.theta * (self.fed + np.arange(n, dtype=np.float64))
            t -= np.floor(t)
            cs, sn = np.cos(2.0 * np.pi * t).astype(f), np.sin(2.0 * np.pi * t).astype(f)
            cr, ci = (d * cs).astype(f), (d * sn).astype(f)
        else:
            pr, pi = self.rot
            dr, di, Z = f(np.float32(self.cfg["pd"][0])), f(np.float32(self.cfg["pd"][1])), f(0)
            cr, ci, pos = np.empty(n, f), np.empty(n, f), 0
            blocks = [n] if blocks is None else blocks
            assert sum(blocks) == n, (blocks, n)
            for b in blocks:  # one call of the rotator per reference block
                for i in range(b):
                    dv = d[pos]
                    cr[pos], ci[pos] = (dv * pr) - (Z * pi), (dv * pi) + (Z * pr)
                    pr, pi = (pr * dr) - (pi * di), (pr * di) + (pi * dr)
                    pos += 1
                    if (i + 1) % RENORM == 0:
                        pr, pi = self._norm(pr, pi)
                if b % RENORM:
                    pr, pi = self._norm(pr, pi)
            self.rot = (pr, pi)
        self.cr.append(cr)
        self.ci.append(ci)
        before = self.nout(self.fed)
        self.fed += n
        self.counts.append(self.nout(self.fed) - before)

    def outputs(self):
        f, c = self.f, self.cfg
        cr = np.concatenate(self.cr) if self.cr else np.zeros(0, f)
        ci = np.concatenate(self.ci) if self.ci else np.zeros(0, f)
        if f == np.float64:
            y = cr + 1j * ci
            for D, taps in c["stages"]:
                y = _fir64(y, taps, D)
            if c["rtaps"] is not None:
                y = _poly(y, c["rtaps"], c["interp"], c["decim"], np.float64)
            return y
        for D, taps in c["stages"]:
            cr, ci = _fir32(cr, ci, taps, D)
        y = (cr + 1j * ci).astype(np.complex64)
        if c["rtaps"] is not None:
            y = _poly(y, c["rtaps"], c["interp"], c["decim"], np.float32)
        return y


# ---- 1. the restatement against the reference's recorded outputs: no context, no device, no oracle -----------------------------------------------
def cfg_of_desc(rd, exact=False):
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy()  # noqa: E731
    c = dict(stages=[(int(rd.stage_decim[i]), arr(rd.stage_taps[i], rd.stage_ntaps[i])) for i in range(rd.n_stages)], interp=int(rd.interp), decim=int(rd.decim),
             rtaps=arr(rd.resamp_taps, rd.resamp_ntaps) if rd.interp != rd.decim else None, pd=(np.float32(rd.phase_delta_re), np.float32(rd.phase_delta_im)),
             inv_dev=INV_DEV, exact=exact)
    c["key"] = (tuple((D, len(t), float(np.sum(np.abs(t.astype(np.float64))))) for D, t in c["stages"]), c["interp"], c["decim"], exact)
    return c


_prod_cache = {}


def product_cfg(exact=False, first_only=False):
    """radio.rds_desc(250e3): {8 x 44, 2 x 12, 2 x 69} and the 5000 / 7813 polyphase stage; first_only: its first stage alone"""
    from sdrplusplus_amd import radio

    if "rd" not in _prod_cache:
        _prod_cache["rd"] = radio.rds_desc(RATE)
    c = cfg_of_desc(_prod_cache["rd"][0], exact)
    if first_only:
        c.update(stages=c["stages"][:1], interp=1, decim=1, rtaps=None)
        c["key"] = (c["key"][0][:1], 1, 1, exact)
    return c


def restate_fixture(name, f):
    z = np.load(GOLDEN)
    x = (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
    r = Restate(product_cfg(exact=True), f, "rotator")
    pos = 0
    for b, n in enumerate(z[name + "_cut"]):
        if b in z[name + "_reset"]:
            r.reset()
        r.push(x[pos:pos + int(n)], on=bool(z[name + "_on"][b]))
        pos += int(n)
    return r, z[name + "_counts"], z[name + "_rds"].view(np.complex64).reshape(-1)


@pytest.mark.parametrize("name", ["steady", "cuts", "toggle_reset"])
def test_restatement_is_the_reference_per_sample(name):
    """CPU only.  In rotator form with the real description, in the fixture's blocks with its `on` flags and resets: the per-block output counts are the recorded
    ones exactly; the recorded float32 outputs take base32's place — their distance from the float64 restatement is the recorded figure (1.25 rule, BASELINE_MAX)."""
    r64, counts, want = restate_fixture(name, np.float64)
    assert r64.counts == [int(c) for c in counts], (name, r64.counts, counts)
    ref = r64.outputs()
    assert len(ref) == len(want) > 100
    fig = dist(want, ref)
    print("\n[rds rows] fixture %s: the reference's recorded outputs %.3g of the float64 restatement's RMS (%d samples)" % (name, fig, len(ref)))
    _note("fixture %s %.3g" % (name, fig))
    assert fig < BASELINE_MAX and fig <= 1.25 * BASELINES["fixture"][name], (name, fig, BASELINES["fixture"][name])


def _note(line):
    if os.environ.get("SDRPP_RDS_FIGURES"):  # (refilling BASELINES: one line per row and leg, appended to the named file)
        with open(os.environ["SDRPP_RDS_FIGURES"], "a") as fh:
            fh.write(line + "\n")


# ---- descriptions -----------------------------------------------------------------------------------------------------------------------------
_taps = {}


def first_taps(K, D):
    """K taps whose ends count: a _lp low-pass (cutoff 0.4 of the output rate) plus a fixed-seed perturbation of 0.15 .. 0.3 of its largest tap, the end taps pushed
    outwards; below 12 taps and at the largest K of a D a flat-topped random set (0.5 .. 1) normalised to unit DC gain."""
    if (K, D) not in _taps:
        rng = np.random.default_rng(1000 * D + K)
        if K < 12 or K >= kmax(D):
            h = rng.uniform(0.5, 1.0, K)
            h /= np.sum(h)
        else:
            lp = _lp(K, 0.4 * RATE / D, RATE).astype(np.float64)
            top = np.max(np.abs(lp))
            p = top * rng.uniform(0.15, 0.3, K) * rng.choice([-1.0, 1.0], K)
            for e in (0, K - 1):
                p[e] = abs(p[e]) * (1.0 if lp[e] >= 0 else -1.0)
            h = lp + p
        _taps[(K, D)] = np.ascontiguousarray(h, np.float32)
    return _taps[(K, D)]


def make_cfg(K, D, exact=False, taps=None):
    from sdrplusplus_amd import capi

    t = first_taps(K, D) if taps is None else taps
    c = dict(stages=[(D, t)], interp=1, decim=1, rtaps=None, pd=tuple(np.float32(v) for v in capi.design_phase_delta(-57000.0, RATE)), inv_dev=INV_DEV, exact=exact)
    c["key"] = (((D, K, float(np.sum(np.abs(t.astype(np.float64))))),), 1, 1, exact)
    return c


def rds_desc_of(cfg):
    from sdrplusplus_amd import capi, radio

    r, keep = capi.RdsDesc(), []
    r.phase_delta_re, r.phase_delta_im = cfg["pd"]
    r.n_stages = len(cfg["stages"])
    for i, (D, taps) in enumerate(cfg["stages"]):
        t = np.ascontiguousarray(taps, np.float32)
        keep.append(t)
        r.stage_decim[i], r.stage_ntaps[i], r.stage_taps[i] = D, len(t), radio._fp(t)
    r.interp, r.decim, r.resamp_ntaps = cfg["interp"], cfg["decim"], 0
    if cfg["rtaps"] is not None:
        rt = np.ascontiguousarray(cfg["rtaps"], np.float32)
        keep.append(rt)
        r.resamp_ntaps, r.resamp_taps = len(rt), radio._fp(rt)
    return r, keep


def wfm_desc(case, cfg=None):
    """the VFO in front of the branch: the case's chain (None: the identity) as a WFM demodulator without audio low-pass; cfg None: the RAW twin"""
    from sdrplusplus_amd import radio

    d, keep, rate = hand_desc(case["sr"], 0.0, *(case["chain"] or ()))
    assert rate == RATE
    if cfg is not None:
        d.demod, d.inv_deviation = radio.DEMOD_CODES["WFM"], INV_DEV
        d.nco_mode = 2 if cfg["exact"] else 0
    return d, keep


# ---- the planner's cutting and the branch's bookkeeping, restated (plan_vfo.h rds_branch, vfo_ctl.h rds_freeze) ---------------------------------
def plan(ops, K, D, exact):
    """-> dict(tiles {(outputs of the tile, is the job's last)}, jobs per push, soffs at push starts, frozen / hist outputs, line jobs [(n, rounds)],
    freezes [(stand-alone launch?, rounds)]) from the schedule alone"""
    geo = rds_tile_geometry(K, D)
    tile = geo[0] if geo else 0
    o = dict(tiles=set(), jobs=[], soffs=[], frozen_out=0, hist_out=0, lines=[], freezes=[], fed=[], mq=[])
    attached = on = frozen = False
    so = fed_row = 0
    for op in ops:
        if op[0] == "attach":
            attached, on, frozen, fed_row, so = True, True, True, 0, 0
        elif op[0] in ("off", "reset", "replace"):
            if attached and on and not exact:  # rds_freeze
                if not frozen:
                    o["freezes"].append((True, (K + CHUNK - 1) // CHUNK))
                else:
                    o["freezes"].append((False, 0))
                frozen, fed_row = True, 0
            if op[0] == "off":
                on = False
        elif op[0] == "on":
            on = True
        elif op[0] == "push" and attached and on:
            n = op[1]
            mq = (n - so + D - 1) // D if n > so else 0
            o["soffs"].append(so)
            o["fed"].append(n)
            o["mq"].append(mq)
            so = so + mq * D - n
            if exact:
                continue
            nj = 0
            for a in range(0, mq, SEG_TILES * tile):
                hi = min(a + SEG_TILES * tile, mq)
                nj += 1
                for m0 in range(a, hi, tile):
                    o["tiles"].add((min(tile, hi - m0), hi - a))
            o["jobs"].append(nj)
            o["frozen_out" if frozen else "hist_out"] += mq
            if frozen and n > 0:
                fed_row += n
                if fed_row >= K:
                    frozen = False
                else:
                    o["lines"].append((n, (K + CHUNK - 1) // CHUNK))
    return o


def nvalid(cnt, K, D):
    return (cnt - 1) * D + K


# ---- inputs and rows --------------------------------------------------------------------------------------------------------------------------
def signal(n, seed, sr=RATE, spikes=()):
    """test_rds.py's broadcast carrier at offset 0: 75 kHz deviation, amplitude 0.5, audio, pilot and the biphase 57 kHz subcarrier"""
    x = broadcast(n, seed, sr=sr, f0=0.0).copy()
    for i, v in spikes:
        x[i] += np.complex64(v)
    return x


class Row:
    """build() -> dict(x, sr, chain, jobs [cfg], ops, ref_block, edge (callable(case, plans) with the row's own CPU assertions), ends (the end-tap condition is
    demanded)); `why`: the edge the row places; family: front / push / line / rotator / bank."""

    def __init__(self, rid, family, why, build, identity=True, group=4):
        self.id, self.family, self.why, self.build, self.identity, self.group = rid, family, why, build, identity, group


def pushes(cuts):
    return [("push", int(n)) for n in cuts]


def _full_and_partial(case, plans):
    """every geometry row: a full tile, a tile that is not full (where a tile holds more than one output) and a push of more than one job"""
    K, D = case["K"], case["D"]
    tile = rds_tile_geometry(K, D)[0]
    cnts = {c for c, _ in plans[0]["tiles"]}
    assert tile in cnts and (tile == 1 or any(c < tile for c in cnts)) and max(plans[0]["jobs"]) >= 2, (tile, cnts, plans[0]["jobs"])


def _geom(K, D, cuts, edge=None, seed=1, taps=None, ends=True):
    def build():
        def e(case, plans):
            _full_and_partial(case, plans)
            if edge:
                edge(case, plans)
        cfg = make_cfg(K, D, taps=taps() if taps else None)
        return dict(x=signal(sum(cuts), seed), jobs=[cfg], ops=[("attach",)] + pushes(cuts), edge=e, ends=ends, K=K, D=D)
    return build


def _edge_k12(case, plans):
    p = plans[0]
    assert rds_tile_geometry(12, 2) == (64, 72) and SEG_TILES * 64 == 256
    q = p["mq"].index(577)  # two full jobs of 256 outputs, a job of 65: a full tile and a last tile of ONE output
    assert p["jobs"][q] == 3 and {(64, 256), (64, 65), (1, 65)} <= p["tiles"], p["tiles"]


def _edge_round(target):
    def edge(case, plans):
        K, D = case["K"], case["D"]
        tile = rds_tile_geometry(K, D)[0]
        assert nvalid(tile, K, D) + 1 == target and target in (LOAD_ROUND, LOAD_ROUND + 1, LOAD_ROUND + 2), (K, D, tile, nvalid(tile, K, D))
    return edge


def _edge_chunk(target):
    def edge(case, plans):
        K, D = case["K"], case["D"]
        tile = rds_tile_geometry(K, D)[0]
        assert nvalid(tile, K, D) == target and target in (3 * CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 1), (K, D, tile, nvalid(tile, K, D))
    return edge


def _edge_small(case, plans):
    K, D = case["K"], case["D"]
    assert K <= D + 1 and (K - 1) >> (D.bit_length() - 1) <= 1  # the window's rows hold the tile's outputs and at most one element more


def _edge_odd_pitch(case, plans):
    K, D = case["K"], case["D"]
    tile, pitch = rds_tile_geometry(K, D)
    assert D >= 16 and pitch % 2 == 1
    if (K, D) == (128, 128):
        assert (tile, pitch) == (1, 1)


def _edge_kmax(case, plans):
    K, D = case["K"], case["D"]
    assert K == KMAX[D] == kmax(D) and rds_tile_geometry(K + 1, D) is None
    tile, pitch = rds_tile_geometry(K, D)
    assert 2 * D * pitch + nvalid(tile, K, D) + 1 <= LDS_WAVE  # window and phases, inside the wavefront's share


def _cuts(K, n, big):
    """warm past K (the set-aside line alone), then the history path: a long push, one sample, seven, the rest"""
    c = [K + 5, big, 1, 7]
    return c + [n - sum(c)]


def _product():
    def build():
        cuts = _cuts(44, 6000, 2931)
        return dict(x=signal(6000, 2), jobs=[product_cfg()], ops=[("attach",)] + pushes(cuts), edge=_full_and_partial, ends=False, K=44, D=8)
    return build


def _push_row(ifcuts, edge, seed):
    """behind a one-tap /2 stage at 500 kS/s (a launch group forms only behind a decimator): the IF is every second input sample"""
    def build():
        n = sum(ifcuts)
        cfg = make_cfg(44, 8)
        return dict(x=signal(2 * n, seed, sr=2 * RATE), sr=2 * RATE, chain=([(2, np.ones(1, np.float32))],), jobs=[cfg], ops=[("attach",)] + pushes(ifcuts), edge=edge,
                    ends=True, K=44, D=8)
    return build


SOFF_CUTS = [49] + [9] * 9 + [801, 15, 15, 15, 15, 1000, 3, 5, 11, 13, 300]


def _edge_soff(case, plans):
    assert set(plans[0]["soffs"]) == set(range(8)), sorted(set(plans[0]["soffs"]))  # a push starts at every residue of D


SHORT_CUTS = [50, 1, 1, 1, 3, 2, 7, 1, 1, 5, 1, 1, 1, 1, 1, 1, 900, 1, 2, 1, 4, 7, 7, 1, 1000, 1, 1, 1, 6]


def _edge_short(case, plans):
    p = plans[0]
    none = [n for n, m in zip(p["fed"], p["mq"]) if m == 0]
    assert 1 in none and max(none) >= 5 and len(none) >= 8, none                # pushes shorter than D without an output, 1-sample pushes among them
    assert any(n == 1 and m == 1 for n, m in zip(p["fed"], p["mq"])), p["mq"]   # and a 1-sample push that holds an output


# the line family: behind each switch one of four patterns, dealt round the rows so that the five rows hold every (switch, pattern) pair
SWITCHES = ("attach", "offon", "reset", "replace")
PATTERNS = ("km1_1", "exact_k", "second_switch", "off_frozen")
LINE_KD = [(64, 8), (65, 2), (128, 8), (129, 2), (200, 8)]


def _pieces(total, k):
    base = [total // k] * k
    base[-1] += total - sum(base)
    return [b for b in base if b > 0]


def _switch(s):
    return {"offon": [("off",), ("push", 50), ("on",)], "reset": [("reset",)], "replace": [("replace",)]}[s]


def line_ops(K, row):
    ops, pairs = [("push", 300), ("attach",)], []  # (the stream has a history before the attach)
    bulk = pushes([K + 8, 40])                     # the line leaves force; then a push on the history path
    for si, s in enumerate(SWITCHES):
        pat = PATTERNS[(row + si) % 4]
        pairs.append((s, pat))
        if s != "attach":
            ops += _switch(s)
        if pat == "km1_1":
            ops += pushes(_pieces(K - 1, 3)) + [("push", 1)]
        elif pat == "exact_k":
            ops += pushes(_pieces(K, 2))
        elif pat == "second_switch":
            ops += [("push", K // 2)] + _switch(SWITCHES[1 + (row + si) % 3]) + pushes(_pieces(K - 1, 2)) + [("push", 1)]
        else:
            ops += [("push", K // 3), ("off",), ("push", 40), ("on",), ("push", K // 2)]
        ops += bulk
    total = sum(o[1] for o in ops if o[0] == "push")
    if total < 2000:
        ops += pushes([2000 - total])
    return ops, pairs


LINE_SEEDS = [21, 21, 22, 23, 24]  # (chosen so that the phase steps behind the resets keep their distance from pi: check_row asserts it)


def _line(i):
    K, D = LINE_KD[i]

    def build():
        ops, pairs = line_ops(K, i)

        def edge(case, plans):
            p = plans[0]
            rounds = (K + CHUNK - 1) // CHUNK
            assert p["lines"] and all(r == rounds for _n, r in p["lines"]) and (rounds == 1) == (K == CHUNK) and rounds == {64: 1, 65: 2, 128: 2, 129: 3, 200: 4}[K], (K, p["lines"])
            assert sum(1 for alone, _r in p["freezes"] if alone) >= 2          # rds_freeze's stand-alone launch, the same rounds
            assert any(not alone for alone, _r in p["freezes"])                # a switch that met the line in force
        return dict(x=signal(sum(o[1] for o in ops if o[0] == "push"), LINE_SEEDS[i]), jobs=[make_cfg(K, D)], ops=ops, edge=edge, ends=True, K=K, D=D, pairs=pairs)
    return build


ROT_BLOCKS = (1, 63, 64, 65, 511, 512, 513, 1024, 1250)


def rot_cuts(B):
    """whole reference blocks per push — several where a block is short — and a partial last block"""
    m = [max(1, round(700 / B)), max(2, round(900 / B)), max(1, round(500 / B))]
    return [m[0] * B, m[1] * B, m[2] * B + (B // 3)]


def _rot(B):
    def build():
        cuts = rot_cuts(B)

        def edge(case, plans):
            chunks = {min(CHUNK, B - c) for c in range(0, B, CHUNK)}  # the rotator's chunks inside a whole block
            assert all(n % B == 0 for n in cuts[:-1]) and cuts[-1] % B == B // 3 and (B == 1 or B // 3 > 0)  # whole blocks, and a partial last one
            assert len(cuts) == 3 and (cuts[1] // B >= 2)                                                      # a push of several blocks
            want = {1: {1}, 63: {63}, 64: {64}, 65: {64, 1}, 511: {64, 63}, 512: {64}, 513: {64, 1}, 1024: {64}, 1250: {64, 34}}[B]
            assert chunks == want, (B, chunks)
            assert (B % RENORM == 0) == (B in (512, 1024))  # the block's end IS a periodic renormalisation: none is added
        cfg = product_cfg(exact=True, first_only=True)
        return dict(x=signal(sum(cuts), 40 + B % 17), jobs=[cfg], ops=[("attach",)] + pushes(cuts), ref_block=B, edge=edge, ends=False, K=44, D=8)
    return build


BANK_KD = [(12, 2, False), (44, 8, True), (200, 8, False), (44, 32, False), (130, 2, False)]


def _bank():
    def build():
        cuts = [210, 1500, 10, 1287]  # (whole reference blocks of 10 in every push but the last: the rotator VFO's one push has the same blocks)
        jobs = [make_cfg(K, D, exact=ex) for K, D, ex in BANK_KD]

        def edge(case, plans):
            assert len(plans) == 5 and sum(c["exact"] for c in case["jobs"]) == 1
            assert len({rds_tile_geometry(K, D) for K, D, _e in BANK_KD}) >= 4  # different tiles and pitches side by side in a workgroup
        return dict(x=signal(sum(cuts), 60), jobs=jobs, ops=[("attach",)] + pushes(cuts), ref_block=10, edge=edge, ends=True, K=None, D=None, alone=True)
    return build


def _ifc():
    def build():
        from sdrplusplus_amd import radio

        cuts = _cuts(44, 3000, 1400)
        ifd = radio.if_desc(RATE, squelch=-150.0)  # (the squelch enabled and open: the chain runs and delivers the input)

        def edge(case, plans):
            _bits_equal(case["ifs"].view(np.float32), case["x"].view(np.float32), "the open chain delivers the input")
        return dict(x=signal(3000, 70), jobs=[make_cfg(44, 8)], ops=[("attach",)] + pushes(cuts), ifd=ifd, edge=edge, ends=True, K=44, D=8)
    return build


def G(K, D, why, cuts=None, edge=None, **kw):
    n = 2400 if D <= 8 else (3200 if D == 16 else 4000 if D <= 64 else 6000)
    return Row("k%d_d%d" % (K, D), "front", "K = %d, D = %d: %s" % (K, D, why), _geom(K, D, cuts or _cuts(K, n, n // 2 + 3), edge, **kw))


ROWS = [
    # ---- front geometry ----
    Row("product", "front", "the product's K = 44, D = 8 (tile 29, pitch 34) with the whole real chain behind it: 2 x 12, 2 x 69 and the 5000 / 7813 stage", _product()),
    G(12, 2, "tile 64, a job of 256 outputs; a push of 577 outputs = two full jobs, a partial one, a last tile of one output", [20, 1154, 1, 7, 1218], _edge_k12),
    G(129, 2, "the loader's round: nvalid + 1 = 256, the last round exactly full", edge=_edge_round(256)),
    G(130, 2, "the loader's round: nvalid + 1 = 257, one element in a second round", edge=_edge_round(257)),
    G(131, 2, "the loader's round: nvalid + 1 = 258", edge=_edge_round(258)),
    G(3, 4, "the loader's round at D = 4: nvalid + 1 = 256", edge=_edge_round(256)),
    G(4, 4, "the loader's round at D = 4: nvalid + 1 = 257", edge=_edge_round(257)),
    G(5, 4, "the loader's round at D = 4: nvalid + 1 = 258", edge=_edge_round(258)),
    G(65, 2, "the difference chunk: nvalid = 191, the third chunk one short", edge=_edge_chunk(191)),
    G(66, 2, "the difference chunk: nvalid = 192, three chunks exactly", edge=_edge_chunk(192)),
    G(67, 2, "the difference chunk: nvalid = 193, one element in a fourth chunk", edge=_edge_chunk(193)),
    G(1, 2, "one tap: no history at all, the window is the tile's own samples", edge=_edge_small),
    G(8, 8, "K = D: every window row holds exactly the tile's outputs", edge=_edge_small),
    G(9, 8, "K = D + 1: one row holds one element more", edge=_edge_small),
    G(44, 16, "D >= 16: the odd-pitch branch", edge=_edge_odd_pitch),
    G(44, 32, "D = 32, odd pitch", edge=_edge_odd_pitch),
    G(64, 64, "K = D = 64, odd pitch", edge=_edge_odd_pitch),
    G(128, 128, "the tile of ONE output, pitch 1: a job is four outputs", edge=_edge_odd_pitch),
    G(272, 2, "the largest K at D = 2: K + 1 has no tile", edge=_edge_kmax),
    G(272, 8, "the largest K at D = 8", edge=_edge_kmax),
    G(255, 32, "the largest K at D = 32", edge=_edge_kmax),
    G(192, 64, "the largest K at D = 64", edge=_edge_kmax),
    # ---- push structure (behind a /2 stage: launch groups form) ----
    Row("soff_walk", "push", "pushes of 9 and 15 IF samples walk soff through every residue of D = 8; grouped, the same cuts are one launch", _push_row(SOFF_CUTS, _edge_soff, 5), identity=False, group=4),
    Row("short_pushes", "push", "pushes shorter than D without an output, 1-sample pushes with and without one; grouped by 3", _push_row(SHORT_CUTS, _edge_short, 6), identity=False, group=3),
    # ---- the set-aside line ----
    Row("line_k64", "line", "K = 64, D = 8: the line body's ONE round exactly full; attach, off/on, reset, replace each followed by a pattern of short pushes", _line(0)),
    Row("line_k65", "line", "K = 65, D = 2: one element in the line body's second round (planner job and rds_freeze's launch)", _line(1)),
    Row("line_k128", "line", "K = 128, D = 8: two rounds exactly", _line(2), group=3),
    Row("line_k129", "line", "K = 129, D = 2: a third round of one element", _line(3)),
    Row("line_k200", "line", "K = 200, D = 8: four rounds, the last partial", _line(4)),
    # ---- the reference rotator ----
] + [Row("rot_b%d" % B, "rotator", "nco_mode = 2, reference blocks of %d IF samples: %s.  At the bar's level this catches a lost state, a skipped or misplaced normalisation, "
         "a wrong chunk edge — not a normalisation done twice (1 ulp)" % (B, why), _rot(B))
     for B, why in ((1, "every sample is a block and ends in a normalisation"), (63, "a block one short of the 64-sample chunk"), (64, "a block of exactly one chunk"),
                    (65, "a chunk and a chunk of one sample"), (511, "one short of the renormalisation period: the end-of-block one applies"),
                    (512, "the block's end coincides with the periodic renormalisation: no second one"), (513, "a periodic renormalisation, then a block end one sample on"),
                    (1024, "two periods exactly"), (1250, "the product's block: two periods and 226 samples"))] + [
    # ---- a bank ----
    Row("bank5", "bank", "five VFOs, first stages (12,2), (44,8) in nco_mode = 2, (200,8), (44,32), (130,2): jobs of different tiles side by side, each VFO equal to itself alone", _bank()),
    # ---- behind the IF chain ----
    Row("ifc_open", "front", "K = 44, D = 8 behind the IF chain (squelch enabled and open): the branch reads the chain's stream, the restatement what vfo_ifc_read delivered", _ifc(), identity=False),
]
PIPED = ("product", "k12_d2", "k130_d2", "k128_d128", "k272_d8", "soff_walk", "short_pushes", "line_k65", "line_k128", "line_k200", "rot_b65", "rot_b512", "rot_b1250", "bank5", "ifc_open")

# dist(the reference's recorded outputs, ref64) per fixture case, and the float32 sequential baselines per row and VFO, measured by this file's own CPU run of the
# restatement: {row: [per VFO (emulator leg, device leg)]}.  Rows whose IF is the input (or every second input sample) have one figure for both legs.
BASELINES = {
    "fixture": {"steady": 5.62e-06, "cuts": 2.58e-06, "toggle_reset": 4.59e-06},
    "product": [(1.41e-06, 1.41e-06)],
    "k12_d2": [(1.22e-06, 1.22e-06)],
    "k129_d2": [(1.08e-06, 1.08e-06)],
    "k130_d2": [(6.92e-07, 6.92e-07)],
    "k131_d2": [(8.72e-07, 8.72e-07)],
    "k3_d4": [(7.86e-07, 7.86e-07)],
    "k4_d4": [(1.42e-06, 1.42e-06)],
    "k5_d4": [(1.27e-06, 1.27e-06)],
    "k65_d2": [(5.62e-07, 5.62e-07)],
    "k66_d2": [(6.77e-07, 6.77e-07)],
    "k67_d2": [(1.06e-06, 1.06e-06)],
    "k1_d2": [(9.84e-07, 9.84e-07)],
    "k8_d8": [(1.62e-06, 1.62e-06)],
    "k9_d8": [(1.72e-06, 1.72e-06)],
    "k44_d16": [(7.03e-07, 7.03e-07)],
    "k44_d32": [(1.45e-06, 1.45e-06)],
    "k64_d64": [(1.24e-06, 1.24e-06)],
    "k128_d128": [(9.11e-07, 9.11e-07)],
    "k272_d2": [(1.45e-06, 1.45e-06)],
    "k272_d8": [(1.39e-06, 1.39e-06)],
    "k255_d32": [(1.4e-06, 1.4e-06)],
    "k192_d64": [(1.87e-06, 1.87e-06)],
    "soff_walk": [(1.57e-06, 1.57e-06)],
    "short_pushes": [(1.55e-06, 1.55e-06)],
    "line_k64": [(1.16e-06, 1.16e-06)],
    "line_k65": [(5.83e-07, 5.83e-07)],
    "line_k128": [(1.06e-06, 1.06e-06)],
    "line_k129": [(1.1e-06, 1.1e-06)],
    "line_k200": [(1.22e-06, 1.22e-06)],
    "rot_b1": [(2.76e-06, 2.76e-06)],
    "rot_b63": [(3.16e-06, 3.16e-06)],
    "rot_b64": [(2.96e-06, 2.96e-06)],
    "rot_b65": [(2.93e-06, 2.93e-06)],
    "rot_b511": [(3.07e-06, 3.07e-06)],
    "rot_b512": [(2.36e-06, 2.36e-06)],
    "rot_b513": [(2.42e-06, 2.42e-06)],
    "rot_b1024": [(3.66e-06, 3.66e-06)],
    "rot_b1250": [(3.53e-06, 3.53e-06)],
    "bank5": [(1.31e-06, 1.31e-06), (2.53e-06, 2.53e-06), (1.83e-06, 1.83e-06), (1.32e-06, 1.32e-06), (8.69e-07, 8.69e-07)],
    "ifc_open": [(1.85e-06, 1.85e-06)],
}


# ---- running ----------------------------------------------------------------------------------------------------------------------------------
_cases = {}


def prepare(row):
    if row.id not in _cases:
        case = row.build()
        for k, v in (("sr", RATE), ("chain", None), ("ref_block", 0), ("ifd", None), ("alone", False)):
            case.setdefault(k, v)
        case["scale"] = int(round(case["sr"] / RATE))
        assert sum(o[1] for o in case["ops"] if o[0] == "push") * case["scale"] == len(case["x"])
        assert [o[0] for o in case["ops"]].count("attach") == 1
        case["plain"] = all(o[0] in ("attach", "push") for o in case["ops"]) and case["ops"][0][0] == "attach"
        _cases[row.id] = case
    return dict(_cases[row.id])


LAG = 16  # results are taken this many pushes behind (SDRPP_RESULT_SLOTS is 24)


def run(case, ops, pipelined=False, group=0, only=None):
    """-> dict(out=[per VFO complex64], counts=[per VFO [outputs per push]], ifs (the stream the branch was fed, ordinary runs), forms, stats, groups); only: that
    VFO alone.  Pipelined runs go pipelined behind the attach (test_rds.py's order)."""
    from sdrplusplus_amd import capi

    sc = case["scale"]
    sizes = [o[1] * sc for o in ops if o[0] == "push"]
    mp = max(sum(sizes[i:i + max(1, group)]) for i in range(len(sizes)))
    ctx = capi.Context(0, max_push=max(mp, 256))
    ctx.set_reference_block(case["ref_block"] * sc)
    jobs = case["jobs"] if only is None else [case["jobs"][only]]
    vids, descs, rds = [], [], []
    for cfg in jobs:
        d, keep = wfm_desc(case, cfg)
        vids.append(ctx.vfo_add(d, keep))
        descs.append((d, keep))
        rds.append(rds_desc_of(cfg))
        if case["ifd"] is not None:
            ctx.vfo_set_if(vids[-1], case["ifd"])
    twin = None
    if case["chain"]:
        d, keep = wfm_desc(case)
        twin = ctx.vfo_add(d, keep)
    out, ifs, pending = [[] for _ in vids], [], []  # pending: (ticket, the handles at that push, the branch on?)
    attached = on = False
    data, cnt = capi.c_float_p(), C.c_int()

    def take():
        tk, hs, was_on = pending.pop(0)
        ctx.result_wait(tk)
        for k, v in enumerate(hs):
            rc = ctx.L.sdrpp_result_rds(ctx.h, tk, v, C.byref(data), C.byref(cnt))
            assert rc == (0 if was_on else NOT_FOUND), (tk, k, rc)
            out[k].append(ctx.result_rds(tk, v) if was_on else np.zeros(0, np.complex64))
        ctx.result_release(tk)

    pos = tickets = 0
    for op in ops:
        if op[0] == "push":
            ctx.push(case["x"][pos:pos + op[1] * sc])
            pos += op[1] * sc
            if pipelined and attached:
                tickets += 1
                pending.append((tickets, list(vids), on))
                if len(pending) > LAG:
                    take()
                continue
            for k, v in enumerate(vids):
                out[k].append(ctx.vfo_rds_read(v).copy() if attached else np.zeros(0, np.complex64))
            if twin is not None:
                ifs.append(np.ascontiguousarray(ctx.vfo_read(twin)).copy().view(np.complex64).reshape(-1))
            elif case["ifd"] is not None:
                ifs.append(ctx.vfo_ifc_read(vids[0]).copy())
            else:
                ifs.append(ctx.vfo_read_if(vids[0]).copy())
        elif op[0] == "attach":
            for v, (rd, rkeep) in zip(vids, rds):
                ctx.vfo_set_rds(v, rd, True, rkeep)
            attached = on = True
            if pipelined:
                ctx.set_pipelined(True, 1 | 32)
                if group:
                    ctx.set_pipeline_group(group)
        elif op[0] in ("on", "off"):
            on = op[0] == "on"
            for v, (rd, rkeep) in zip(vids, rds):
                ctx.vfo_set_rds(v, rd, on, rkeep)
        elif op[0] == "reset":
            for v in vids:
                ctx.vfo_reset(v)
        else:
            assert op[0] == "replace", op
            vids = [ctx.vfo_replace(v, d, 3, keep) for v, (d, keep) in zip(vids, descs)]
    while pending:
        take()
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    gs = ctx.pipeline_group_stats() if (pipelined and group) else None
    if pipelined:
        ctx.set_pipelined(False)
    ctx.close()
    return dict(out=[np.concatenate(o) for o in out], counts=[[len(p) for p in o] for o in out], ifs=np.concatenate(ifs) if ifs else None, forms=forms, stats=st, groups=gs,
                tickets=tickets)


_restated = {}


def restated(row, case, j, y, leg):
    """(ref64, base32, the float64 Restate) of VFO j over the IF y in the case's schedule; computed once per row, description and leg and left unchanged"""
    cfg = case["jobs"][j]
    key = (row.id, cfg["key"], "cpu" if row.identity or case["chain"] else leg)
    if key not in _restated:
        res = []
        for f in (np.float64, np.float32):
            r = Restate(cfg, f, "rotator" if cfg["exact"] else "closed")
            pos, attached, on = 0, False, False
            for op in case["ops"]:
                if op[0] == "push":
                    n, B = op[1], case["ref_block"]
                    blocks = ([B] * (n // B) + ([n % B] if n % B else [])) if B else None
                    r.push(y[pos:pos + n], on=attached and on, blocks=blocks)
                    pos += n
                elif op[0] == "attach":
                    attached = on = True
                elif op[0] in ("on", "off"):
                    on = op[0] == "on"
                elif op[0] == "reset":
                    r.reset()
            assert pos == len(y)
            o = r.outputs()
            o.setflags(write=False)
            res.append((o, r))
        _restated[key] = (res[0][0], res[1][0], res[0][1], res[1][1])
    return _restated[key]


def check_row(row, case, leg):
    """The CPU check of a row, before its outputs are looked at -> [(ref64, base32, counts)] per VFO"""
    out, plans = [], []
    for j, cfg in enumerate(case["jobs"]):
        o64, o32, r64, r32 = restated(row, case, j, case["ifs"], leg)
        for r in (r64, r32):
            assert r.qmargin >= MIN_WRAP_MARGIN, (row.id, j, "a phase step comes too close to pi", r.qmargin)
            assert r.xmin >= MIN_X, (row.id, j, "the envelope comes too close to zero", r.xmin)
        assert r64.wraps >= 1 and r64.wraps == r32.wraps, (row.id, j, r64.wraps, r32.wraps)
        assert r64.counts == r32.counts and len(o64) == sum(r64.counts)
        assert rms(o64) >= MIN_RMS, (row.id, j, rms(o64))
        D, h = cfg["stages"][0]
        if case["ends"]:
            assert min(abs(float(h[0])), abs(float(h[-1]))) >= END_TAPS * float(np.max(np.abs(h))), (row.id, j, h[0], h[-1], np.max(np.abs(h)))
        p = plan(case["ops"], len(h), D, cfg["exact"])
        if not cfg["exact"]:
            assert p["frozen_out"] > 0 and p["hist_out"] > 0, (row.id, j, "both the set-aside line and the stream's history must feed outputs", p["frozen_out"], p["hist_out"])
        plans.append(p)
        out.append((o64, o32, r64.counts))
    n_if = len(case["ifs"])
    assert 2000 <= n_if <= 6000, (row.id, n_if)
    if case.get("edge"):
        case["edge"](case, plans)
    return out


_alone = {}


def alone(backend, row, case, j):
    key = (backend, row.id, j)
    if key not in _alone:
        _alone[key] = run(case, case["ops"], only=j)["out"][0]
        _alone[key].setflags(write=False)
    return _alone[key]


def _same(a, b, what):
    for j, (p, q) in enumerate(zip(a["out"], b["out"])):
        _bits_equal(p.view(np.float32), q.view(np.float32), "%s, VFO %d" % (what, j))
    assert a["counts"] == b["counts"], what


def known_if(case):
    return case["x"] if not case["chain"] else np.ascontiguousarray(case["x"][::case["scale"]])


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_rds_sample_by_sample(backend, row):
    case = prepare(row)
    early = case["ifd"] is None
    if early:  # the row's edge on the CPU before anything runs on a device: the IF is the input (every second input sample behind the one-tap stage)
        case["ifs"] = known_if(case)
        checked = check_row(row, case, backend)
    a = run(case, case["ops"])
    if early:
        _bits_equal(a["ifs"].view(np.float32), case["ifs"].view(np.float32), "%s: the IF is the input" % row.id)
    else:
        case["ifs"] = a["ifs"]
        checked = check_row(row, case, backend)
    for j in range(len(case["jobs"])):
        assert a["counts"][j] == checked[j][2], (row.id, j, "outputs per push", a["counts"][j], checked[j][2])
    assert a["forms"].get("ifc", 0) > 0, a["forms"]
    if case["plain"]:
        n = sum(o[1] for o in case["ops"] if o[0] == "push")
        b = run(case, [("attach",), ("push", n)])
        for j, cfg in enumerate(case["jobs"]):
            if cfg["exact"]:
                _bits_equal(a["out"][j].view(np.float32), b["out"][j].view(np.float32), "%s: one push vs whole reference blocks per push, VFO %d" % (row.id, j))
            else:
                rel = rms(b["out"][j] - a["out"][j]) / rms(a["out"][j])
                assert len(b["out"][j]) == len(a["out"][j]) and rel < 1e-6, (row.id, j, "one push vs the row's cuts", rel)
    if row.id in PIPED:
        c = run(case, case["ops"], pipelined=True)
        d = run(case, case["ops"], pipelined=True, group=row.group)
        _same(a, c, "%s: pipelined vs ordinary passes" % row.id)
        _same(a, d, "%s: launch groups of %d vs ordinary passes" % (row.id, row.group))
        for r, what in ((c, "pipelined"), (d, "grouped")):
            st = r["stats"]
            assert st["pass_blocks"] == 0 and st["tick_blocks"] == r["tickets"] > 0, (row.id, what, st)
            assert st["roles"].get("ifc", 0) > 0, (row.id, what, st["roles"])
        if case["chain"]:  # (a chain without a decimator stage goes out one push per launch)
            assert d["groups"]["multi_groups"] >= 2 and d["groups"]["largest"] == row.group, d["groups"]
    if case["alone"]:
        for j in range(len(case["jobs"])):
            _bits_equal(a["out"][j].view(np.float32), alone(backend, row, case, j).view(np.float32), "%s: VFO %d in the bank vs alone in its context" % (row.id, j))
    figs = []
    for j in range(len(case["jobs"])):
        o64, o32, _c = checked[j]
        base, e = dist(o32, o64), dist(a["out"][j], o64)
        figs.append((base, e))
        print("\n[rds rows %s VFO %d] %s per-sample max-abs / rms: baseline %.3g library %.3g (bar %.3g) over %d outputs" % (row.id, j, backend, base, e, MARGIN * base, len(o64)), end="")
    print()
    _note("%s %s %s" % (row.id, backend, " ".join("%.3g:%.3g" % be for be in figs)))
    for j, (base, e) in enumerate(figs):
        assert base < BASELINE_MAX, ("ill-conditioned input: float32 sequential baseline", row.id, j, base)
        at = int(np.argmax(np.abs(a["out"][j].astype(np.complex128) - checked[j][0])))
        assert e <= MARGIN * base, (row.id, "VFO %d: %.3g against a float32 sequential baseline of %.3g" % (j, e, base), "worst output", at)
        rec = BASELINES[row.id][j][backend == "gpu"]
        assert base <= 1.25 * rec, ("the float32 sequential baseline moved up: the bar may not loosen unseen", row.id, j, backend, base, rec)


def test_every_row_states_its_edge_and_the_table_is_complete():
    ids = [r.id for r in ROWS]
    assert len(set(ids)) == len(ids) and all(len(r.why) > 8 for r in ROWS) and set(PIPED) <= set(ids)
    assert sorted(BASELINES) == sorted(ids + ["fixture"]), (set(ids) ^ set(BASELINES))
    assert len(ROWS) // 3 <= len(PIPED)
    fam = {r.id: r.family for r in ROWS}
    assert {fam[i] for i in PIPED} == {"front", "push", "line", "rotator", "bank"} == set(fam.values())
    kd, pairs, blocks = set(), set(), set()
    for r in ROWS:
        case = prepare(r)
        n = len(case["x"]) // case["scale"]
        assert 2000 <= n <= 6000, (r.id, n)
        assert len(BASELINES[r.id]) == len(case["jobs"]), r.id
        if r.family == "front" and case["K"]:
            kd.add((case["K"], case["D"]))
        if r.family == "line":
            pairs |= set(case["pairs"])
        if r.family == "rotator":
            blocks.add(case["ref_block"])
    want = {(44, 8), (12, 2), (129, 2), (130, 2), (131, 2), (3, 4), (4, 4), (5, 4), (65, 2), (66, 2), (67, 2), (1, 2), (8, 8), (9, 8), (44, 16), (44, 32), (64, 64), (128, 128),
            (272, 2), (272, 8), (255, 32), (192, 64)}
    assert want <= kd, want - kd
    assert pairs == {(s, p) for s in SWITCHES for p in PATTERNS}, pairs  # every pattern behind every switch
    assert blocks == set(ROT_BLOCKS)
    assert rds_tile_geometry(44, 8) == (29, 34) and nvalid(29, 44, 8) == 268  # what the product runs


def test_constants_are_the_headers(backend):
    """rds_tile_geometry and SDRPP_WAVE_LDS_FLOATS as the library enforces them: for every D the largest K with a tile is taken by sdrpp_vfo_set_rds, K + 1 is
    refused as unsupported in closed form and taken with nco_mode = 2, where no tile is needed.  kRdsSegTiles, the loader's round, the chunk and the rotator's
    period have no such surface: they are restated above under the names the sources give them."""
    from sdrplusplus_amd import capi

    assert {D: kmax(D) for D in KMAX} == KMAX
    ctx = capi.Context(0, max_push=4096)
    case = dict(sr=RATE, chain=None)
    for D, K in KMAX.items():
        for k, exact, want in ((K, False, 0), (K + 1, False, UNSUPPORTED), (K + 1, True, 0)):
            cfg = make_cfg(k, D, exact=exact, taps=np.full(k, 1.0 / k, np.float32))
            d, keep = wfm_desc(case, cfg)
            vid = ctx.vfo_add(d, keep)
            rd, rkeep = rds_desc_of(cfg)
            assert ctx.L.sdrpp_vfo_set_rds(ctx.h, vid, C.byref(rd), 1) == want, (D, k, exact, want)
            ctx.vfo_remove(vid)
    ctx.close()
