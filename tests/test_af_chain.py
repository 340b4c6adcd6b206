"""The radio's AF chain (sdrpp_vfo_set_af: resampler to the sink's rate -> optional 300 Hz high-pass -> optional de-emphasis), sample by sample,
at every structural class the reference's rate planner produces for the radio's four AF input rates and the audio rates the sinks offer.

test_parity_vfo.py::test_af_chain and the pipelined AF tests run the chain at 48 000 Hz with three option sets and compare RMS over a push.  Here
every row of ROWS is one class of capi.design_resampler's answer (nothing, pre-decimation only, an interpolating or decimating polyphase stage
in the matrix form (L <= 15) or in the vector form, stages + polyphase, the high-pass beyond the channel filter's 4 096 taps), and the plan a row
is there for is asserted before anything runs.  The receiver rates (1 MHz WFM, 200 kHz NFM, 240 kHz AM, 192 kHz SSB) give the VFO's own chain a
power-of-two decimation and NO polyphase stage, so a `polyc` launch is the AF chain's.

THE YARDSTICK (restate_af64) is a float64 restatement of the chain in numpy, taking the float32 coefficients as given: the PowerDecimator stages and the
polyphase bank in polyphase_bank.h's phase order (test_kernel_forms.py's _fir64 / _poly), the high-pass FIR, and y = alpha * x + beta * y per channel with
beta the float32 value of 1 - alpha.  ITS INPUT IS THE PRODUCT'S OWN DEMODULATOR OUTPUT for the same pushes (sdrpp_vfo_read after ordinary passes): the chain
is isolated from the demodulator, and AGC look-ahead and NCO drift do not matter.

THE BAR is test_kernel_forms.py's (MARGIN, BASELINE_MAX and the 1.25 rule are imported, not chosen): max |got - ref64| / rms(ref64) over every output
frame from the first must stay within MARGIN x the same quantity measured at run time for the pinned oracle's float32-sequential chain (orc_resampler_*,
orc_fir_*, orc_deemp_* as test_parity_vfo._OracleAf drives them) fed the same input; that baseline may not exceed 1.25 x the figure recorded in BASELINES
for its leg nor BASELINE_MAX.  The project's RMS bar (within 1e-5 of the oracle chain) is kept beside it.

Four runs per row: ordinary in one push; ordinary over test_kernel_forms.ragged's cuts with its 1- and 7-sample pushes a second time in mid-stream
(cuts_of: pushes that give no audio frame, at which the stage phases, offsets and the de-emphasis state slot must stand still); pipelined over the same cuts; pipelined with launch groups of 3.  Runs 1 and 2 meet the
per-sample bar, each against the restatement of its own demodulator output; run 3 equals run 2 bit for bit; run 4 does too without de-emphasis and
meets the per-sample bar with it (the scan's segments start where a launch starts, see test_grouped_launches_mixed_modes_af_and_reference_blocks); runs 3
and 4 never fall back to an ordinary pass."""
import numpy as np
import pytest

import support as S
from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_kernel_forms import BASELINE_MAX, MARGIN, _bits_equal, _fir64, _poly, dist, ragged, rms
from test_parity_vfo import _OracleAf

# receiver rate per mode: the VFO's own resampler is a power-of-two decimation, no polyphase stage
RX_RATE = {"WFM": 1.0e6, "NFM": 200e3, "AM": 240e3, "USB": 192e3, "LSB": 192e3, "DSB": 192e3}
POLY_FORMS = ("polyc", "poly", "polyb_4", "polyb_4_odd", "polyb_8", "polyb_8_odd")


class Row:
    """mode -> audio rate with options; `plan` = (stage decimations, interp, decim) the row is there for, `form` = how its polyphase stage must run."""

    def __init__(self, mode, rate, tau=None, hp=False, plan=((), 1, 1), form=None, n=20000, hp_taps=0):
        self.mode, self.rate, self.tau, self.hp, self.plan, self.form, self.n, self.hp_taps = mode, float(rate), tau, hp, plan, form, n, hp_taps
        self.id = "%s_%d%s%s" % (mode.lower(), rate, "_hp" if hp else "", "_%dus" % round(tau * 1e6) if tau else "")


ROWS = [
    # ---- no resampler ----
    Row("NFM", 50000, tau=75e-6),
    Row("USB", 24000, hp=True, hp_taps=912),
    Row("USB", 24000),
    # ---- pre-decimation only ----
    Row("USB", 12000, plan=((2,), 1, 1)),
    # ---- matrix form, interpolating (lane bases with A / L repeating, more outputs than inputs per tile) ----
    Row("USB", 48000, hp=True, plan=((), 2, 1), form="matrix", hp_taps=1824),
    Row("LSB", 96000, plan=((), 4, 1), form="matrix"),
    Row("DSB", 192000, plan=((), 8, 1), form="matrix"),
    Row("AM", 24000, plan=((), 8, 5), form="matrix", n=30000),
    # ---- matrix form, decimating ----
    Row("USB", 16000, plan=((), 2, 3), form="matrix"),
    Row("AM", 12000, plan=((), 4, 5), form="matrix", n=30000),
    Row("AM", 8000, plan=((), 8, 15), form="matrix", n=30000),
    # ---- vector form ----
    Row("AM", 44100, hp=True, plan=((), 147, 50), form="vector", n=30000, hp_taps=1675),
    Row("AM", 176400, plan=((), 294, 25), form="vector", n=30000),
    Row("NFM", 44100, tau=75e-6, hp=True, plan=((), 441, 500), form="vector", hp_taps=1675),
    Row("NFM", 192000, tau=22e-6, plan=((), 96, 25), form="vector"),
    # ---- stages + polyphase ----
    Row("WFM", 44100, tau=50e-6, plan=((2, 2), 441, 625), form="vector", n=50000),
    Row("WFM", 8000, plan=((8, 2), 64, 125), form="vector", n=50000),
    Row("WFM", 50000, plan=((2, 2), 4, 5), form="matrix", n=50000),
    Row("WFM", 96000, tau=22e-6, plan=((2,), 96, 125), form="vector", n=50000),
    Row("NFM", 11025, plan=((2, 2), 441, 500), form="vector", n=50000),
    # ---- the high-pass beyond the channel filter's 4 096 taps ----
    Row("NFM", 96000, hp=True, plan=((), 48, 25), form="vector", n=12000, hp_taps=3648),
    Row("WFM", 192000, tau=22e-6, hp=True, plan=((), 96, 125), form="vector", n=40000, hp_taps=7296),
    Row("NFM", 176400, hp=True, plan=((), 441, 125), form="vector", n=10000, hp_taps=6703),
]

# Measured float32-sequential baselines (the pinned oracle's chain against the float64 restatement, max-abs / rms; the larger of the one-push and the ragged
# run): (emulator leg, device leg).  The oracle is CPU code, but its input here is the product's own demodulator output, which differs between the legs in the
# last bits (atan2f, fused multiply-adds) — and a maximum over a few thousand frames moves with them, 0.58e-6 / 0.88e-6 at its widest.  The bar of a row is
# MARGIN x the baseline measured at run time, which may not exceed 1.25 x the figure recorded here for its leg.
BASELINES = {
    "nfm_50000_75us": (5.79e-07, 8.79e-07),
    "usb_24000_hp": (7.57e-06, 7.76e-06),
    "usb_24000": (0, 0),
    "usb_12000": (1.02e-06, 1.69e-06),
    "usb_48000_hp": (1.16e-05, 1.27e-05),
    "lsb_96000": (1.27e-06, 1.48e-06),
    "dsb_192000": (1.47e-06, 1.47e-06),
    "am_24000": (3.09e-06, 3.17e-06),
    "usb_16000": (2.06e-06, 1.79e-06),
    "am_12000": (2.21e-06, 2.21e-06),
    "am_8000": (3.74e-06, 4.59e-06),
    "am_44100_hp": (2e-05, 2.13e-05),
    "am_176400": (5.54e-06, 4.62e-06),
    "nfm_44100_hp_75us": (2.33e-06, 2.45e-06),
    "nfm_192000_22us": (9.44e-07, 8.38e-07),
    "wfm_44100_50us": (1.05e-06, 1e-06),
    "wfm_8000": (1.2e-06, 9.19e-07),
    "wfm_50000": (2.02e-06, 2.07e-06),
    "wfm_96000_22us": (1.09e-06, 1.02e-06),
    "nfm_96000_hp": (1.48e-05, 1.47e-05),
    "wfm_192000_hp_22us": (1.46e-05, 1.5e-05),
    "nfm_176400_hp": (2.13e-05, 2.09e-05),
    "nfm_11025": (2.56e-06, 2.2e-06),
}


def signal(mode, sr, n, offset, seed=5):
    """Seeded noise + one carrier where the VFO listens, with audio between 700 Hz and 2.7 kHz (float64 maths, one rounding)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 1e-3
    w = 2 * np.pi * offset * t
    if mode in ("WFM", "NFM"):
        dev = 30e3 if mode == "WFM" else 2.5e3
        x += 0.2 * np.exp(1j * (w + (dev / 700.0) * 0.6 * np.sin(2 * np.pi * 700.0 * t) + (dev / 2300.0) * 0.4 * np.sin(2 * np.pi * 2300.0 * t)))
    elif mode == "AM":
        x += 0.2 * (1.0 + 0.3 * np.sin(2 * np.pi * 1000.0 * t) + 0.2 * np.sin(2 * np.pi * 2700.0 * t)) * np.exp(1j * w)
    else:
        for s in {"USB": (1,), "LSB": (-1,), "DSB": (1, -1)}[mode]:
            x += 0.1 * np.exp(1j * (w + s * 2 * np.pi * 700.0 * t)) + 0.07 * np.exp(1j * (w + s * 2 * np.pi * 1530.0 * t + 0.3))
    return x.astype(np.complex64)


def af_parts(a):
    """The float32 coefficients of an sdrpp_af_desc as numpy arrays: what the restatement takes as given."""
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy()
    return dict(stages=[(a.stage_decim[i], arr(a.stage_taps[i], a.stage_ntaps[i])) for i in range(a.n_stages)], interp=a.interp, decim=a.decim,
                rtaps=arr(a.resamp_taps, a.resamp_ntaps) if a.interp != a.decim else None, htaps=arr(a.hpf_taps, a.hpf_ntaps) if a.hpf_ntaps else None,
                alpha=np.float32(a.deemph_alpha))


def restate_af64(p, x):
    """The AF chain in float64 over one channel x of the whole stream, from cleared state."""
    y = np.asarray(x, np.float64)
    for D, taps in p["stages"]:
        y = _fir64(y, taps, D)
    if p["rtaps"] is not None:
        y = _poly(y, p["rtaps"], p["interp"], p["decim"], np.float64).real
    if p["htaps"] is not None:
        y = _fir64(y, p["htaps"])
    if p["alpha"] != 0:
        alpha, beta = np.float64(p["alpha"]), np.float64(np.float32(1) - p["alpha"])  # deephasis.h: (1 - alpha) is a float
        out, last = np.empty_like(y), 0.0
        for i, v in enumerate(y.tolist()):  # sequential by nature
            last = alpha * v + beta * last
            out[i] = last
        y = out
    return y


def cuts_of(n, tile):
    """test_kernel_forms.ragged (1 sample, 7 samples, a prime, a tile - 1 / + 1, two uneven parts) with the two short pushes a second time behind the prime: a
    push without an audio frame at the start of a stream finds every state still next to zero, in mid-stream it finds them in use."""
    c = ragged(n - 8, tile)
    return c[:3] + [1, 7] + c[3:]


def build(row):
    from sdrplusplus_amd import capi, radio

    sr = RX_RATE[row.mode]
    if_rate, bw = radio.RADIO_DEFAULTS[row.mode]
    offset = 0.21 * sr
    d, keep = radio.vfo_desc(sr, if_rate, bw, offset, row.mode)
    assert d.interp == d.decim, "the VFO's own chain must have no polyphase stage at this receiver rate"
    a, akeep = radio.af_desc(if_rate, row.rate, row.tau, row.hp)
    got_plan = (tuple(a.stage_decim[i] for i in range(a.n_stages)), a.interp, a.decim)
    assert got_plan == row.plan, ("the rate planner answers this row with another structure", row.id, got_plan, row.plan)
    assert a.hpf_ntaps == row.hp_taps and bool(a.deemph_alpha) == bool(row.tau), (row.id, a.hpf_ntaps)
    if row.form is not None:
        assert (a.interp <= 15) == (row.form == "matrix"), (row.id, a.interp)  # toep_build_poly: 15 / L whole phase cycles per tile, none for L > 15
    vdec = int(round(sr / if_rate))
    adec = int(np.prod(row.plan[0])) if row.plan[0] else 1
    cyc = (15 // a.interp if a.interp <= 15 else 1) * a.decim if a.interp != a.decim else 15
    return dict(sr=sr, if_rate=if_rate, vfo=(d, keep), af=(a, akeep), parts=af_parts(a), x=signal(row.mode, sr, row.n, offset), tile=vdec * adec * cyc,
                per_frame=vdec * adec * a.decim / a.interp)


def run(case, cuts, pipelined=False, group=0):
    """-> (demodulator output or None, AF output, pass forms, pipeline stats), concatenated over the pushes"""
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max(cuts) * max(1, group))
    vid = ctx.vfo_add(*case["vfo"])
    ctx.vfo_set_af(vid, *case["af"])
    if pipelined:
        ctx.set_pipelined(True, 1)
        if group:
            ctx.set_pipeline_group(group)
    dem, af, pos = [], [], 0
    for c in cuts:
        ctx.push(case["x"][pos:pos + c])
        pos += c
        if not pipelined:
            dem.append(ctx.vfo_read(vid).copy())
            af.append(ctx.vfo_af_read(vid).copy())
            assert len(af[-1]) == ctx.vfo_af_count(vid)
    if pipelined:
        for t in range(1, len(cuts) + 1):
            af.append(ctx.result_wait(t)["vfo"][vid])
            ctx.result_release(t)
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    ctx.close()
    cat = lambda q: np.concatenate(q) if q else np.zeros((0, 2), np.float32)
    return (None if pipelined else cat(dem)), cat(af), forms, st, [len(q) for q in af]


def oracle_af(case, row, dem):
    oaf = _OracleAf(case["if_rate"], row.rate, row.tau, row.hp)
    if row.hp:
        assert np.array_equal(oaf.hp_taps, case["parts"]["htaps"])
    return oaf.process(dem)


def per_sample(case, row, dem, got, what):
    """-> (baseline, library figure); asserts the per-sample bar and the project's RMS bar of `got` for the demodulator output `dem`."""
    assert np.array_equal(dem[:, 0], dem[:, 1]) and np.array_equal(got[:, 0], got[:, 1]), "these demodulators are mono: both channels carry the same bits"
    ref = restate_af64(case["parts"], dem[:, 0])
    orc = oracle_af(case, row, dem)
    assert len(ref) == len(orc) == len(got) > 0, (row.id, what, len(ref), len(orc), len(got))
    base, e = dist(orc[:, 0], ref), dist(got[:, 0], ref)
    assert base < BASELINE_MAX, ("ill-conditioned input: float32 sequential baseline", row.id, what, base)
    at = int(np.argmax(np.abs(got[:, 0].astype(np.float64) - ref)))
    assert e <= MARGIN * base, (row.id, "%s: %.3g against a float32 sequential baseline of %.3g" % (what, e, base), at, len(got))
    old = rms(got - orc) / max(1.0, rms(orc))
    assert old < 1e-5, (row.id, what, old)
    return base, e


def check_forms(row, forms, roles, what):
    if row.form == "vector":
        assert (forms if roles is None else roles).get("polyc", 0) > 0, (row.id, what, "polyc never ran", forms, roles)
    else:
        ran = [f for f in POLY_FORMS if forms.get(f, 0) or (roles or {}).get(f, 0)]
        assert not ran, (row.id, what, "a VALU polyphase form ran in a row without a vector-form stage", ran)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_af_chain_sample_by_sample(backend, row):
    case = build(row)
    cuts = cuts_of(row.n, case["tile"])
    dem1, af1, forms1, _, _ = run(case, [row.n])
    dem2, af2, forms2, _, cnt2 = run(case, cuts)
    _, af3, forms3, st3, cnt3 = run(case, cuts, pipelined=True)
    _, af4, forms4, st4, cnt4 = run(case, cuts, pipelined=True, group=3)
    if case["per_frame"] > 7:  # (the very first sample of a stream is an output of every decimator: the first 1-sample push gives one frame)
        assert cnt2[1] == 0, ("the 7-sample push must give no audio frame", cnt2)
    if case["per_frame"] > 2:
        assert min(cnt2[3:5]) == 0, ("no push without an audio frame in mid-stream", cnt2)
    assert cnt3 == cnt2 and cnt4 == cnt2, (cnt2, cnt3, cnt4)
    check_forms(row, forms1, None, "one push")
    check_forms(row, forms2, None, "ragged")
    for st, forms, what in ((st3, forms3, "pipelined"), (st4, forms4, "grouped")):
        assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(cuts) and not forms, (row.id, what, st, forms)
        check_forms(row, {}, st["roles"], what)
    base1, e1 = per_sample(case, row, dem1, af1, "one push")
    base2, e2 = per_sample(case, row, dem2, af2, "ragged")
    _bits_equal(af2, af3, "%s: pipelined vs ordinary" % row.id)
    e4 = 0.0
    if row.tau:
        _, e4 = per_sample(case, row, dem2, af4, "grouped")  # (a launch group's demodulator output is the ungrouped one bit for bit: test_pipelined.py)
    else:
        _bits_equal(af2, af4, "%s: grouped vs ordinary" % row.id)
    if not (row.hp or row.tau or row.plan != ((), 1, 1)):
        _bits_equal(dem1, af1, "%s: an empty chain hands the demodulator output on" % row.id)
        _bits_equal(dem2, af2, "%s: an empty chain hands the demodulator output on" % row.id)
    base = max(base1, base2)
    print("\n[af %s] %s per-sample max-abs / rms: baseline %.3g library %.3g (bar %.3g) | frames %d | pass forms %s | tick roles %s" % (
        row.id, backend, base, max(e1, e2, e4), MARGIN * base, len(af1), sorted(forms1), sorted(st3["roles"])))
    rec = BASELINES[row.id][backend == "gpu"]
    assert base <= 1.25 * rec, ("the float32 sequential baseline moved up: the bar may not loosen unseen", row.id, backend, base, rec)


SEG_PUSHES = [4 * 4095, 4 * 4096, 4 * 4097, 4, 4 * 8193, 4 * 12289, 64, 4 * 4096]
SEG_BASELINE = (6.85e-07, 7.47e-07)  # (emulator leg, device leg), as BASELINES


def test_deemphasis_segment_edges(backend):
    """The de-emphasis scan takes a second segment above 4 096 frames in one push (SDRPP_DEEMP_SEG).  NFM at 200 kHz -> 50 000 Hz with de-emphasis only
    makes frames = input / 4: pushes of 4 095, 4 096, 4 097, 1, 8 193, 12 289, 16 and 4 096 frames are 1, 1, 2, 1, 3, 4, 1, 1 segments — the state
    hand-over at a whole number of segments and of 16-frame work-item chunks.  Ordinary and pipelined, per sample."""
    row = Row("NFM", 50000, tau=50e-6, n=sum(SEG_PUSHES))
    case = build(row)
    dem, af, _, _, cnt = run(case, SEG_PUSHES)
    assert cnt == [c // 4 for c in SEG_PUSHES], cnt
    assert [(c + 4095) // 4096 for c in cnt] == [1, 1, 2, 1, 3, 4, 1, 1]
    base, e = per_sample(case, row, dem, af, "ordinary")
    _, afp, forms, st, cntp = run(case, SEG_PUSHES, pipelined=True)
    assert cntp == cnt and st["pass_blocks"] == 0 and st["tick_blocks"] == len(SEG_PUSHES) and not forms, (cntp, st, forms)
    for role in ("deemp_p0", "deemp_p1"):
        assert st["roles"].get(role, 0) > 0, (role, st["roles"])
    _, ep = per_sample(case, row, dem, afp, "pipelined")
    print("\n[af deemphasis segments] %s per-sample max-abs / rms: baseline %.3g library %.3g pipelined %.3g (bar %.3g)" % (backend, base, e, ep, MARGIN * base))
    assert base <= 1.25 * SEG_BASELINE[backend == "gpu"], ("the float32 sequential baseline moved up: the bar may not loosen unseen", base, SEG_BASELINE)


def test_high_pass_tap_limit(backend):
    """The AF high-pass is not bound by the channel filter's 4 096 taps (kChanHistCap: that history is pre-allocated, this one is sized from the tap count); what
    remains is a bound of 65 536 taps stated in include/sdrpp_gpu.h, answered with SDRPP_ERR_UNSUPPORTED and the tap count."""
    import ctypes as C
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=4096)
    d, keep = radio.vfo_desc(200e3, 50000.0, 12500.0, 10e3, "NFM")
    vid = ctx.vfo_add(d, keep)
    a, akeep = radio.af_desc(50000.0, 50000.0, None, False)
    taps = np.zeros(65537, np.float32)
    taps[65535] = 1.0  # (fir.h: out[m] = sum_k taps[k] * buf[m + k] over (K - 1 of history) ++ x — the LAST tap meets x[m])
    a.hpf_taps = radio._fp(taps)
    a.hpf_ntaps = 65537
    assert ctx.L.sdrpp_vfo_set_af(ctx.h, vid, C.byref(a)) == -5  # SDRPP_ERR_UNSUPPORTED
    assert "65537" in ctx.L.sdrpp_last_error(ctx.h).decode()
    a.hpf_ntaps = -1
    assert ctx.L.sdrpp_vfo_set_af(ctx.h, vid, C.byref(a)) == -2  # SDRPP_ERR_INVALID
    a.hpf_ntaps = 65536  # the bound itself is taken (and runs untiled: too long for an LDS tile of the register-blocked form)
    assert ctx.L.sdrpp_vfo_set_af(ctx.h, vid, C.byref(a)) == 0
    x = signal("NFM", 200e3, 512, 10e3)
    ctx.push(x)
    _bits_equal(ctx.vfo_read(vid), ctx.vfo_af_read(vid), "a one-tap-of-unity high-pass of 65 536 taps hands the stream on")
    forms = ctx.pass_form_stats()
    assert forms.get("fird", 0) > 0 and not forms.get("firb_c", 0), forms
    ctx.close()


def test_every_row_is_pinned_to_the_reference():
    """tests/test_oracle_vs_reference.py pins the oracle's resampler at every (AF rate, audio rate) pair, its high-pass taps at every rate and its de-emphasis
    at every time constant that a row above takes the baseline chain to."""
    import inspect

    import test_oracle_vs_reference as T
    from sdrplusplus_amd import radio

    pairs = {(a, b) for a, b, *_ in T.AF_RATE_PAIRS}
    hp = {48000.0} | {r for r, _ in _params(T.test_af_high_pass_taps_every_rate_bit_exact)}
    de = {(50e-6, 48000.0)} | set(_params(T.test_af_deemphasis_every_setting_bit_exact))
    assert "48000.0" in inspect.getsource(T.test_high_pass_and_windows_bit_exact) and "50e-6, 48000.0" in inspect.getsource(T.test_af_resampler_and_deemphasis_bit_exact)
    for row in ROWS:
        assert (radio.RADIO_DEFAULTS[row.mode][0], row.rate) in pairs, row.id
        if row.hp and row.rate > 24000:  # (24 000 Hz: the 48 000 Hz design at half the length, not a rate the sinks offer — the row is there for `no resampler`)
            assert row.rate in hp, row.id
        if row.tau:
            assert (row.tau, row.rate) in de, row.id
    assert (50e-6, 50000.0) in de  # test_deemphasis_segment_edges


def _params(fn):
    return [tuple(m.args[1]) for m in fn.pytestmark if m.name == "parametrize"][0]
