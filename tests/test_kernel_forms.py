"""Every channeliser kernel form the planner can select, reached on purpose and checked sample by sample.

The parity suite builds its VFOs with radio.vfo_desc — the reference's decimation plans and the radio module's IF rates — and the planner
answers those with a handful of forms.  sdrpp_vfo_add takes ANY descriptor, and the generic matrix front ends (fcm_6 / fcm_10 / fcm_16),
the long first stage without register prefetch (fcl_0), the register-blocked few-phase resampler (polyb_*) and the VALU front ends with
8 / 4 / 2 VFOs per job are only reached by descriptors a host designs itself.  ROWS below has one row per form: it names the forms it must
reach and asserts them — on the ordinary pass through sdrpp_pass_form_stats, on the pipelined leg through sdrpp_pipeline_stats.

Three runs per row: the ordinary pass in ONE push, the ordinary pass over a ragged list of pushes (1 sample, 7 samples, a prime, one tile
of front-end outputs - 1 / + 1 sample), the pipelined mode over the same ragged pushes.  The two ragged runs must be bit-identical (as in
test_pipelined.py); the one-push run must equal them within what test_push_size_invariance allows (the closed-form NCO is anchored at the
start of a push, so cuts move its double-precision phase origin: not the same bits by design).

THE BAR IS PER SAMPLE.  Every output sample of every VFO, from the first one (zero history), is compared with a float64 restatement of
the operation written here in numpy (restate64: NCO exp(j arg(phaseDelta_f32) n), decimating FIRs, the polyphase bank in
polyphase_bank.h's phase order, channel FIR, discriminator + audio low-pass for FM), taking the float32 taps as given.  The quantity is
max |got - ref64| / rms(ref64).  The bar is not a chosen number: for every row the same distance is measured, on the CPU, for a float32
SEQUENTIAL evaluation of the row (the pinned oracle with its ideal-NCO switch for radio.vfo_desc rows; orc_xlator (ideal) + orc_fir per
stage + a float32 numpy accumulation of the custom resampler for the hand-built ones), and the library must stay within 4x that baseline.
The product sums in another order (tap pairs then differences, k-ordered fmaf chains): the same sqrt(K) eps growth, not the same bits —
while an indexing, phase or history error costs at least one tap's weight, orders of magnitude more.  A baseline above 1e-4 means the
row's input is ill-conditioned (an FM discriminator on a fading envelope): the input is wrong then, not the margin.

Every row checks the IF per sample, and every demodulating row its audio as well, on the one-push run AND the ragged run: FM through the
discriminator + audio low-pass; AM as envelope -> DC blocker -> audio low-pass and USB as the second translation's real part, both with
the AGC pinned to unit gain (pin_agc: the reference's AGC looks ahead over its block, so its output depends on the push cuts by design and
test_parity_vfo.py pins it to the oracle block by block).  Rows built with radio.vfo_desc also keep the project's existing bars against
the pinned oracle (FM audio RMS < 1e-5, IF relative RMS < 2e-6 against the ideal-NCO oracle and < 2e-3 against the reference's own rotator).

The measured float32-sequential baseline of every row is recorded in BASELINES beside the case table (the bar is MARGIN x the baseline
measured at run time, which may not exceed 1.25 x the recorded one); every case prints baseline, library figure and bar.  DESIGN.md
section 2 tabulates those printed figures for the emulator and the device, row by row."""
import inspect

import numpy as np
import pytest

import support as S
from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)

MARGIN = 4.0          # library <= MARGIN x float32-sequential baseline (see above)
BASELINE_MAX = 1e-4   # a row whose float32-sequential baseline is worse has an ill-conditioned input


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)) ** 2))) if a.size else 0.0


# ---- descriptors built by hand -----------------------------------------------------------------------------------------------------------
def _lp(ntaps, cutoff, rate):
    """A low-pass of exactly `ntaps` taps from capi.design_low_pass: the transition width is searched, the cutoff is as given."""
    from sdrplusplus_amd import capi

    L = capi.load()
    lo, hi = rate * 1e-4, rate * 20.0  # tap count falls as the transition widens
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        n = L.sdrpp_design_low_pass(cutoff, mid, rate, int(ntaps & 1), None, 0)
        if n == ntaps:
            t = capi.design_low_pass(cutoff, mid, rate, odd=bool(ntaps & 1))
            assert len(t) == ntaps
            return t
        if n > ntaps:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no %d-tap low-pass at cutoff %g / rate %g" % (ntaps, cutoff, rate))


def hand_desc(sr, offset, stages=(), interp=1, decim=1, rtaps=None, ctaps=None, mode="RAW", bandwidth=0.0):
    """sdrpp_vfo_desc from explicit parts: stage (decimation, taps) pairs, interp / decim + resampler prototype, channel taps; the
    demodulator's fields as radio.vfo_desc fills them.  Returns (desc, keepalive, out_rate)."""
    from sdrplusplus_amd import capi, radio

    d = capi.VfoDesc()
    keep = []
    d.nco_mode = 0
    d.phase_delta_re, d.phase_delta_im = capi.design_phase_delta(-offset, sr)
    d.n_stages = len(stages)
    rate = sr
    for i, (dec, taps) in enumerate(stages):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        keep.append(t)
        d.stage_decim[i], d.stage_ntaps[i], d.stage_taps[i] = dec, len(t), radio._fp(t)
        rate /= dec
    d.interp, d.decim, d.resamp_ntaps = interp, decim, 0
    if interp != decim:
        rt = np.ascontiguousarray(rtaps, dtype=np.float32)
        keep.append(rt)
        d.resamp_ntaps, d.resamp_taps = len(rt), radio._fp(rt)
        rate = rate * interp / decim
    d.chan_ntaps = 0
    if ctaps is not None:
        ct = np.ascontiguousarray(ctaps, dtype=np.float32)
        keep.append(ct)
        d.chan_ntaps, d.chan_taps = len(ct), radio._fp(ct)
    d.demod = radio.DEMOD_CODES[mode]
    d.agc_set_point, d.agc_max_gain, d.agc_max_output_amp, d.agc_init_gain = 1.0, 10e6, 10.0, float("inf")
    d.agc_attack, d.agc_decay = np.float32(50.0 / rate), np.float32(5.0 / rate)
    d.dc_block_rate = np.float32(100.0 / rate)
    d.ssb_phase_delta_re, d.ssb_phase_delta_im = 1.0, 0.0
    d.inv_deviation, d.audio_ntaps = 0.0, 0
    if mode == "NFM":
        d.inv_deviation = np.float32(1.0 / radio.hz_to_rads(bandwidth / 2.0, rate))
        at = capi.design_low_pass(bandwidth / 2.0, (bandwidth / 2.0) * 0.1, rate)
        keep.append(at)
        d.audio_ntaps, d.audio_taps = len(at), radio._fp(at)
    else:
        assert mode == "RAW", mode
    return d, keep, rate


def _parts(d):
    """The float32 taps of a descriptor, as numpy arrays (what both the restatement and the float32 baseline take as given)."""
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n > 0 else None
    return dict(delta=(np.float32(d.phase_delta_re), np.float32(d.phase_delta_im)),
                stages=[(d.stage_decim[i], arr(d.stage_taps[i], d.stage_ntaps[i])) for i in range(d.n_stages)],
                interp=d.interp, decim=d.decim, rtaps=arr(d.resamp_taps, d.resamp_ntaps) if d.interp != d.decim else None,
                ctaps=arr(d.chan_taps, d.chan_ntaps), demod=d.demod, inv_dev=np.float32(d.inv_deviation), ataps=arr(d.audio_taps, d.audio_ntaps),
                dc_rate=np.float32(d.dc_block_rate), ssb=(np.float32(d.ssb_phase_delta_re), np.float32(d.ssb_phase_delta_im)))


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------------
def _fir64(x, taps, D=1):
    """fir.h / decimating_fir.h: out[m] = sum_k taps[k] * buf[m * D + k], buf = (K - 1 zeros of history) ++ x."""
    t = np.asarray(taps, dtype=np.float64)
    return np.convolve(x, t[::-1])[:len(x)][::D]


def _poly_index(n_in, L, M):
    """polyphase_resampler.h:69-99 from (phase, offset) = (0, 0): output m reads buf[offset_m ...] with bank[phase_m]."""
    m = np.arange((n_in * L + M - 1) // M, dtype=np.int64)
    A = m * M
    return A // L, A % L


def _bank(rtaps, L, dtype):
    tpp = (len(rtaps) + L - 1) // L
    bank = np.zeros((L, tpp), dtype=dtype)
    for i in range(len(rtaps)):
        bank[(L - 1) - (i % L), i // L] = rtaps[i]  # polyphase_bank.h:31-34
    return bank, tpp


def _poly(x, rtaps, L, M, dtype):
    """The polyphase resampler, accumulated tap by tap in `dtype` (complex128: the restatement; complex64: the float32 sequential baseline)."""
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    bank, tpp = _bank(rtaps, L, dtype)
    off, ph = _poly_index(len(x), L, M)
    buf = np.concatenate([np.zeros(tpp - 1, ctype), x.astype(ctype)])
    acc = np.zeros(len(off), ctype)
    for k in range(tpp):  # k-ordered, one rounding per product and per sum in float32 — volk's generic dot product
        acc = (acc + buf[off + k] * bank[ph, k].astype(dtype)).astype(ctype)
    return acc


def restate64(p, x):
    """(IF, audio or None) in float64 for descriptor parts `p` over the whole stream x (complex64), zero history."""
    theta = np.arctan2(np.float64(p["delta"][1]), np.float64(p["delta"][0]))
    y = x.astype(np.complex128) * np.exp(1j * theta * np.arange(len(x), dtype=np.float64))
    for D, taps in p["stages"]:
        y = _fir64(y, taps, D)
    if p["rtaps"] is not None:
        y = _poly(y, p["rtaps"], p["interp"], p["decim"], np.float64)
    if p["ctaps"] is not None:
        y = _fir64(y, p["ctaps"])
    audio = None
    if p["demod"] in (0, 1):  # WFM / NFM: quadrature.h — normalised phase difference x invDeviation, then the audio low-pass
        ph = np.angle(y)
        dphi = np.diff(np.concatenate([[0.0], ph]))
        dphi = (dphi + np.pi) % (2.0 * np.pi) - np.pi
        audio = dphi * np.float64(p["inv_dev"])
        if p["ataps"] is not None:
            audio = _fir64(audio, p["ataps"])
    elif p["demod"] in (2, 3):
        audio = demod_am_ssb(p, y, np.float64)
    return y, audio


def demod_am_ssb(p, y, dtype):
    """AM (demod/am.h:101-131) and USB (ssb.h:77-92) behind the IF stream y with the AGC PINNED to unit gain (pin_agc), in `dtype`: float64 = the
    restatement, float32 = the sequential baseline (one rounding per operation, the reference's order).
    AM: envelope -> DC blocker (dc_blocker.h:54-60: out = in - offset; offset += out * rate) -> audio low-pass.  USB: Re(y * exp(j theta2 n))."""
    f = dtype
    re, im = y.real.astype(f), y.imag.astype(f)
    if p["demod"] == 2:
        m = np.sqrt((re * re) + (im * im)).astype(f)
        out = np.empty(len(m), f)
        off, rate = f(0.0), f(p["dc_rate"])
        for i in range(len(m)):  # sequential by nature
            o = f(m[i] - off)
            out[i] = o
            off = f(off + f(o * rate))
        if f == np.float64:
            return _fir64(out, p["ataps"])
        return _orc_fir(out, p["ataps"], 1, width=1)
    theta2 = np.arctan2(np.float64(p["ssb"][1]), np.float64(p["ssb"][0])) / (2.0 * np.pi)  # turns per sample of the stored float phaseDelta
    ph = theta2 * np.arange(len(y), dtype=np.float64)
    ph -= np.floor(ph)
    pr, pi = np.cos(2.0 * np.pi * ph).astype(f), np.sin(2.0 * np.pi * ph).astype(f)
    return ((re * pr).astype(f) - (im * pi).astype(f)).astype(f)


def pin_agc(d):
    """The AGC of an AM / SSB descriptor held at unit gain: amp starts at setPoint / initGain = 1 and attack = decay = 0 leave it there (agc.h:70-109:
    amp = amp * (1 - rate) + |x| * rate), so the audio is a feed-forward function of the IF and can be restated sample by sample."""
    d.agc_attack, d.agc_decay, d.agc_init_gain = 0.0, 0.0, 1.0
    return d


def _orc_fir(y, taps, D, width=2):
    o = S.oracle()
    t = np.ascontiguousarray(taps, np.float32)
    h = o.orc_fir_create(S._fp(t), len(t), D, width)
    y = np.ascontiguousarray(y, np.complex64 if width == 2 else np.float32)
    out = np.empty(len(y) + 8, y.dtype)
    n = o.orc_fir_process(h, len(y), S._fp(y.view(np.float32)), S._fp(out.view(np.float32)))
    o.orc_fir_destroy(h)
    return out[:n].copy()


def baseline32_hand(p, x, sr, offset):
    """float32 sequential evaluation of a hand-built row: the oracle's FrequencyXlator with its ideal-NCO switch, orc_fir per stage, a float32 numpy
    accumulation of the custom resampler, orc_fir for the channel filter, the oracle's discriminator + audio FIR."""
    o = S.oracle()
    fir = _orc_fir

    xl = o.orc_xlator_create(-offset, sr)
    o.orc_xlator_set_ideal(xl, 1)
    xin = S.c64(x)
    y = np.empty_like(xin)
    o.orc_xlator_process(xl, len(xin), S._fp(xin.view(np.float32)), S._fp(y.view(np.float32)))
    o.orc_xlator_destroy(xl)
    for D, taps in p["stages"]:
        y = fir(y, taps, D)
    if p["rtaps"] is not None:
        y = _poly(y, p["rtaps"], p["interp"], p["decim"], np.float32)
    if p["ctaps"] is not None:
        y = fir(y, p["ctaps"], 1)
    audio = None
    if p["demod"] in (0, 1):
        cph = np.arctan2(y.imag, y.real).astype(np.float32)
        d = (cph - np.concatenate([np.zeros(1, np.float32), cph[:-1]])).astype(np.float32)
        d = np.where(d > np.float32(np.pi), d - np.float32(2 * np.pi), np.where(d <= -np.float32(np.pi), d + np.float32(2 * np.pi), d)).astype(np.float32)
        audio = (d * p["inv_dev"]).astype(np.float32)
        if p["ataps"] is not None:
            audio = fir(audio, p["ataps"], 1, width=1)
    return y, audio


def dist(got, ref64):
    """max-abs distance relative to the reference stream's RMS; every sample counts."""
    assert len(got) == len(ref64), (len(got), len(ref64))
    return float(np.max(np.abs(np.asarray(got).astype(ref64.dtype) - ref64))) / rms(ref64)


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
def _fm_mix(sr, n, offsets, seed, dev, tone=700.0, amp=0.05, noise=2e-3):
    """Seeded noise + one FM carrier per VFO (float64 maths, one rounding)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * noise
    for k, f in enumerate(offsets):
        tn = tone + 37.0 * (k % 11)
        x += amp * np.exp(1j * (2 * np.pi * f * t + (dev / tn) * np.sin(2 * np.pi * tn * t)))
    return x.astype(np.complex64)


def _spread(nv, sr, frac=0.8):
    return [((k + 0.5) / nv - 0.5) * frac * sr + 13.0 * k for k in range(nv)]


class Row:
    """One row: `build(backend)` -> dict(sr, n, descs=[(desc, keep, parts, offset, oracle_args or None)], x); forms_pass / roles_tick: what must
    have run; tile: input samples of one front-end tile (32 << lgD) for the ragged cuts; tick: False = the form has no tick role."""

    def __init__(self, rid, build, forms_pass, roles_tick, tile, tick=True):
        self.id, self.build, self.forms_pass, self.roles_tick, self.tile, self.tick = rid, build, forms_pass, roles_tick, tile, tick
        # the matrix front ends run a second time with their tiles dealt out over WALK_WAVES wavefronts per job (SDRPP_GPU_FRONT_WAVES): every wavefront then
        # walks several tiles — the next tile's window fetched under the current matrix loop, the planes re-used, a partial last tile — as it does
        # under the planner's own rules only from ~10^5 outputs per job on
        self.walk = any(f.startswith(("fcm_", "fcl_")) for f in forms_pass)


def _radio_row(sr, mode, nv=1, n_emu=None, dev=None, offsets=None, bandwidth=None):
    def build(backend):
        from sdrplusplus_amd import radio

        if_rate, bw = radio.RADIO_DEFAULTS[mode]
        bw = bandwidth or bw
        offs = offsets or ([0.21 * sr] if nv == 1 else _spread(nv, sr, 0.6))
        n = n_emu or int(sr / 200)  # (both legs run the same block: the float32 baseline, measured on the CPU, is then the same figure on both)
        descs = []
        for f in offs:
            d, keep = radio.vfo_desc(sr, if_rate, bw, f, mode)
            if mode in ("AM", "USB"):
                pin_agc(d)
            descs.append((d, keep, _parts(d), f, (sr, if_rate, bw, f, S.MODES[mode])))
        x = _fm_mix(sr, n, offs, 21, dev or min(0.3 * bw, 0.2 * if_rate), amp=0.2 / max(1, nv) ** 0.5)
        return dict(sr=sr, n=n, descs=descs, x=x)

    return build


def _hand_row(sr, nv, stages_spec, interp=1, decim=1, rt_spec=None, chan=None, mode="RAW", bw=0.0, n_emu=20000, asym2=False):
    """stages_spec: [(decimation, ntaps)]; rt_spec: prototype tap count of the resampler; chan: channel-filter tap count."""
    def build(backend):
        rate, stages = sr, []
        for i, (D, K) in enumerate(stages_spec):
            t = _lp(K + (1 if (asym2 and i == 1) else 0), 0.4 * rate / D, rate)
            if asym2 and i == 1:
                t = t[:K].copy()  # a linear-phase low-pass with its last tap cut off: not symmetric any more
                assert not np.array_equal(t, t[::-1])
            stages.append((D, t))
            rate /= D
        rt = None
        if interp != decim:
            rt = _lp(rt_spec, 0.45 * rate * min(interp, interp * interp / decim) / interp, rate * interp) * np.float32(interp)
        out = rate * interp / decim
        ct = _lp(chan, 0.3 * out, out) if chan else None
        offs = _spread(nv, sr, 0.7)
        descs = []
        for f in offs:
            d, keep, orate = hand_desc(sr, f, stages, interp, decim, rt, ct, mode, bw)
            descs.append((d, keep, _parts(d), f, None))
        n = n_emu  # (both legs run the same block)
        x = _fm_mix(sr, n, offs, 33, 0.08 * out, amp=0.3 / max(1, nv) ** 0.5)
        return dict(sr=sr, n=n, descs=descs, x=x)

    return build


# One row per form.  The float32-sequential baseline of every row is in BASELINES below the table; the bar of a row is MARGIN x its baseline.
ROWS = [
    # ---- rows the reference's plans reach (radio.vfo_desc at a real receiver rate) ----
    Row("polyc_2048k_wfm", _radio_row(2.048e6, "WFM", n_emu=350000), {"polyc"}, {"polyc"}, 32 * 4),
    Row("polyc_768k_wfm", _radio_row(768e3, "WFM", n_emu=90000), {"polyc"}, {"polyc"}, 32 * 2),
    Row("s1d_firb_8M_usb", _radio_row(8e6, "USB"), {"s1d_1", "firb_c"}, {"s1d_1", "firb_c"}, 32 * 32),
    Row("fcl_pf_firb_8M_usb", _radio_row(8e6, "USB", nv=2), {"fcl_pf", "firb_c"}, {"fcl_pf", "firb_c"}, 16 * 32),
    Row("poly_6M_am", _radio_row(6e6, "AM"), {"poly"}, {"poly"}, 32 * 32),
    Row("rot_384k_wfm", _radio_row(384e3, "WFM"), {"rot"}, {"rot"}, 256),
    Row("as_planned_56M_nfm", _radio_row(56e6, "NFM", n_emu=140000), {"s1d_1"}, {"s1d_1"}, 32 * 64),
    # ---- audio filters too long for the matrix form (toep_upload: table + four windows > 160 KB / 3): the register-blocked VALU FIRs ----
    Row("firb_q_400k_nfm_bw2000", _radio_row(400e3, "NFM", n_emu=40000, bandwidth=2000.0), {"firb_q"}, {"firb_q"}, 32 * 8),
    Row("firb_s_480k_am_bw500", _radio_row(480e3, "AM", n_emu=40000, bandwidth=500.0), {"firb_s"}, {"firb_s"}, 32 * 32),
    # ---- the generic matrix front ends (front2_t2 / frontcm_ok), bank-size edges 17 / 32 / 33 / 65 ----
    Row("fcm_6_nv17", _hand_row(200e3, 17, [(2, 11), (2, 7)], chan=31), {"fcm_6"}, {"fcm_6"}, 32 * 4),
    Row("fcm_6_evenK_nv33", _hand_row(200e3, 33, [(2, 12), (2, 8)], chan=31), {"fcm_6", "f2_1"}, {"fcm_6", "f2_1"}, 32 * 4),
    Row("fcm_10_nv32", _hand_row(400e3, 32, [(4, 27), (2, 31)], chan=31), {"fcm_10"}, {"fcm_10"}, 32 * 8),
    # ((8, 44) + (2, 31), K = 284, fails frontcm_ok's LDS clause: frontcm_layout(284, 4).total * 4 = 73 984 B > 160 KB / 3 — K <= 156 fits at lgD = 4)
    Row("fcm_16_nv65", _hand_row(800e3, 65, [(8, 44), (2, 15)], chan=31, n_emu=28000), {"fcm_16", "f2_1"}, {"fcm_16", "f2_1"}, 32 * 16),
    Row("fcm_16_lgD5_oddK_nv17", _hand_row(1.6e6, 17, [(16, 15), (2, 2)], chan=31, n_emu=54000), {"fcm_16"}, {"fcm_16"}, 32 * 32),
    # ---- long first stages: register prefetch or not, 16-row and 32-row shapes (2 / 16 / 17 VFOs) ----
    Row("fcl_0_nv2", _hand_row(3.2e6, 2, [(64, 513)], chan=31, n_emu=64000), {"fcl_0"}, {"fcl_0"}, 16 * 64),
    Row("fcl_pf_nv16", _hand_row(1.6e6, 16, [(32, 129)], chan=31, n_emu=40000), {"fcl_pf"}, {"fcl_pf"}, 16 * 32),
    Row("fcl_pf_nv17", _hand_row(1.6e6, 17, [(32, 130)], chan=31, n_emu=54000), {"fcl_pf"}, {"fcl_pf"}, 32 * 32),
    # ---- the VALU front ends with 8 / 4 / 2 VFOs per job (ordinary pass only; a tick runs them one VFO per job) ----
    Row("s1_8_4_2_nv15", _hand_row(400e3, 15, [(8, 45)], chan=31), {"s1_8", "s1_4", "s1_2", "s1_1"}, {"s1_1"}, 256 * 8),
    Row("f2_8_4_2_nv15", _hand_row(400e3, 15, [(4, 27), (2, 31)], chan=31), {"f2_8", "f2_4", "f2_2", "f2_1"}, {"f2_1"}, 256),
    Row("s1d_8_4_2_nv15", _hand_row(1.6e6, 15, [(32, 7)], chan=31, n_emu=40000), {"s1d_8", "s1d_4", "s1d_2", "s1d_1"}, {"s1d_1"}, 256 * 32),
    Row("asym_stage2_nv18", _hand_row(400e3, 18, [(4, 27), (2, 12)], chan=31, asym2=True), {"s1_8", "s1_2", "toep_c"}, {"s1_1", "toep_c"}, 256 * 4),
    # ---- polyb: interp <= 4 and 5 ... 8, even and odd decim, a decim large enough that the Toeplitz window does not fit (no tick role) ----
    Row("polyb_4_3over64", _hand_row(1.0e6, 2, [], 3, 64, rt_spec=601, chan=31, mode="NFM", bw=12500.0, n_emu=60000), {"rot", "polyb_4"}, set(), 256, tick=False),
    Row("polyb_4_odd_4over45", _hand_row(0.6e6, 1, [], 4, 45, rt_spec=480, chan=31, mode="NFM", bw=12500.0, n_emu=40000), {"rot", "polyb_4_odd"}, set(), 256, tick=False),
    Row("polyb_8_5over72", _hand_row(0.75e6, 1, [], 5, 72, rt_spec=1001, chan=31, mode="NFM", bw=12500.0, n_emu=50000), {"rot", "polyb_8"}, set(), 256, tick=False),
    Row("polyb_8_odd_7over51", _hand_row(0.4e6, 2, [(2, 11)], 7, 51, rt_spec=700, chan=31, n_emu=50000), {"polyb_8_odd"}, set(), 256, tick=False),
]


# The measured float32-sequential baselines of every row (worst VFO; max-abs / rms against the float64 restatement): (IF, audio or None).  The bar of
# a row is MARGIN x the baseline measured at run time; that baseline may not exceed 1.25 x the figure recorded here.
BASELINES = {
    "polyc_2048k_wfm": (9.13e-07, 3.03e-06),
    "polyc_768k_wfm": (9.18e-07, 2.73e-06),
    "s1d_firb_8M_usb": (1.69e-06, 2.54e-06),
    "fcl_pf_firb_8M_usb": (1.74e-06, 2.33e-06),
    "poly_6M_am": (1.65e-06, 4.46e-06),
    "rot_384k_wfm": (7.81e-07, 1.73e-06),
    "as_planned_56M_nfm": (1.63e-06, 2.75e-05),
    "firb_q_400k_nfm_bw2000": (2.92e-06, 6.29e-06),
    "firb_s_480k_am_bw500": (9.13e-06, 3.09e-05),
    "fcm_6_nv17": (7.3e-07, None),
    "fcm_6_evenK_nv33": (1.14e-06, None),
    "fcm_10_nv32": (8.51e-07, None),
    "fcm_16_nv65": (1.06e-06, None),
    "fcm_16_lgD5_oddK_nv17": (6.93e-07, None),
    "fcl_0_nv2": (9.17e-07, None),
    "fcl_pf_nv16": (7.42e-07, None),
    "fcl_pf_nv17": (7.42e-07, None),
    "s1_8_4_2_nv15": (7.94e-07, None),
    "f2_8_4_2_nv15": (7.62e-07, None),
    "s1d_8_4_2_nv15": (8.94e-07, None),
    "asym_stage2_nv18": (7.16e-07, None),
    "polyb_4_3over64": (7.03e-07, 3.28e-06),
    "polyb_4_odd_4over45": (7.27e-07, 2.76e-06),
    "polyb_8_5over72": (7.8e-07, 3.57e-06),
    "polyb_8_odd_7over51": (5.25e-07, None),
}


def _is_prime(k):
    return k > 1 and all(k % q for q in range(2, int(k ** 0.5) + 1))


def ragged(n, tile):
    """Cuts of n samples: 1 sample, 7 samples, a prime, one tile of front-end outputs - 1 / + 1 sample, the rest in two uneven parts."""
    prime = next(k for k in range(max(11, n // 7), n) if _is_prime(k))
    cuts = [1, 7, prime, tile - 1, tile + 1]
    rest = n - sum(cuts)
    assert rest > 2 * tile, (n, cuts)
    a = rest * 3 // 5 + 1
    cuts += [a, rest - a]
    assert sum(cuts) == n and min(cuts) >= 1
    return cuts


def _run(case, cuts, pipelined):
    """-> (per-VFO IF, per-VFO output or None, forms of the ordinary pass, pipeline stats)"""
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max(cuts))
    vids = [ctx.vfo_add(d, keep) for d, keep, _, _, _ in case["descs"]]
    raw = [p["demod"] == -1 for _, _, p, _, _ in case["descs"]]
    if pipelined:
        ctx.set_pipelined(True, 1)
    ifs, outs, pos = [[] for _ in vids], [[] for _ in vids], 0
    for c in cuts:
        ctx.push(case["x"][pos:pos + c])
        pos += c
        if not pipelined:
            for i, v in enumerate(vids):
                ifs[i].append(ctx.vfo_read_if(v))
                if not raw[i]:
                    outs[i].append(ctx.vfo_read(v).copy())
    if pipelined:
        for t in range(1, len(cuts) + 1):
            got = ctx.result_wait(t)
            for i, v in enumerate(vids):
                a = got["vfo"][v]
                (ifs if raw[i] else outs)[i].append(a.copy().view(np.complex64).reshape(-1) if raw[i] else a)
            ctx.result_release(t)
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    ctx.close()
    cat = lambda parts, dt, shape: np.concatenate(parts) if parts else np.zeros(shape, dt)
    return ([cat(q, np.complex64, 0) for q in ifs], [cat(q, np.float32, (0, 2)) if not raw[i] else None for i, q in enumerate(outs)], forms, st)


def _bits_equal(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), (what, float(np.max(np.abs(a - b))))


WALK_WAVES = 8
CASES = [(r, False) for r in ROWS] + [(r, True) for r in ROWS if r.walk]


@pytest.mark.parametrize("row,walk", CASES, ids=[r.id + ("-walk" if w else "") for r, w in CASES])
def test_form_reached_and_right_sample_by_sample(backend, row, walk, monkeypatch):
    case = row.build(backend)
    n, x = case["n"], case["x"]
    cuts = ragged(n, row.tile)
    if walk:
        monkeypatch.setenv("SDRPP_GPU_FRONT_WAVES", str(WALK_WAVES))  # (read when a context is created)
        assert max(cuts) // row.tile >= 3 * WALK_WAVES and n // row.tile >= 3 * WALK_WAVES, "every wavefront of the long pushes must walk at least three tiles"
    if1, out1, forms1, _ = _run(case, [n], False)
    if2, out2, forms2, _ = _run(case, cuts, False)
    if3, out3, forms3, st3 = _run(case, cuts, True)
    print("\n[%s] %s: pass forms %s | ragged %s | tick roles %s pass_blocks %d" % (row.id, backend, sorted(forms1), sorted(forms2), sorted(st3["roles"]), st3["pass_blocks"]))
    # ---- the forms this row exists for ----
    for f in sorted(row.forms_pass):
        assert forms1.get(f, 0) > 0 and forms2.get(f, 0) > 0, ("ordinary pass never launched " + f, forms1, forms2)
    if row.tick:
        assert st3["pass_blocks"] == 0 and st3["tick_blocks"] == len(cuts), st3
        assert not forms3, ("a pipelined run launched ordinary-pass forms", forms3)
        for f in sorted(row.roles_tick):
            assert st3["roles"].get(f, 0) > 0, ("no tick ran role " + f, st3["roles"])
    else:  # a form without a tick role: every block that needs it falls back to an ordinary pass, and says so
        assert st3["pass_blocks"] > 0, st3
        for f in sorted(row.forms_pass):
            assert forms3.get(f, 0) > 0, ("fallen-back blocks never launched " + f, forms3)
    worst = dict(base_if=0.0, got_if=0.0, base_a=0.0, got_a=0.0)
    for i, (d, keep, p, offset, oargs) in enumerate(case["descs"]):
        raw = p["demod"] == -1
        # ---- pipelined == ordinary, bit for bit, over the same pushes ----
        if raw:
            _bits_equal(if2[i].view(np.float32), if3[i].view(np.float32), "%s vfo %d IF: tick vs pass" % (row.id, i))
        else:
            _bits_equal(out2[i], out3[i], "%s vfo %d output: tick vs pass" % (row.id, i))
        # ---- float64 restatement, float32 sequential baseline ----
        r_if, r_a = restate64(p, x)
        if oargs is not None:
            ch = S.OracleChain(*oargs, ideal_nco=True)
            b_if, b_a = ch.process(x)
            b_a = b_a[:, 0] if p["demod"] in (0, 1) else demod_am_ssb(p, b_if, np.float32)  # (AM / USB: the AGC is pinned, the oracle's is not)
            ch.close()
        else:
            b_if, b_a = baseline32_hand(p, x, case["sr"], offset)
        base_if = dist(b_if, r_if)
        assert base_if < BASELINE_MAX, ("ill-conditioned input: float32 sequential IF baseline", row.id, i, base_if)
        for name, g in (("one push", if1[i]), ("ragged", if2[i])):
            e = dist(g, r_if)
            worst["got_if"] = max(worst["got_if"], e)
            assert e <= MARGIN * base_if, (row.id, "vfo %d IF, %s: %.3g against a float32 sequential baseline of %.3g" % (i, name, e, base_if),
                                           int(np.argmax(np.abs(g.astype(np.complex128) - r_if))), len(g))
        worst["base_if"] = max(worst["base_if"], base_if)
        assert base_if <= 1.25 * BASELINES[row.id][0], ("the float32 sequential IF baseline moved up: the bar may not loosen unseen", row.id, i, base_if, BASELINES[row.id][0])
        # push-size invariance (test_push_size_invariance: only the NCO's double-precision phase origin moves), scaled to the stream's level
        assert np.max(np.abs(if1[i] - if2[i])) < 2e-7 * max(1.0, rms(r_if) / 0.05), (row.id, i, float(np.max(np.abs(if1[i] - if2[i]))))
        if not raw:
            base_a = dist(b_a, r_a)
            assert base_a < BASELINE_MAX, ("ill-conditioned input: float32 sequential audio baseline", row.id, i, base_a)
            for name, g in (("one push", out1[i]), ("ragged", out2[i])):
                assert np.array_equal(g[:, 0], g[:, 1])
                e = dist(g[:, 0], r_a)
                worst["got_a"] = max(worst["got_a"], e)
                assert e <= MARGIN * base_a, (row.id, "vfo %d audio, %s: %.3g against a float32 sequential baseline of %.3g" % (i, name, e, base_a),
                                              int(np.argmax(np.abs(g[:, 0].astype(np.float64) - r_a))), len(g))
            worst["base_a"] = max(worst["base_a"], base_a)
            assert base_a <= 1.25 * BASELINES[row.id][1], ("the float32 sequential audio baseline moved up: the bar may not loosen unseen", row.id, i, base_a, BASELINES[row.id][1])
            assert np.max(np.abs(out1[i] - out2[i])) < 2e-6 * max(1.0, rms(r_a)), (row.id, i, float(np.max(np.abs(out1[i] - out2[i]))))
        # ---- the project's existing bars against the pinned oracle (rows the reference's own plans reach) ----
        if oargs is not None:
            ch = S.OracleChain(*oargs)
            o_if, o_a = ch.process(x)
            ch.close()
            assert rms(if1[i] - b_if) / rms(b_if) < 2e-6 and rms(if1[i] - o_if) / rms(o_if) < 2e-3, (row.id, rms(if1[i] - b_if) / rms(b_if), rms(if1[i] - o_if) / rms(o_if))
            if p["demod"] in (0, 1):  # (AM / USB rows run with the AGC pinned, which the oracle's demodulator cannot: their audio is checked per sample above)
                assert rms(out1[i] - o_a) < 1e-5 and rms(out2[i] - o_a) < 1e-5, (row.id, rms(out1[i] - o_a), rms(out2[i] - o_a))
    print("[%s] %s per-sample max-abs / rms: IF baseline %.3g library %.3g (bar %.3g) | audio baseline %.3g library %.3g (bar %.3g)" % (
        row.id, backend, worst["base_if"], worst["got_if"], MARGIN * worst["base_if"], worst["base_a"], worst["got_a"], MARGIN * worst["base_a"]))


# ---- FFT / zoom roles the other tests do not name ---------------------------------------------------------------------------------------------
FFT_ROLES = {10: ("fft_s10", "zoom_1"), 11: ("fft_s11", "zoom_1"), 12: ("fft_s12", "zoom_1"), 13: ("fft_p1_6", "fft_p2_7", "zoom_4"), 14: ("fft_p1_7", "fft_p2_7", "zoom_4"),
             15: ("fft_p1_7", "fft_p2_8", "zoom_16"), 16: ("fft_p1_8", "fft_p2_8", "zoom_16"), 17: ("fft_p1_5", "fft_p2row", "fft_tr", "zoom_16"),
             18: ("fft_p1_6", "fft_p2row", "fft_tr", "zoom_16"), 19: ("fft_p1_7", "fft_p2row", "fft_tr", "zoom_16"), 20: ("fft_p1_8", "fft_p2row", "fft_tr", "zoom_16")}


@pytest.mark.parametrize("lg", list(range(10, 21)))
def test_fft_and_zoom_roles_by_size(backend, lg):
    """2^10 ... 2^20-point transforms, pipelined against the ordinary pass (which test_every_fft_size_bit_exact pins bit-exactly to the oracle):
    raw lines, zoomed lines and palette indices identical, no block falls back, and the roles of that size ran."""
    from sdrplusplus_amd import capi

    N = 1 << lg
    reps = 2 if lg <= 16 else 1
    pushes = [N // 2 + 3, N * reps - N // 2 + 2]
    r = np.random.default_rng(100 + lg)
    n = sum(pushes)
    x = ((r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.01 + 0.5 * np.exp(2j * np.pi * 0.1234 * np.arange(n))).astype(np.complex64)
    res = []
    for pipelined in (False, True):
        ctx = capi.Context(0, max_push=max(pushes))
        ctx.fft_configure(N, N, 0, capi.design_fft_window(2, N))
        ctx.fft_set_view(N // 8, N // 2, 733, -110.0, -15.0)
        if pipelined:
            ctx.set_pipelined(True, 6)
        lines, pos = [], 0
        for c in pushes:
            ctx.push(x[pos:pos + c])
            pos += c
            if not pipelined:
                lines.append(ctx.fft_read())
        if pipelined:
            for t in range(1, len(pushes) + 1):
                g = ctx.result_wait(t)
                lines.append((g["raw"], g["zoomed"], g["index"]) if g["n_lines"] else (np.zeros((0, N), np.float32), None, None))
                ctx.result_release(t)
        res.append((lines, ctx.pipeline_stats()))
        ctx.close()
    (la, _), (lb, st) = res
    total = 0
    for (ra, za, ia), (rb, zb, ib) in zip(la, lb):
        assert len(ra) == len(rb)
        total += len(ra)
        if len(ra):
            assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)) and np.array_equal(za.view(np.uint32), zb.view(np.uint32)) and np.array_equal(ia, ib)
    assert total == reps
    assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(pushes), st
    print("\n[fft 2^%d] %s roles %s" % (lg, backend, sorted(st["roles"])))
    for role in FFT_ROLES[lg]:
        assert st["roles"].get(role, 0) > 0, (lg, role, st["roles"])


# ---- the ledger: no form without a test that names it -----------------------------------------------------------------------------------------
_HERE = "test_kernel_forms"
CLAIMS = {
    # role / form -> (test module, test function) whose source asserts that name
    "rot": (_HERE, "ROWS"), "fcm_6": (_HERE, "ROWS"), "fcm_10": (_HERE, "ROWS"), "fcm_16": (_HERE, "ROWS"), "fcl_0": (_HERE, "ROWS"), "fcl_pf": (_HERE, "ROWS"),
    "toep_c": (_HERE, "ROWS"), "firb_c": (_HERE, "ROWS"), "polyc": (_HERE, "ROWS"), "poly": (_HERE, "ROWS"), "s1_1": (_HERE, "ROWS"), "s1d_1": (_HERE, "ROWS"),
    "f2_1": (_HERE, "ROWS"), "polyb_4": (_HERE, "ROWS"), "polyb_8": (_HERE, "ROWS"), "polyb_4_odd": (_HERE, "ROWS"), "polyb_8_odd": (_HERE, "ROWS"),
    "s1_8": (_HERE, "ROWS"), "s1_4": (_HERE, "ROWS"), "s1_2": (_HERE, "ROWS"), "s1d_8": (_HERE, "ROWS"), "s1d_4": (_HERE, "ROWS"), "s1d_2": (_HERE, "ROWS"),
    "f2_8": (_HERE, "ROWS"), "f2_4": (_HERE, "ROWS"), "f2_2": (_HERE, "ROWS"),
    "firb_q": (_HERE, "ROWS"), "firb_s": (_HERE, "ROWS"), "fft_p2_7": (_HERE, "FFT_ROLES"), "zoom_16": (_HERE, "FFT_ROLES"),
    "ifc": ("test_ifchain", "test_pipelined_and_grouped_equal_the_ordinary_path"),
    "deemp_p0": ("test_pipelined", "test_pipelined_equals_ordinary_with_af_chain"), "deemp_p1": ("test_pipelined", "test_pipelined_equals_ordinary_with_af_chain"),
    "wf_ring": ("test_pipelined", "test_pipelined_equals_ordinary_with_waterfall_state"), "wf_trace": ("test_pipelined", "test_pipelined_equals_ordinary_with_waterfall_state"),
    "dc_p0": ("test_pipelined", "test_pipelined_equals_ordinary_with_preproc_chain"), "dc_p1": ("test_pipelined", "test_pipelined_equals_ordinary_with_preproc_chain"),
    "toep_r": (_HERE, "test_mode_roles"), "toep_q": (_HERE, "test_mode_roles"), "pre": (_HERE, "test_mode_roles"), "seq": (_HERE, "test_mode_roles"),
    "carry": (_HERE, "test_mode_roles"), "copy": (_HERE, "test_mode_roles"), "f2_8_44_3": (_HERE, "test_mode_roles"), "fcm_132_4": (_HERE, "test_mode_roles"),
    "pipe": (_HERE, "test_mode_roles"),
    "fft_s10": (_HERE, "FFT_ROLES"), "fft_s11": (_HERE, "FFT_ROLES"), "fft_s12": (_HERE, "FFT_ROLES"), "fft_p1_5": (_HERE, "FFT_ROLES"), "fft_p1_6": (_HERE, "FFT_ROLES"),
    "fft_p1_7": (_HERE, "FFT_ROLES"), "fft_p1_8": (_HERE, "FFT_ROLES"), "fft_p2_8": (_HERE, "FFT_ROLES"), "fft_p2row": (_HERE, "FFT_ROLES"), "fft_tr": (_HERE, "FFT_ROLES"),
    "zoom_4": (_HERE, "FFT_ROLES"), "zoom_1": (_HERE, "FFT_ROLES"),
    "fcm16_132_4": ("test_bench_geometry_gpu", "test_cfg3_pipelined_bench_geometry_vs_oracle"),
    "rotx16": ("test_pipelined", "test_reference_rotator_vfos_stay_in_the_tick"), "fird": ("test_pipelined", "test_reference_rotator_vfos_stay_in_the_tick"),
    "ssbx": ("test_pipelined", "test_reference_rotator_vfos_stay_in_the_tick"),
    "rotx_1": ("test_parity_vfo", "test_reference_rotator_four_wavefront_kernel_is_bit_identical"),
}
EXEMPT = {
    "none": "TR_NONE: the empty entry of a tick table, not a kernel",
    "firb_r": "unreachable: launch_fir emits TR_FIRB_R only for width == 1 && !stereo && !quad, and its width-1 callers (audio, audio_fm) both pass stereo = true",
    "fft_p1_9": "unreachable: fft_split gives lg1 = m / 2 <= 8 for 13 <= m <= 16 and lg1 = m - 12 <= 8 for 17 <= m <= 20 (sdrpp_fft_configure refuses fft_size > 2^20)",
    "fft_p1_10": "unreachable: fft_split gives lg1 = m / 2 <= 8 for 13 <= m <= 16 and lg1 = m - 12 <= 8 for 17 <= m <= 20 (sdrpp_fft_configure refuses fft_size > 2^20)",
    "fft_p2_9": "unreachable: fft_split gives lg2 = m - m / 2 in {7, 8} for 13 <= m <= 16 and lg2 = 12 (fft_p2row) above; 9 would need m = 17 or 18 in the even split",
    "fft_p2_10": "unreachable: fft_split gives lg2 = m - m / 2 in {7, 8} for 13 <= m <= 16 and lg2 = 12 (fft_p2row) above; 10 would need m = 19 or 20 in the even split",
}


def test_mode_roles(backend):
    """The roles a mixed bank brings that no row above names: WFM x 20 at 10 MS/s (fcm_132_4 in a tick, the unrolled f2_8_44_3 of a 10-VFO bank in a pass, toep_q audio, the FM back end as ONE launch — `pipe`, ordinary passes only) and AM (toep_r audio, pre, seq), with the
    history carries and the result copies of every tick."""
    from sdrplusplus_amd import capi, radio, workloads

    sr = 10e6
    n = 50000 if backend == "gpu" else 12000
    specs = [("WFM", (k - 9.5) * 300e3) for k in range(20)] + [("AM", 4.1e6)]
    x = _fm_mix(sr, 2 * n, [f for _, f in specs], 9, 40e3, amp=0.04)
    out = []
    for pipelined in (False, True):
        ctx = capi.Context(0, max_push=n)
        vids = []
        for mode, f in specs if pipelined else specs[:10] + specs[20:]:  # (an ordinary pass with 10 WFM VFOs: too few for the matrix front end)
            d, keep = radio.vfo_desc(sr, *radio.RADIO_DEFAULTS[mode], f, mode)
            vids.append(ctx.vfo_add(d, keep))
        if pipelined:
            ctx.set_pipelined(True, 1)
        for b in range(2):
            ctx.push(x[b * n:(b + 1) * n])
        if pipelined:
            for t in (1, 2):
                ctx.result_wait(t)
                ctx.result_release(t)
        out.append((ctx.pass_form_stats(), ctx.pipeline_stats()))
        ctx.close()
    (forms, _), (tick_forms, st) = out
    print("\n[mode roles] %s pass forms %s | tick roles %s" % (backend, sorted(forms), sorted(st["roles"])))
    assert st["pass_blocks"] == 0 and not tick_forms, (st, tick_forms)
    for name in ("f2_8_44_3", "pipe", "toep_r", "pre", "seq", "carry"):
        assert forms.get(name, 0) > 0, (name, forms)
    for name in ("fcm_132_4", "toep_q", "toep_r", "pre", "seq", "carry", "copy"):
        assert st["roles"].get(name, 0) > 0, (name, st["roles"])


def _all_forms():
    from sdrplusplus_amd import capi
    import os

    capi.DEFAULT_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdrplusplus_amd", "csrc", "libsdrpp_gpu.so")
    names = capi.pass_form_names()
    L = capi.load()
    roles = []
    while L.sdrpp_pipeline_role_name(len(roles)) is not None:
        roles.append(L.sdrpp_pipeline_role_name(len(roles)).decode())
    assert names[:len(roles)] == roles and len(names) > len(roles), (names, roles)
    return names


def _claim_holds(name, module, func):
    """A claim on a table of this module holds when a row REQUIRES the form (ROWS: in forms_pass, which the row's test asserts launch by launch; FFT_ROLES:
    in a size's tuple); a claim on a test function when the quoted name stands in an assert statement of its source, or in the tuple of a `for` loop whose
    body's first statement is an assert."""
    import importlib
    import re

    if (module, func) == (_HERE, "ROWS"):
        return any(name in r.forms_pass for r in ROWS)
    if (module, func) == (_HERE, "FFT_ROLES"):
        return any(name in v for v in FFT_ROLES.values())
    obj = getattr(importlib.import_module(module), func, None)
    assert callable(obj), "%s.%s does not exist" % (module, func)
    lines = inspect.getsource(obj).split("\n")
    quoted = re.compile(r"[\"']%s[\"']" % re.escape(name))
    for k, line in enumerate(lines):
        if not quoted.search(line):
            continue
        st = line.strip()
        if st.startswith("assert "):
            return True
        if st.startswith("for ") and k + 1 < len(lines) and lines[k + 1].strip().startswith("assert "):
            return True
    return False


def test_ledger_every_form_is_claimed_or_exempt():
    """Every role of the tick kernel and every extra form of the ordinary pass has a test that asserts it ran (CLAIMS: the named function or table
    exists and its source names the form in an assertion) or a written exemption (EXEMPT).  A role added to TickRole without either fails here."""
    import re

    names = _all_forms()
    assert len(set(names)) == len(names)
    for name in names:
        if name in EXEMPT:
            assert len(EXEMPT[name]) > 20 and name not in CLAIMS, name
            continue
        assert name in CLAIMS, "kernel form '%s' has neither a test that asserts it nor an exemption" % name
        assert _claim_holds(name, *CLAIMS[name]), "%s.%s does not assert '%s'" % (CLAIMS[name] + (name,))
    stale = [k for k in list(CLAIMS) + list(EXEMPT) if k not in names]
    assert not stale, ("ledger entries for forms that no longer exist", stale)
