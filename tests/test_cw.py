"""The radio's CW mode on the device (SDRPP_DEMOD_CW; decoder_modules/radio/src/demodulators/cw.h over dsp/demod/cw.h) and the ground its numbers lead onto:
3 kS/s IF behind captures of up to 24.576 MS/s (plan 8192: /128 with 726 taps, /8, /4, /2), resamplers of 375 and 3 000 phases, a channel filter of 4 560
taps at the mode's minimum bandwidth, sr / 200 blocks of 15 IF samples and pushes that give no IF sample at all, an AF chain that goes UP (3 000 -> 48 000).

THE REFERENCE.  dsp::demod::CW(tone) is statement for statement dsp::demod::SSB(USB, bandwidth = 2 * tone): one FrequencyXlator by `tone`, ComplexToReal,
loop::AGC(1.0, attack, decay, 10e6, 10.0, INFINITY), MonoToStereo.  tests/golden/cw_ref.npz holds what the reference's real CW<stereo_t> gave
(make_cw_golden.py); the first two tests pin the pinned oracle's — and, where it is built, the compiled reference's — USB entry with bandwidth 1 600 Hz to
those records bit for bit.  After that the USB entry IS the CW reference: the yardstick below is orc_rxvfo (bandwidth = the channel's) + orc_demod(USB, 2 *
tone, 3 000, attack 100, decay 5).

BARS.  Parity: the project's USB bar, audio RMS within 1e-5 of the yardstick — with nco_mode = 2 (the reference's rotator) against the pinned yardstick over
the whole stream, with the closed-form NCO against the yardstick with its ideal-NCO switch.  Per sample (resampler extremes, the /128 stage): test_kernel_forms'
bar, MARGIN x the float32-sequential baseline against the float64 restatement, both imported; the baselines of the rows added here are measured at run time
and recorded in BASELINES under the same 1.25 x rule.  Bit for bit wherever two paths of the device compute the same thing (ordinary pass, pipelined, launch
groups)."""
import os

import numpy as np
import pytest

import support as S
import test_af_chain as AF
from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_kernel_forms import BASELINE_MAX, MARGIN, _bits_equal, _fm_mix, _parts, _run, _spread, baseline32_hand, demod_am_ssb, dist, hand_desc, pin_agc, ragged, restate64, rms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cw_ref.npz")
IF_RATE, TONE, BW = 3000.0, 800.0, 200.0
ATTACK, DECAY = 100.0, 5.0  # demodulators/cw.h:105-106
UNSUPPORTED = -5
USB = S.MODES["USB"]


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------------
class Yard:
    """orc_rxvfo(in_sr -> 3 000, bandwidth, offset) + orc_demod(USB, 2 * tone): the CW chain out of pinned pieces.  ideal: both translations with the
    oracle's float64 NCO (the closed-form comparison)."""

    def __init__(self, in_sr, bw, offset, tone=TONE, attack=ATTACK, decay=DECAY, ideal=False):
        self.O, self.ideal = S.oracle(), ideal
        self.vfo = self.O.orc_rxvfo_create(S.plans_handle(), in_sr, IF_RATE, bw, offset)
        if ideal:
            self.O.orc_rxvfo_set_ideal_nco(self.vfo, 1)
        self.dem = self.O.orc_demod_create(USB, 2.0 * tone, IF_RATE, 0, attack, decay, 0)
        if ideal:
            self.O.orc_demod_set_ideal_nco(self.dem, 1)

    def set_bandwidth(self, bw):
        self.O.orc_rxvfo_set_bandwidth(self.vfo, float(bw))

    def block(self, iq):
        """one reference block -> (IF, audio [n, 2])"""
        iq = S.c64(iq)
        ifs = np.empty(len(iq) + 16, np.complex64)
        n = self.O.orc_rxvfo_process(self.vfo, len(iq), S._fp(iq.view(np.float32)), S._fp(ifs.view(np.float32)))
        ifs = ifs[:n].copy()
        a = np.empty((n + 1, 2), np.float32)
        if n:
            self.O.orc_demod_process(self.dem, n, S._fp(ifs.view(np.float32)), S._fp(a))
        return ifs, a[:n].copy()

    def push(self, iq, ref_block):
        """a push as the device cuts it: consecutive reference blocks of `ref_block` samples, the last one shorter (0: the push is one block)"""
        step = ref_block if ref_block > 0 else max(len(iq), 1)
        parts = [self.block(iq[lo:lo + step]) for lo in range(0, len(iq), step)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def close(self):
        self.O.orc_rxvfo_destroy(self.vfo)
        self.O.orc_demod_destroy(self.dem)


def keyed(sr, n, f0, seed, amp=0.3, noise=0.002, dot=0.06, beat=20.0):
    """Morse-like keying of a carrier `beat` Hz above f0 (dots of `dot` seconds, one mark in four a dash), plus noise; float64 maths, one rounding."""
    r = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    unit = max(int(dot * sr), 1)
    key = np.zeros(n)
    pos = unit // 2
    while pos < n:
        mark = unit * (3 if r.integers(0, 4) == 0 else 1)
        key[pos:pos + mark] = 1.0
        pos += mark + unit * int(r.integers(1, 4))
    return amp * key * np.exp(2j * np.pi * (f0 + beat) * t) + noise * (r.standard_normal(n) + 1j * r.standard_normal(n))


def cw_desc(in_sr, bw, offset, nco_mode=0, tone=TONE, **kw):
    from sdrplusplus_amd import radio

    return radio.vfo_desc(in_sr, IF_RATE, bw, offset, "CW", nco_mode=nco_mode, tone=tone, **kw)


def audio_err(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return rms(got - want) / max(1.0, rms(want))


# ---- 0. the fixture pins the USB entries ------------------------------------------------------------------------------------------------------
def _golden_case(z, name):
    x = (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
    return x, [int(c) for c in z[name + "_cut"]], z[name + "_ops"], z[name + "_audio"]


def _usb_entry_over(lib, prefix, x, cut):
    dem = getattr(lib, prefix + "demod_create")(USB, 2.0 * TONE, IF_RATE, 0, ATTACK, DECAY, 0)
    out, pos = [], 0
    for n in cut:
        blk = np.ascontiguousarray(x[pos:pos + n])
        a = np.empty((n + 1, 2), np.float32)
        assert getattr(lib, prefix + "demod_process")(dem, n, S._fp(blk.view(np.float32)), S._fp(a)) == n
        assert np.array_equal(a[:n, 0].view(np.uint32), a[:n, 1].view(np.uint32))
        out.append(a[:n, 0].copy())
        pos += n
    getattr(lib, prefix + "demod_destroy")(dem)
    return np.concatenate(out)


@pytest.mark.parametrize("name", ["steady", "cuts"])
def test_oracle_usb_entry_is_the_recorded_cw(name):
    """orc_demod_create(USB, 2 * tone, 3000, attack 100, decay 5) over the fixture's inputs with its block schedule (blocks of 15; ragged cuts with 1-sample
    blocks) gives what the reference's dsp::demod::CW<stereo_t> recorded, bit for bit."""
    x, cut, ops, want = _golden_case(np.load(GOLDEN), name)
    assert len(ops) == 0 and len(want) == len(x) > 2000 and (name != "cuts" or 1 in cut)
    got = _usb_entry_over(S.oracle(), "orc_", x, cut)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


@pytest.mark.skipif(not S.ref_available(), reason="oracle/_ref not built (needs the reference tree at build time)")
@pytest.mark.parametrize("name", ["steady", "cuts"])
def test_reference_usb_entry_is_the_recorded_cw(name):
    """ref_demod_create(REF_USB, 2 * tone, 3000, ...) — the reference's own SSB<stereo_t>, compiled — against the same records: CW is SSB(USB, 2 * tone)."""
    x, cut, _, want = _golden_case(np.load(GOLDEN), name)
    got = _usb_entry_over(S.ref(), "ref_", x, cut)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name


# ---- 1. the demodulator alone: 48 kS/s -> 3 kS/s, plan 16, no resampler -------------------------------------------------------------------------
SR1, N1, F1 = 48000.0, 240 * 267, 5000.0
RAGGED1 = [1, 7, 15, 3, 240, 11, 997, 2, 5, 4801, 13, 1, 9, 2400, 14, 12000, 6, 8, 20000]
RAGGED1 = RAGGED1 + [N1 - sum(RAGGED1)]


def _cw_run(x, in_sr, bw, offset, nco_mode, cuts, ref_block, pipelined=False, group=0):
    """one CW VFO over `cuts` -> (audio per push, IF per push or None, pass forms, pipeline stats)"""
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max(cuts) * max(1, group))
    ctx.set_reference_block(ref_block)
    d, keep = cw_desc(in_sr, bw, offset, nco_mode)
    vid = ctx.vfo_add(d, keep)
    if pipelined:
        ctx.set_pipelined(True, 1)
        if group:
            ctx.set_pipeline_group(group)
    audio, ifs, pos = [], [], 0
    for c in cuts:
        ctx.push(x[pos:pos + c])
        pos += c
        if not pipelined:
            audio.append(ctx.vfo_read(vid).copy())
            ifs.append(ctx.vfo_read_if(vid).copy())
            assert len(audio[-1]) == ctx.vfo_out_count(vid) == len(ifs[-1])
    if pipelined:
        for t in range(1, len(cuts) + 1):
            audio.append(ctx.result_wait(t)["vfo"][vid])
            ctx.result_release(t)
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    ctx.close()
    return audio, (None if pipelined else ifs), forms, st


@pytest.mark.parametrize("nco_mode", [1, 2], ids=["closed_form", "rotator"])
def test_cw_alone_one_push_blocks_and_ragged(backend, nco_mode):
    """One CW VFO, bandwidth 200, tone 800, ~64 000 samples at 48 kS/s, as ONE push, as sr / 200 pushes of 240 (15 IF samples each) and ragged with pushes of
    1 .. 15 samples that give no IF sample: per-push counts equal the yardstick's, audio within 1e-5.  The ragged run again pipelined and in launch groups of
    3: the same bits as the ordinary pass, no block falls back."""
    x = keyed(SR1, N1, F1, 11).astype(np.complex64)
    assert sum(RAGGED1) == N1 and min(RAGGED1) >= 1
    for name, cuts, ref_block in (("one push", [N1], 0), ("blocks of 240", [240] * (N1 // 240), 240), ("ragged", RAGGED1, 240)):
        audio, ifs, forms, _ = _cw_run(x, SR1, BW, F1, nco_mode, cuts, ref_block)
        y = Yard(SR1, BW, F1, ideal=(nco_mode == 1))
        want, pos = [], 0
        for c in cuts:
            want.append(y.push(x[pos:pos + c], ref_block))
            pos += c
        y.close()
        assert [len(a) for a in audio] == [len(w[1]) for w in want], (name, "samples per push")
        if name == "ragged":
            assert sum(1 for c, a in zip(cuts, audio) if c <= 15 and len(a) == 0) >= 6, "short pushes that give no IF sample"
        if name == "blocks of 240":
            assert all(len(a) == 15 for a in audio)
        ga, wa = np.concatenate(audio), np.concatenate([w[1] for w in want])
        gi, wi = np.concatenate(ifs), np.concatenate([w[0] for w in want])
        assert len(ga) == N1 // 16 and np.array_equal(ga[:, 0], ga[:, 1])
        e_a, e_if = audio_err(ga, wa), rms(gi - wi) / rms(wi)
        print("\n[cw alone] %s nco %d %s: audio %.3g IF %.3g forms %s" % (backend, nco_mode, name, e_a, e_if, sorted(forms)))
        assert e_a < 1e-5 and e_if < 2e-6, (name, e_a, e_if)
        assert forms.get("seq", 0) > 0 and forms.get("ssbx" if nco_mode == 2 else "pre", 0) > 0, forms
        if name == "ragged":
            base = audio
    for what, group in (("pipelined", 0), ("grouped", 3)):
        audio, _, forms, st = _cw_run(x, SR1, BW, F1, nco_mode, RAGGED1, 240, pipelined=True, group=group)
        assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(RAGGED1) and not forms, (what, st, forms)
        assert st["roles"].get("seq", 0) > 0 and st["roles"].get("ssbx" if nco_mode == 2 else "pre", 0) > 0, st["roles"]
        for k, (a, b) in enumerate(zip(base, audio)):
            _bits_equal(a, b, "%s vs ordinary, push %d" % (what, k))


# ---- 2. controls: setTone, the AGC setters, replace, the demodulator switch --------------------------------------------------------------------
def _golden_on_device(name, nco_mode, replace_at=()):
    """A VFO of 3 kS/s -> 3 kS/s with bandwidth = rate and offset 0 (no stage, no resampler, no channel filter: its IF is its input) fed the fixture's inputs
    with its block schedule and its setter calls: setTone through sdrpp_vfo_set_ssb_phase_delta, the AGC setters through sdrpp_vfo_replace with keep = 3."""
    from sdrplusplus_amd import capi

    x, cut, ops, want = _golden_case(np.load(GOLDEN), name)
    ctx = capi.Context(0, max_push=max(cut))
    d, keep = cw_desc(IF_RATE, IF_RATE, 0.0, nco_mode)
    assert d.n_stages == 0 and d.interp == d.decim and d.chan_ntaps == 0 and d.demod == capi.DEMOD_CW
    assert d.agc_attack == np.float32(ATTACK / IF_RATE) and d.agc_decay == np.float32(DECAY / IF_RATE), "CW's own AGC defaults (cw.h:105-106)"
    vid = ctx.vfo_add(d, keep)
    out, pos = [], 0
    for b, n in enumerate(cut):
        for ob, setter, value in ops:
            if int(ob) != b:
                continue
            if int(setter) == 0:
                ctx.vfo_set_ssb_phase_delta(vid, *capi.design_phase_delta(float(value), IF_RATE))
            else:
                if int(setter) == 1:
                    d.agc_attack = np.float32(value / IF_RATE)
                else:
                    d.agc_decay = np.float32(value / IF_RATE)
                vid = ctx.vfo_replace(vid, d, 3, keep)
        if b in replace_at:
            vid = ctx.vfo_replace(vid, d, 3, keep)
        ctx.push(x[pos:pos + n])
        a = ctx.vfo_read(vid)
        assert len(a) == n and np.array_equal(a[:, 0], a[:, 1])
        out.append(a[:, 0].copy())
        pos += n
    ctx.close()
    return np.concatenate(out), want, len(ops)


@pytest.mark.parametrize("nco_mode", [1, 2], ids=["closed_form", "rotator"])
@pytest.mark.parametrize("name", ["steady", "cuts", "tone", "agc"])
def test_cw_controls_against_the_recorded_reference(backend, name, nco_mode):
    """The reference's CW over blocks of 15, over ragged cuts with 1-sample blocks, through setTone(800 -> 600) and through setAGCAttack / setAGCDecay in
    mid-stream (the tone translation's phase and the AGC's amplitude estimate live on), reproduced by the device within 1e-5 of the record's RMS — the
    steady case a second time with sdrpp_vfo_replace(keep = 3) CW -> CW between blocks, which must change nothing."""
    got, want, nops = _golden_on_device(name, nco_mode)
    assert nops == {"steady": 0, "cuts": 0, "tone": 1, "agc": 3}[name]
    e = rms(got - want) / max(1.0, rms(want))
    print("\n[cw golden] %s %s nco %d: %.3g of rms %.3g" % (backend, name, nco_mode, e, rms(want)))
    assert e < 1e-5, (name, e)
    if name == "steady":
        got2, _, _ = _golden_on_device(name, nco_mode, replace_at=(50, 51, 120))
        assert np.array_equal(got2.view(np.uint32), got.view(np.uint32)), "vfo_replace CW -> CW with keep = 3 is the same demodulator"


def test_cw_set_tone_and_refusals(backend):
    """sdrpp_vfo_set_ssb_phase_delta serves CW::setTone on a CW VFO and is refused on an AM one; a seventh demodulator code is refused by sdrpp_vfo_add."""
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=4096)
    d, keep = cw_desc(SR1, BW, F1)
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_ssb_phase_delta(vid, *capi.design_phase_delta(600.0, IF_RATE))
    da, ka = radio.vfo_desc(SR1, 15000.0, 10000.0, F1, "AM")
    am = ctx.vfo_add(da, ka)
    with pytest.raises(capi.SdrppError):
        ctx.vfo_set_ssb_phase_delta(am, 1.0, 0.0)
    d.demod = 7
    with pytest.raises(capi.SdrppError):
        ctx.vfo_add(d, keep)
    assert radio.RADIO_DEFAULTS["CW"] == (3000.0, 200.0) and radio.DEMOD_CODES["CW"] == capi.DEMOD_CW == 6
    ctx.close()


def test_mode_switch_usb_cw_usb_follows_the_reference(backend):
    """The radio's mode switch USB -> CW -> USB on one channel (RxVFO::setOutSamplerate, then a NEW demodulator: radio_module.h:419-563; sdrpp_vfo_replace
    with keep = 1) against the COMPILED REFERENCE's own RxVFO and SSB objects: audio and IF of every block from its first sample."""
    from sdrplusplus_amd import capi, radio

    if not S.ref_available():
        pytest.skip("oracle/_ref not built (needs the reference tree at build time)")
    R = S.ref()
    sr, B, off = 48000.0, 2400, 6000.0  # (off = sr / 8: phase steps exact in float, no rotator drift between the closed form and the reference)
    x = keyed(sr, 12 * B, off, 5, dot=0.02).astype(np.complex64)
    ctx = capi.Context(0, max_push=B)
    d, keep = radio.vfo_desc(sr, 24000.0, 2800.0, off, "USB")
    vid = ctx.vfo_add(d, keep)
    vfo = R.ref_rxvfo_create(sr, 24000.0, 2800.0, off)
    dem = R.ref_demod_create(USB, 2800.0, 24000.0, 0, 50.0, 5.0, 0)
    for b in range(12):
        if b in (4, 9):
            R.ref_demod_destroy(dem)
            if b == 4:
                R.ref_rxvfo_set_out_samplerate(vfo, IF_RATE, BW)
                dem = R.ref_demod_create(USB, 2.0 * TONE, IF_RATE, 0, ATTACK, DECAY, 0)
                d, keep = cw_desc(sr, BW, off)
            else:
                R.ref_rxvfo_set_out_samplerate(vfo, 24000.0, 2800.0)
                dem = R.ref_demod_create(USB, 2800.0, 24000.0, 0, 50.0, 5.0, 0)
                d, keep = radio.vfo_desc(sr, 24000.0, 2800.0, off, "USB")
            vid = ctx.vfo_replace(vid, d, 1, keep)
        blk = x[b * B:(b + 1) * B]
        ctx.push(blk)
        gi, ga = ctx.vfo_read_if(vid), ctx.vfo_read(vid)
        oi = np.empty(B + 16, np.complex64)
        n = R.ref_rxvfo_process(vfo, B, S._fp(blk.view(np.float32)), S._fp(oi.view(np.float32)))
        oi = oi[:n].copy()
        assert gi.shape == oi.shape and rms(gi - oi) / max(rms(oi), 1e-9) < 5e-6, (b, "IF", rms(gi - oi) / max(rms(oi), 1e-9))
        oa = np.empty((n + 1, 2), np.float32)
        R.ref_demod_process(dem, n, S._fp(oi.view(np.float32)), S._fp(oa))
        oa = oa[:n]
        assert ga.shape == oa.shape and audio_err(ga, oa) < 1e-5, (b, audio_err(ga, oa))
    R.ref_rxvfo_destroy(vfo)
    R.ref_demod_destroy(dem)
    ctx.close()


# ---- 3. resampler extremes: the smallest input rates that keep the ratio --------------------------------------------------------------------------
# (input rate, samples, the plan the reference's reconfigure chooses: (pre-decimation, interp, decim, taps per phase), the form its polyphase stage runs in)
# (the prototype filters have 1 900, 44 536 and 371 108 taps: compared with the oracle's count, whatever it is)
RESAMP_ROWS = [
    ("24over25", 50000.0, 12000, (16, 24, 25, 80), "polyc"),
    ("375over586", 4688.0, 4000, (1, 375, 586, 119), "polyc"),
    ("3000over4883", 4883.0, 4000, (1, 3000, 4883, 124), "poly"),
]
# float32-sequential baselines of the rows this file adds (max-abs / rms against the float64 restatement; measured on the CPU — the same figure on both legs):
# (IF, audio or None).  The bar is MARGIN x the baseline measured at run time, which may not exceed 1.25 x the figure recorded here.
BASELINES = {
    "24over25": (6.54e-06, 6.11e-06),
    "375over586": (2.89e-06, 3.9e-06),
    "3000over4883": (2.55e-06, 3.52e-06),
    "s128_nv2": (1.25e-06, None),
    "s128_nv16": (1.77e-06, None),
    "s128_nv17": (1.49e-06, None),
    "s128_nv32": (1.65e-06, None),
}


def _per_sample(rid, what, got, base, ref64, which):
    """the per-sample bar of test_kernel_forms: -> (baseline, library figure)"""
    b, e = dist(base, ref64), dist(got, ref64)
    assert b < BASELINE_MAX, ("ill-conditioned input: float32 sequential baseline", rid, what, b)
    assert e <= MARGIN * b, (rid, "%s: %.3g against a float32 sequential baseline of %.3g" % (what, e, b), int(np.argmax(np.abs(np.asarray(got).astype(ref64.dtype) - ref64))), len(got))
    assert b <= 1.25 * BASELINES[rid][which], ("the float32 sequential baseline moved up: the bar may not loosen unseen", rid, what, b, BASELINES[rid][which])
    return b, e


@pytest.mark.parametrize("rid,in_sr,n,plan,form", RESAMP_ROWS, ids=[r[0] for r in RESAMP_ROWS])
def test_resampler_extremes_sample_by_sample(backend, rid, in_sr, n, plan, form):
    """CW's 3 kS/s from 50 kS/s (24 / 25 behind /16), 4 688 S/s (375 / 586, no pre-decimation) and 4 883 S/s (3000 / 4883, 124 taps per phase): the plan
    is the reference's own (sdrpp_design_resampler against the oracle's reconfigure), the polyphase stage runs in the form the planner states for it, and
    every IF and audio sample (AGC pinned to unit gain) of a one-push and a ragged run meets the per-sample bar; pipelined equals ordinary bit for bit."""
    from sdrplusplus_amd import capi, radio

    offset = 0.21 * in_sr
    rs = capi.design_resampler(in_sr, IF_RATE, radio.plans().max_ratio)
    got_plan = (rs["predec"], rs["interp"], rs["decim"], (len(rs["taps"]) + rs["interp"] - 1) // rs["interp"])
    assert got_plan == plan, (rid, got_plan)
    ch = S.OracleChain(in_sr, IF_RATE, BW, offset, USB)
    info = S.oracle_rxvfo_info(ch)
    ch.close()
    assert (info["predec"], info["interp"], info["decim"], info["taps_per_phase"]) == plan and info["rtaps"] == len(rs["taps"]), (rid, info, len(rs["taps"]))
    d, keep = cw_desc(in_sr, BW, offset)
    pin_agc(d)
    p = _parts(d)
    p["demod"] = USB  # (the restatement's SSB branch: Re(IF x the stored second increment) — CW's arithmetic with the tone as that increment)
    assert p["ctaps"] is not None and len(p["ctaps"]) == 1140
    x = _fm_mix(in_sr, n, [offset], 41, 30.0, tone=90.0, amp=0.3)
    case = dict(sr=in_sr, n=n, descs=[(d, keep, p, offset, None)], x=x)
    cuts = ragged(n, 16 * plan[0] * 4)
    if1, out1, forms1, _ = _run(case, [n], False)
    if2, out2, forms2, _ = _run(case, cuts, False)
    _, out3, forms3, st3 = _run(case, cuts, True)
    print("\n[cw resampler %s] %s pass forms %s | tick roles %s pass_blocks %d" % (rid, backend, sorted(forms1), sorted(st3["roles"]), st3["pass_blocks"]))
    for f in (forms1, forms2):
        assert f.get(form, 0) > 0 and not [k for k in f if k.startswith("poly") and k != form], (rid, f)
    assert st3["pass_blocks"] == 0 and not forms3 and st3["roles"].get(form, 0) > 0, (rid, st3, forms3)
    _bits_equal(out2[0], out3[0], "%s: pipelined vs ordinary" % rid)
    r_if, r_a = restate64(p, x)
    ych = S.OracleChain(in_sr, IF_RATE, BW, offset, USB, ideal_nco=True)
    b_if, _ = ych.process(x)
    ych.close()
    b_a = demod_am_ssb(p, b_if, np.float32)
    assert len(r_if) == len(b_if) == len(if1[0]) == len(if2[0]) > 400
    worst = [0.0, 0.0, 0.0, 0.0]
    for what, gi, ga in (("one push", if1[0], out1[0]), ("ragged", if2[0], out2[0])):
        assert np.array_equal(ga[:, 0], ga[:, 1])
        bi, ei = _per_sample(rid, what + " IF", gi, b_if, r_if, 0)
        ba, ea = _per_sample(rid, what + " audio", ga[:, 0], b_a, r_a, 1)
        worst = [max(worst[0], bi), max(worst[1], ei), max(worst[2], ba), max(worst[3], ea)]
    print("[cw resampler %s] %s per-sample max-abs / rms: IF baseline %.3g library %.3g | audio baseline %.3g library %.3g (%d samples)" % ((rid, backend) + tuple(worst) + (len(r_if),)))


# ---- 4. the channel filter at CW's minimum bandwidth: lowPass(25, 2.5, 3000) has 4 560 taps ------------------------------------------------------
def test_channel_filter_4560_taps_parity(backend):
    """One CW VFO at bandwidth 50 Hz, 48 kS/s, reference rotator, 96 000 samples in reference blocks of 240: audio 1e-5, IF 2e-6 against the yardstick."""
    n = 96000
    x = keyed(SR1, n, F1, 17).astype(np.complex64)
    d, _ = cw_desc(SR1, 50.0, F1, 2)
    assert d.chan_ntaps == 4560
    cuts = [24000, 240 * 37 + 5, n - 24000 - 240 * 37 - 5]
    audio, ifs, forms, _ = _cw_run(x, SR1, 50.0, F1, 2, cuts, 240)
    y = Yard(SR1, 50.0, F1)
    want, pos = [], 0
    for c in cuts:
        want.append(y.push(x[pos:pos + c], 240))
        pos += c
    y.close()
    ga, wa = np.concatenate(audio), np.concatenate([w[1] for w in want])
    gi, wi = np.concatenate(ifs), np.concatenate([w[0] for w in want])
    e_a, e_if = audio_err(ga, wa), rms(gi - wi) / rms(wi)
    print("\n[cw 4560 taps] %s audio %.3g IF %.3g forms %s" % (backend, e_a, e_if, sorted(forms)))
    assert len(ga) == n // 16 and e_a < 1e-5 and e_if < 2e-6, (e_a, e_if)
    assert forms.get("firb_c", 0) > 0, forms


def test_channel_taps_1140_4560_456_mid_stream(backend):
    """RxVFO::setBandwidth 200 -> 50 -> 500 Hz while the stream runs (sdrpp_vfo_set_channel_taps: 1 140 -> 4 560 -> 456 taps): the delay line is carried as
    FIR::setTaps carries it (fir.h:31-52) — the longer filter starts with zeros in front of the old line — audio and IF of every block from its first sample."""
    from sdrplusplus_amd import capi

    B, nblk = 4800, 15
    x = keyed(SR1, B * nblk, F1, 19).astype(np.complex64)
    ctx = capi.Context(0, max_push=B)
    ctx.set_reference_block(240)
    d, keep = cw_desc(SR1, BW, F1, 2)
    vid = ctx.vfo_add(d, keep)
    y = Yard(SR1, BW, F1)
    for b in range(nblk):
        if b in (5, 10):
            bw = 50.0 if b == 5 else 500.0
            taps = capi.design_low_pass(bw / 2.0, bw / 20.0, IF_RATE)
            assert len(taps) == (4560 if b == 5 else 456)
            ctx.vfo_set_channel_taps(vid, taps)
            y.set_bandwidth(bw)
        blk = x[b * B:(b + 1) * B]
        ctx.push(blk)
        wi, wa = y.push(blk, 240)
        gi, ga = ctx.vfo_read_if(vid), ctx.vfo_read(vid)
        head = 40
        assert gi.shape == wi.shape and rms(gi - wi) / rms(wi) < 2e-6 and rms(gi[:head] - wi[:head]) / rms(wi) < 2e-6, (b, rms(gi - wi) / rms(wi))
        assert audio_err(ga, wa) < 1e-5 and audio_err(ga[:head], wa[:head]) < 1e-5, (b, audio_err(ga, wa))
    y.close()
    ctx.close()


def test_channel_filter_tap_bound(backend):
    """65 536 taps are taken, 65 537 are refused with SDRPP_ERR_UNSUPPORTED and the count in the message, by sdrpp_vfo_add and by sdrpp_vfo_set_channel_taps;
    a VFO with a 4 096-tap channel filter plans what it planned before the bound moved: the same forms, the same roles, the same job tables (byte count)."""
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=4800)
    d, keep = cw_desc(SR1, BW, F1)
    vid = ctx.vfo_add(d, keep)
    long_taps = np.zeros(65537, np.float32)
    long_taps[0] = 1.0
    with pytest.raises(capi.SdrppError) as ei:
        ctx.vfo_set_channel_taps(vid, long_taps)
    assert ei.value.code == UNSUPPORTED and "65537" in str(ei.value), ei.value
    ctx.vfo_set_channel_taps(vid, long_taps[:65536])
    d2, keep2 = cw_desc(SR1, BW, F1)
    d2.chan_ntaps, d2.chan_taps = 65537, radio._fp(long_taps)
    with pytest.raises(capi.SdrppError) as ei:
        ctx.vfo_add(d2, keep2)
    assert ei.value.code == UNSUPPORTED and "65537" in str(ei.value), ei.value
    ctx.close()
    x = keyed(SR1, 2 * 4800, F1, 23).astype(np.complex64)
    t4096 = np.zeros(4096, np.float32)
    t4096[[0, 4095]] = 0.5
    res = []
    for pipelined in (False, True):
        ctx = capi.Context(0, max_push=4800)
        d3, keep3 = radio.vfo_desc(SR1, IF_RATE, BW, F1, "USB")
        d3.chan_ntaps, d3.chan_taps = 4096, radio._fp(t4096)
        ctx.vfo_add(d3, keep3)
        if pipelined:
            ctx.set_pipelined(True, 1)
        for b in range(2):
            ctx.push(x[b * 4800:(b + 1) * 4800])
        if pipelined:
            for t in (1, 2):
                ctx.result_wait(t)
                ctx.result_release(t)
        res.append((ctx.pass_form_stats(), ctx.pipeline_stats()))
        ctx.close()
    (forms, _), (_, st) = res
    print("\n[cw 4096 taps] %s forms %s | roles %s table bytes %d" % (backend, forms, st["roles"], st["table_bytes"]))
    assert (forms, sorted(st["roles"]), st["table_bytes"]) == PLAN_4096, (forms, sorted(st["roles"]), st["table_bytes"])


# what a USB VFO (48 kS/s -> 3 kS/s) with a 4 096-tap channel filter planned on the commit before this file, over two pushes of 4 800 samples
PLAN_4096 = ({"carry": 2, "toep_c": 2, "firb_c": 2, "pre": 2, "seq": 2, "s1_1": 2}, ["carry", "copy", "firb_c", "pre", "s1_1", "seq", "toep_c"], 928)


# ---- 5. plan 8192's first stage alone: /128, 726 taps, on the matrix cores ------------------------------------------------------------------------
SR8192 = 24.576e6
S128_N = 128 * (32 * 3 + 5 + 24)  # 125 outputs: three 32-output tiles and a ragged fourth (seven 16-output tiles and a ragged eighth)
S128_CUTS = [128 * 40 + 3, 1, 128 * 64]
S128_CUTS = S128_CUTS + [S128_N - sum(S128_CUTS)]


@pytest.mark.parametrize("nv", [2, 16, 17, 32])
def test_plan_8192_first_stage_on_the_matrix_cores(backend, nv):
    """Hand descriptors, RAW, one stage = the reference's fir_8192_128 (726 taps, /128), 2 / 16 / 17 / 32 VFOs (the 16-row and the 32-row tile, a job that is
    not full): the stage runs as fcl_0 — one tile engine per workgroup, two engines' planes do not fit — in the ordinary pass and as a tick role, never as
    s1d_*; windows straddle the history and the push ends; tick and pass bit for bit; every sample meets the per-sample bar."""
    from sdrplusplus_amd import radio

    stage = radio.plans().stages(8192)[0]
    assert stage[0] == 128 and len(stage[1]) == 726
    offs = _spread(nv, SR8192, 0.7)
    descs = []
    for f in offs:
        d, keep, rate = hand_desc(SR8192, f, [stage])
        descs.append((d, keep, _parts(d), f, None))
    x = _fm_mix(SR8192, S128_N, offs, 33, 0.08 * rate, amp=0.3 / nv ** 0.5)
    case = dict(sr=SR8192, n=S128_N, descs=descs, x=x)
    assert sum(S128_CUTS) == S128_N and min(S128_CUTS) >= 1
    if1, _, forms1, _ = _run(case, [S128_N], False)
    if2, _, forms2, _ = _run(case, S128_CUTS, False)
    if3, _, forms3, st3 = _run(case, S128_CUTS, True)
    print("\n[cw /128 nv %d] %s pass forms %s | ragged %s | tick roles %s" % (nv, backend, sorted(forms1), sorted(forms2), sorted(st3["roles"])))
    for f in (forms1, forms2, st3["roles"]):
        assert f.get("fcl_0", 0) > 0 and not [k for k in f if k.startswith("s1d")], f
    assert st3["pass_blocks"] == 0 and st3["tick_blocks"] == len(S128_CUTS) and not forms3, (st3, forms3)
    rid, wb, we = "s128_nv%d" % nv, 0.0, 0.0
    for i, (d, keep, p, off, _) in enumerate(descs):
        _bits_equal(if2[i].view(np.float32), if3[i].view(np.float32), "vfo %d: tick vs pass" % i)
        r_if, _ = restate64(p, x)
        b_if, _ = baseline32_hand(p, x, SR8192, off)
        assert len(r_if) == S128_N // 128
        for what, g in (("one push", if1[i]), ("ragged", if2[i])):
            b, e = _per_sample(rid, "vfo %d %s" % (i, what), g, b_if, r_if, 0)
            wb, we = max(wb, b), max(we, e)
        assert np.max(np.abs(if1[i] - if2[i])) < 2e-7 * max(1.0, rms(r_if) / 0.05), i  # (test_push_size_invariance: only the NCO's phase origin moves)
    print("[cw /128 nv %d] %s per-sample max-abs / rms: baseline %.3g library %.3g (bar %.3g)" % (nv, backend, wb, we, MARGIN * wb))


# ---- 6. plan 8192 whole ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,nco_mode", [(3, 2), (20, 2), (3, 1)], ids=["nv3-rotator", "nv20-rotator", "nv3-closed_form"])
def test_plan_8192_whole(backend, nv, nco_mode):
    """24.576 MS/s -> 3 kS/s is exactly /8192 (stages /128, /8, /4, /2, no resampler): 3 and 20 CW VFOs over 2^21 samples (256 IF samples) in the
    reference's sr / 200 blocks, reference rotator, audio within 1e-5 of the yardstick — and 3 VFOs once more with the closed-form NCO against the ideal-NCO
    yardstick, where the /128 stage is the matrix front end (fcl_0)."""
    from sdrplusplus_amd import capi

    n, ref_block = 1 << 21, int(SR8192 / 200)
    offs = _spread(nv, SR8192, 0.7)
    x = np.zeros(n, np.complex128)
    for k, f in enumerate(offs):
        x += keyed(SR8192, n, f, 50 + k, amp=0.3 / nv ** 0.5, noise=0.002 / nv ** 0.5, dot=0.012)
    x = x.astype(np.complex64)
    ctx = capi.Context(0, max_push=n)
    ctx.set_reference_block(ref_block)
    vids = []
    for f in offs:
        d, keep = cw_desc(SR8192, BW, f, nco_mode)
        assert [d.stage_decim[i] for i in range(d.n_stages)] == [128, 8, 4, 2] and d.stage_ntaps[0] == 726 and d.interp == d.decim
        vids.append(ctx.vfo_add(d, keep))
    ctx.push(x)
    got = [ctx.vfo_read(v).copy() for v in vids]
    forms = ctx.pass_form_stats()
    ctx.close()
    if nco_mode == 1:
        assert forms.get("fcl_0", 0) > 0 and not [k for k in forms if k.startswith("s1d")], forms
    worst = 0.0
    for f, ga in zip(offs, got):
        y = Yard(SR8192, BW, f, ideal=(nco_mode == 1))
        _, wa = y.push(x, ref_block)
        y.close()
        assert len(ga) == 256 and rms(wa) > 0.05
        worst = max(worst, audio_err(ga, wa))
    print("\n[cw plan 8192] %s nv %d nco %d: worst audio %.3g forms %s" % (backend, nv, nco_mode, worst, sorted(forms)))
    assert worst < 1e-5, worst


# ---- 7. the AF chain goes UP: 3 000 -> 48 000 -------------------------------------------------------------------------------------------------
AF_BASELINE = (1.93e-06, 1.93e-06)  # (emulator leg, device leg), as test_af_chain.BASELINES


def test_af_chain_3000_to_48000(backend):
    """RationalResampler<stereo_t>(3 000 -> 48 000) behind a CW VFO: interp 16, decim 1, 1 216 taps, no pre-decimation — the one AF rate of the radio that
    interpolates by more than the matrix form's 15 phases.  test_af_chain's yardstick and runs: every output frame against the float64 restatement of the chain fed the
    device's own demodulator output; one push, ragged, pipelined, launch groups of 3."""
    from sdrplusplus_amd import radio

    row = AF.Row("USB", 48000, plan=((), 16, 1), form="vector", n=240 * 100)
    d, keep = cw_desc(SR1, BW, F1)
    a, akeep = radio.af_desc(IF_RATE, 48000.0, None, False)
    assert (a.n_stages, a.interp, a.decim, a.resamp_ntaps, a.hpf_ntaps, a.deemph_alpha) == (0, 16, 1, 1216, 0, 0.0)
    case = dict(sr=SR1, if_rate=IF_RATE, vfo=(d, keep), af=(a, akeep), parts=AF.af_parts(a), x=keyed(SR1, row.n, F1, 29).astype(np.complex64))
    cuts = AF.cuts_of(row.n, 16 * 15)
    dem1, af1, forms1, _, _ = AF.run(case, [row.n])
    dem2, af2, forms2, _, cnt2 = AF.run(case, cuts)
    _, af3, forms3, st3, cnt3 = AF.run(case, cuts, pipelined=True)
    _, af4, forms4, st4, cnt4 = AF.run(case, cuts, pipelined=True, group=3)
    assert len(af1) == 16 * len(dem1) == row.n and cnt2[1] == 0 and min(cnt2[3:5]) == 0 and cnt3 == cnt2 and cnt4 == cnt2, cnt2
    assert forms1.get("polyc", 0) > 0 and forms2.get("polyc", 0) > 0, (forms1, forms2)
    for st, forms in ((st3, forms3), (st4, forms4)):
        assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(cuts) and not forms and st["roles"].get("polyc", 0) > 0, (st, forms)
    base1, e1 = AF.per_sample(case, row, dem1, af1, "one push")
    base2, e2 = AF.per_sample(case, row, dem2, af2, "ragged")
    _bits_equal(af2, af3, "pipelined vs ordinary")
    _bits_equal(af2, af4, "grouped vs ordinary")
    base = max(base1, base2)
    print("\n[cw af 3000 -> 48000] %s per-sample max-abs / rms: baseline %.3g library %.3g (bar %.3g) | frames %d" % (backend, base, max(e1, e2), MARGIN * base, len(af1)))
    assert base <= 1.25 * AF_BASELINE[backend == "gpu"], ("the float32 sequential baseline moved up: the bar may not loosen unseen", base, AF_BASELINE)
