"""Host-side parameterisation of one VFO: what RxVFO::init (core/src/dsp/channel/rx_vfo.h:19-36), RationalResampler::
reconfigure (dsp/multirate/rational_resampler.h:120-165), PowerDecimator::reconfigure (power_decimator.h:93-111) and
the radio module's demodulators (decoder_modules/radio/src/demodulators/*.h) compute before any sample flows.
All double-precision design maths is done by the library's sdrpp_design_* functions (C++, libm) so that the constants
are bit-identical to the reference's; this module only wires them into a `sdrpp_vfo_desc`."""
import math
import os
import struct

import numpy as np

from . import capi

PLANS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "decim_plans.bin")

# radio-module defaults: (IF sample rate, default bandwidth) — wfm.h:268-270, nfm.h:56-58, am.h:76-78, usb.h:70-72, lsb.h, dsb.h, cw.h:82-84
RADIO_DEFAULTS = {
    "WFM": (250000.0, 150000.0),
    "NFM": (50000.0, 12500.0),
    "AM": (15000.0, 10000.0),
    "USB": (24000.0, 2800.0),
    "LSB": (24000.0, 2800.0),
    "DSB": (24000.0, 4600.0),
    "CW": (3000.0, 200.0),
}
DEMOD_CODES = {"RAW": capi.DEMOD_RAW, "WFM": capi.DEMOD_WFM, "NFM": capi.DEMOD_NFM, "AM": capi.DEMOD_AM,
               "USB": capi.DEMOD_USB, "LSB": capi.DEMOD_LSB, "DSB": capi.DEMOD_DSB, "CW": capi.DEMOD_CW}
CW_AGC_DEFAULTS = (100.0, 5.0)  # demodulators/cw.h:105-106 (SSB's and AM's are 50 / 5)


class DecimPlans:
    """The reference's power-of-two decimation plans (numbers extracted by tools/extract_decim_plans.cpp)."""

    def __init__(self, path=PLANS_PATH):
        with open(path, "rb") as f:
            blob = f.read()
        assert blob[:4] == b"SDPL", "bad plan file"
        ver, n = struct.unpack_from("<II", blob, 4)
        assert ver == 1
        off = 12
        self.plans = {}
        for _ in range(n):
            ratio, ns = struct.unpack_from("<II", blob, off)
            off += 8
            stages = []
            for _ in range(ns):
                d, nt = struct.unpack_from("<II", blob, off)
                off += 8
                taps = np.frombuffer(blob, dtype="<f4", count=nt, offset=off).copy()
                off += 4 * nt
                stages.append((d, taps))
            self.plans[ratio] = stages
        self.max_ratio = 1 << n  # power_decimator.h:29-31

    def stages(self, ratio):
        return [] if ratio == 1 else self.plans[ratio]


_plans = None


def plans():
    global _plans
    if _plans is None:
        _plans = DecimPlans()
    return _plans


def hz_to_rads(freq, samplerate):
    return 2.0 * math.pi * (freq / samplerate)  # dsp/math/hz_to_rads.h:6-8


def _fp(a):
    return a.ctypes.data_as(capi.c_float_p)


def meter_table(vfos):
    """The table of signal meters (Context.wf_set_meters) for a list of VFOs given as (offset, bandwidth) pairs in the units and sign vfo_desc
    takes them in: one band per VFO, in order — the band the waterfall measures for that VFO (calculateVFOSignalInfo, waterfall.cpp:558-598:
    centre = the VFO's offset, width = its bandwidth)."""
    return [(float(offset), float(bandwidth)) for offset, bandwidth in vfos]


def vfo_desc(in_sr, out_sr, bandwidth, offset, mode="RAW", low_pass=True, agc_attack=None, agc_decay=None, carrier_agc=False, nco_mode=0, tone=800.0):
    """Build a sdrpp_vfo_desc for RxVFO(in_sr -> out_sr, bandwidth, offset) followed by radio demodulator `mode`.
    agc_attack / agc_decay None: the mode's own defaults (50 / 5; CW 100 / 5).  tone: CW's beat note in Hz (demodulators/cw.h:107).
    Returns (desc, keepalive) — keepalive holds the numpy arrays the descriptor points into (sdrpp_vfo_add copies them)."""
    if agc_attack is None:
        agc_attack = CW_AGC_DEFAULTS[0] if mode == "CW" else 50.0
    if agc_decay is None:
        agc_decay = CW_AGC_DEFAULTS[1] if mode == "CW" else 5.0
    d = capi.VfoDesc()
    d.nco_mode = int(nco_mode)  # 0: the context's NCO mode, 1: closed form, 2: the reference's float rotator recursion (this VFO only)
    keep = []
    # FrequencyXlator: xlator.init(NULL, -_offset, _inSamplerate) (rx_vfo.h:27)
    d.phase_delta_re, d.phase_delta_im = capi.design_phase_delta(-offset, in_sr)
    # RationalResampler
    rs = capi.design_resampler(in_sr, out_sr, plans().max_ratio)
    stages = plans().stages(rs["predec"]) if rs["mode"] in (0, 1) else []
    d.n_stages = len(stages)
    for i, (dec, taps) in enumerate(stages):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        keep.append(t)
        d.stage_decim[i] = dec
        d.stage_ntaps[i] = len(t)
        d.stage_taps[i] = _fp(t)
    if rs["mode"] in (0, 2):
        rt = np.ascontiguousarray(rs["taps"], dtype=np.float32)
        keep.append(rt)
        d.interp, d.decim = rs["interp"], rs["decim"]
        d.resamp_ntaps = len(rt)
        d.resamp_taps = _fp(rt)
    else:
        d.interp, d.decim = 1, 1
        d.resamp_ntaps = 0
    # channel filter: generateTaps (rx_vfo.h:117-121), used when bandwidth != out rate (rx_vfo.h:24)
    if bandwidth != out_sr:
        fw = bandwidth / 2.0
        ct = capi.design_low_pass(fw, fw * 0.1, out_sr)
        keep.append(ct)
        d.chan_ntaps = len(ct)
        d.chan_taps = _fp(ct)
    else:
        d.chan_ntaps = 0
    # demodulator
    d.demod = DEMOD_CODES[mode]
    d.agc_set_point, d.agc_max_gain, d.agc_max_output_amp, d.agc_init_gain = 1.0, 10e6, 10.0, float("inf")  # am.h:30-31, ssb.h:27
    d.agc_attack = np.float32(agc_attack / out_sr)
    d.agc_decay = np.float32(agc_decay / out_sr)
    d.am_carrier_agc = int(carrier_agc)
    d.dc_block_rate = np.float32(100.0 / out_sr)  # radio am.h:34
    d.inv_deviation = 0.0
    d.audio_ntaps = 0
    d.ssb_phase_delta_re, d.ssb_phase_delta_im = 1.0, 0.0
    if mode == "WFM":
        d.inv_deviation = np.float32(1.0 / hz_to_rads(bandwidth / 2.0, out_sr))  # wfm.h:78, quadrature.h:19-26
        if low_pass:
            at = capi.design_low_pass(15000.0, 4000.0, out_sr)  # broadcast_fm.h:49
            keep.append(at)
            d.audio_ntaps = len(at)
            d.audio_taps = _fp(at)
    elif mode == "NFM":
        d.inv_deviation = np.float32(1.0 / hz_to_rads(bandwidth / 2.0, out_sr))  # fm.h:32
        if low_pass:
            at = capi.design_low_pass(bandwidth / 2.0, (bandwidth / 2.0) * 0.1, out_sr)  # fm.h:156
            keep.append(at)
            d.audio_ntaps = len(at)
            d.audio_taps = _fp(at)
    elif mode == "AM":
        at = capi.design_low_pass(bandwidth / 2.0, (bandwidth / 2.0) * 0.1, out_sr)  # demod/am.h:33
        keep.append(at)
        d.audio_ntaps = len(at)
        d.audio_taps = _fp(at)
    elif mode in ("USB", "LSB", "DSB"):
        tr = {"USB": bandwidth / 2.0, "LSB": -bandwidth / 2.0, "DSB": 0.0}[mode]  # ssb.h:106-117
        d.ssb_phase_delta_re, d.ssb_phase_delta_im = capi.design_phase_delta(tr, out_sr)
    elif mode == "CW":  # dsp/demod/cw.h:20: xlator.init(NULL, tone, samplerate) — the bandwidth plays no part (demodulators/cw.h:73)
        d.ssb_phase_delta_re, d.ssb_phase_delta_im = capi.design_phase_delta(tone, out_sr)
    return d, keep


def describe(desc):
    """Plan summary (used by tests to compare against the oracle / reference printout)."""
    predec = 1
    for i in range(desc.n_stages):
        predec *= desc.stage_decim[i]
    return dict(predec=predec, interp=desc.interp, decim=desc.decim, rtaps=desc.resamp_ntaps, chan_taps=desc.chan_ntaps,
                audio_taps=desc.audio_ntaps, stages=[(desc.stage_decim[i], desc.stage_ntaps[i]) for i in range(desc.n_stages)])


def af_desc(af_rate, audio_rate=48000.0, deemp_tau=50e-6, high_pass=False):
    """sdrpp_af_desc for the radio module's AF chain (radio_module.h:98-110): RationalResampler<stereo_t>(af_rate -> audio_rate),
    optional highPass(300, 100, audio_rate) FIR, optional Deemphasis(tau, audio_rate) (tau None/0 = off).
    Returns (desc, keepalive)."""
    a = capi.AfDesc()
    keep = []
    rs = capi.design_resampler(af_rate, audio_rate, plans().max_ratio)
    stages = plans().stages(rs["predec"]) if rs["mode"] in (0, 1) else []
    a.n_stages = len(stages)
    for i, (dec, taps) in enumerate(stages):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        keep.append(t)
        a.stage_decim[i] = dec
        a.stage_ntaps[i] = len(t)
        a.stage_taps[i] = _fp(t)
    if rs["mode"] in (0, 2):
        rt = np.ascontiguousarray(rs["taps"], dtype=np.float32)
        keep.append(rt)
        a.interp, a.decim = rs["interp"], rs["decim"]
        a.resamp_ntaps = len(rt)
        a.resamp_taps = _fp(rt)
    else:
        a.interp, a.decim, a.resamp_ntaps = 1, 1, 0
    if high_pass:
        ht = capi.design_high_pass(300.0, 100.0, audio_rate)
        keep.append(ht)
        a.hpf_ntaps = len(ht)
        a.hpf_taps = _fp(ht)
    a.deemph_alpha = capi.design_deemphasis_alpha(deemp_tau, audio_rate) if deemp_tau else 0.0
    return a, keep


def rds_desc(if_rate=250e3, out_rate=5000.0, offset=-57000.0):
    """sdrpp_rds_desc for the WFM demodulator's RDS branch (broadcast_fm.h:60-62): FrequencyXlator(offset, if_rate) and
    RationalResampler<complex_t>(if_rate -> out_rate) — at 250 kS/s the ratio-32 plan {8 x 44, 2 x 12, 2 x 69} and the 5000 / 7813 polyphase stage.
    Returns (desc, keepalive)."""
    r = capi.RdsDesc()
    keep = []
    r.phase_delta_re, r.phase_delta_im = capi.design_phase_delta(offset, if_rate)
    rs = capi.design_resampler(if_rate, out_rate, plans().max_ratio)
    stages = plans().stages(rs["predec"]) if rs["mode"] in (0, 1) else []
    r.n_stages = len(stages)
    for i, (dec, taps) in enumerate(stages):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        keep.append(t)
        r.stage_decim[i] = dec
        r.stage_ntaps[i] = len(t)
        r.stage_taps[i] = _fp(t)
    if rs["mode"] in (0, 2):
        rt = np.ascontiguousarray(rs["taps"], dtype=np.float32)
        keep.append(rt)
        r.interp, r.decim = rs["interp"], rs["decim"]
        r.resamp_ntaps = len(rt)
        r.resamp_taps = _fp(rt)
    else:
        r.interp, r.decim, r.resamp_ntaps = 1, 1, 0
    return r, keep


def stereo_desc(if_rate=250e3, enabled=True):
    """sdrpp_stereo_desc for the WFM demodulator's stereo branch as BroadcastFM::init sets it up (broadcast_fm.h:43-48): the complex pilot band-pass
    bandPass<complex_t>(18750, 19250, 3000, if_rate, odd), PLL(25000 / if_rate, phase 0, 19 kHz, limits 18.75 / 19.25 kHz), delay (taps - 1) / 2 + 1.
    Returns (desc, keepalive)."""
    s = capi.StereoDesc()
    taps = np.ascontiguousarray(capi.design_band_pass_complex(18750.0, 19250.0, 3000.0, if_rate, True))
    s.pilot_taps = _fp(taps.view(np.float32))
    s.pilot_ntaps = len(taps)
    s.delay = (len(taps) - 1) // 2 + 1
    s.alpha, s.beta = capi.design_pll(25000.0 / if_rate)
    s.init_freq = np.float32(hz_to_rads(19000.0, if_rate))
    s.min_freq = np.float32(hz_to_rads(18750.0, if_rate))
    s.max_freq = np.float32(hz_to_rads(19250.0, if_rate))
    s.enabled = int(bool(enabled))
    return s, [taps]


def pager_desc(if_rate=24000.0, baud=2400.0):
    """sdrpp_sym_desc for the pager decoder's POCSAGDSP::init(in, if_rate, baud) (pocsag/dsp.h:20-37): Quadrature(-4500 Hz), ten shaping taps of 0.1f,
    MM<float>(if_rate / baud, omega gain 1e-4, mu gain 1.0, relative limit 0.05) with its 128 x 8 interpolator.  Returns (desc, keepalive)."""
    s = capi.design_pager(if_rate, baud)
    taps = np.full(10, np.float32(0.1), dtype=np.float32)
    bank = capi.design_mm_interp(s.interp_phases, s.interp_ntaps)
    s.shape_taps = _fp(taps)
    s.interp_bank = _fp(bank)
    return s, [taps, bank]


def rds_demod_desc(rate=5000.0, source=0):
    """sdrpp_rdsd_desc for the radio module's RDSDemod::init (radio/src/rds_demod.h:19-41) on a stream of `rate` samples per second: FastAGC(1, 1e6, 0.1),
    Costas<2>(0.005), the 190-tap complex band-pass 0 .. 2375 Hz, Costas<2>(0.01) at 1187.5 Hz +- 10 %, MM<float>(rate / 1187.5, 1e-6, 0.01, 0.01).
    source 0: behind the VFO's RDS branch; 1: the stream a demodulator would read (RAW VFOs).  Returns (desc, keepalive)."""
    d, taps, bank = capi.design_rds_demod(rate)
    d.source = int(source)
    return d, [taps, bank]


def meteor_desc(symbolrate=72000.0, samplerate=150000.0, rrc_taps=33, rrc_beta=capi._F32(0.6), agc_rate=capi._F32(0.1), costas_bw=capi._F32(0.005), broken=False, oqpsk=False,
                omega_gain=1e-6, mu_gain=0.01):
    """sdrpp_qpsk_desc for the meteor_demodulator module's dsp::demod::Meteor::init (meteor_demod.h:24-43): rootRaisedCosine(rrc_taps, rrc_beta), FastAGC(1, 10e6,
    agc_rate), MeteorCostas(costas_bw), MM<complex_t>(samplerate / symbolrate, omega_gain, mu_gain, 0.01), int8 = value * 84.  The defaults are the module's
    (main.cpp:66).  For a RAW VFO whose output rate is `samplerate`.  Returns (desc, keepalive)."""
    d, taps, bank = capi.design_meteor(symbolrate, samplerate, rrc_taps, rrc_beta, agc_rate, costas_bw, broken, oqpsk, omega_gain, mu_gain)
    return d, [taps, bank]


def m17_desc(if_rate=14400.0):
    """The two descriptions of the M17 decoder's front (m17_decoder/src/m17dsp.h) at if_rate: sdrpp_sym_desc for its GFSK demodulator — Quadrature(2400 Hz), 31
    root-raised-cosine taps (alpha 0.5, 4800 baud), MM<float>(if_rate / 4800, omega gain 1e-6, mu gain 0.01, relative limit 0.01) with its 128 x 8 interpolator —
    and sdrpp_frame_desc for M17Slice4FSK / M17FrameDemux.  Returns (sym_desc, frame_desc, keepalive)."""
    sym, frame, taps, scr, il = capi.design_m17(if_rate)
    bank = capi.design_mm_interp(sym.interp_phases, sym.interp_ntaps)
    sym.interp_bank = _fp(bank)
    return sym, frame, [taps, bank, scr, il]


def if_desc(if_rate, nb=False, nb_level=10.0, squelch=None):
    """sdrpp_if_desc for the radio module's IF chain (radio_module.h:84-96): NoiseBlanker(rate = 500 / if_rate, level; :90, :526) ->
    PowerSquelch(level in dB; None = off).  FMIF, the chain's last block, is switched by Context.vfo_set_fmnr (IFNR_BINS); the CTCSS squelch is not on the device."""
    f = capi.IfDesc()
    f.nb_enabled = int(bool(nb))
    f.nb_rate = 500.0 / float(if_rate)
    f.nb_level = float(nb_level)
    f.squelch_enabled = int(squelch is not None)
    f.squelch_level = float(squelch) if squelch is not None else 0.0
    return f


# The radio module's "IF Noise Reduction" presets: FMIF's bin count (radio_module.h:31-36); WFM always runs 32 (radio_module.h:531)
IFNR_BINS = {"NOAA_APT": 9, "VOICE": 15, "NARROW_BAND": 31, "BROADCAST": 32}
