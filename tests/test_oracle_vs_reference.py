"""Pins the oracle (oracle/oracle.c) against the reference's own code compiled in the build container (oracle/_ref):
every comparison is BIT-EXACT.  Skipped where oracle/_ref was never built (no /root/reference and no prebuilt .so)."""
import ctypes as C

import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.skipif(not S.ref_available(), reason="oracle/_ref not built (needs /root/reference)")


def _noise(n, seed, scale=0.1):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * scale).astype(np.complex64)


@pytest.mark.parametrize("args", [(75000.0, 7500.0, 250000.0), (6250.0, 625.0, 50000.0), (15000.0, 4000.0, 250000.0), (1400.0, 140.0, 24000.0)])
def test_low_pass_taps_bit_exact(args):
    t = S.oracle_low_pass(*args)
    buf = np.zeros(len(t) + 8, np.float32)
    n = S.ref().ref_low_pass(*args, 0, S._fp(buf), len(buf))
    assert n == len(t) and np.array_equal(buf[:n], t)


def test_high_pass_and_windows_bit_exact():
    o, r = S.oracle(), S.ref()
    a = np.zeros(4096, np.float32)
    b = np.zeros(4096, np.float32)
    na = o.orc_high_pass(300.0, 100.0, 48000.0, 0, S._fp(a), 4096)
    nb = r.ref_high_pass(300.0, 100.0, 48000.0, 0, S._fp(b), 4096)
    assert na == nb and np.array_equal(a[:na], b[:nb])
    for n in (0.0, 1.0, 17.5, 4095.0):
        assert o.orc_nuttall(n, 4096.0) == r.ref_nuttall(n, 4096.0)
        assert o.orc_blackman(n, 4096.0) == r.ref_blackman(n, 4096.0)


CASES = [  # (input rate, mode, offset, block)
    (10e6, "WFM", 1.35e6, 50000),
    (2.4e6, "WFM", 300e3, 12000),
    (61.44e6, "NFM", -3.2e6, 307200),
    (61.44e6, "AM", 600e3, 307200),
    (61.44e6, "USB", 1.0014e6, 307200),
    (61.44e6, "LSB", -7.6786e6, 307200),
    (61.44e6, "DSB", 2.0e6, 307200),
]


@pytest.mark.parametrize("sr,mode,offset,block", CASES)
def test_rxvfo_and_demod_bit_exact(sr, mode, offset, block):
    from sdrplusplus_amd import radio

    if_rate, bw = radio.RADIO_DEFAULTS[mode]
    oc = S.OracleChain(sr, if_rate, bw, offset, S.MODES[mode])
    rc = S.RefChain(sr, if_rate, bw, offset, S.MODES[mode])
    x = _noise(block * 3, 42)
    t = np.arange(len(x)) / sr
    x = (x + 0.3 * (1 + 0.3 * np.cos(2 * np.pi * 1000 * t)) * np.exp(2j * np.pi * offset * t)).astype(np.complex64)
    for b in range(3):
        blk = x[b * block:(b + 1) * block]
        oi, oa = oc.process(blk)
        ri, ra = rc.process(blk)
        assert np.array_equal(oi, ri), "RxVFO::out differs in block %d" % b
        assert np.array_equal(oa, ra), "demodulator output differs in block %d" % b


def test_retune_mid_stream_bit_exact():
    oc = S.OracleChain(10e6, 250e3, 150e3, 1.0e6, None)
    rc = S.RefChain(10e6, 250e3, 150e3, 1.0e6, None)
    x = _noise(150000, 5)
    for b, off in enumerate((1.0e6, -2.2e6, 0.3e6)):
        oc.set_offset(off)
        rc.set_offset(off)
        oi, _ = oc.process(x[b * 50000:(b + 1) * 50000])
        ri, _ = rc.process(x[b * 50000:(b + 1) * 50000])
        assert np.array_equal(oi, ri)


def test_bandwidth_change_mid_stream_bit_exact():
    """RxVFO::setBandwidth (rx_vfo.h:60-70) between blocks: fewer taps, more taps, filter bypassed (bandwidth == out rate: the stale delay line
    stays) and back — FIR::setTaps keeps the delay line (fir.h:31-52).  Oracle restatement vs the compiled reference, bit for bit."""
    oc = S.OracleChain(10e6, 250e3, 150e3, 0.7e6, None)
    rc = S.RefChain(10e6, 250e3, 150e3, 0.7e6, None)
    x = _noise(5 * 50000, 6)
    for b, bw in enumerate((150e3, 200e3, 90e3, 250e3, 120e3)):
        if b:
            oc.set_bandwidth(bw)
            rc.set_bandwidth(bw)
        oi, _ = oc.process(x[b * 50000:(b + 1) * 50000])
        ri, _ = rc.process(x[b * 50000:(b + 1) * 50000])
        assert oi.shape == ri.shape and np.array_equal(oi, ri), "block %d (bandwidth %g)" % (b, bw)


def test_one_tap_filter_bypass_long_taps_bit_exact():
    """A bandwidth far above the IF rate makes taps::lowPass return ONE tap (windowed_sinc.h: 3.8 * rate / transition < 2); FIR::setTaps then leaves an
    empty delay line (fir.h:31-52).  Bypassed behind that and switched on again with long taps, the filter starts from ZEROS — not from what an earlier
    bypass left behind.  Oracle restatement vs the compiled reference, bit for bit."""
    oc = S.OracleChain(10e6, 250e3, 150e3, 0.7e6, None)
    rc = S.RefChain(10e6, 250e3, 150e3, 0.7e6, None)
    seq = (150e3, 250e3, 120e3, 10e6, 250e3, 150e3, 250e3, 10e6, 90e3)
    x = _noise(len(seq) * 50000, 16)
    for b, bw in enumerate(seq):
        if b:
            oc.set_bandwidth(bw)
            rc.set_bandwidth(bw)
        oi, _ = oc.process(x[b * 50000:(b + 1) * 50000])
        ri, _ = rc.process(x[b * 50000:(b + 1) * 50000])
        assert oi.shape == ri.shape and np.array_equal(oi, ri), "block %d (bandwidth %g)" % (b, bw)


def test_frontend_lines_bit_exact():
    """IQFrontEnd (threads, Splitter, Reshaper, handler — iq_frontend.cpp verbatim) vs the streaming restatement."""
    o, r = S.oracle(), S.ref()
    sr, N = 2.4e6, 4096
    skip, nz = C.c_int(), C.c_int()
    o.orc_gen_reshape_params(sr, N, 20.0, C.byref(skip), C.byref(nz))
    assert (nz.value, skip.value) == (4096, 115904)
    # The reference's Reshaper hands a frame on only after it has also consumed that frame's `skip` samples
    # (ring_buffer.h:66-110: read, then skip, then swap); the restatement publishes a line as soon as its nz samples
    # are in.  Same lines, `skip` samples earlier — so feed whole frame periods here.
    n = 12000 * 50
    x = (_noise(n, 9, 0.01) + 0.5 * np.exp(2j * np.pi * 0.125 * np.arange(n))).astype(np.complex64)
    w = S.oracle_fft_window(2, nz.value)
    sp = S.OracleSpectrum(N, nz.value, skip.value, w)
    ol = np.concatenate([sp.push(x[b * 12000:(b + 1) * 12000]) for b in range(50)])
    fe = r.ref_frontend_create(sr, N, 20.0, 2)
    got = r.ref_frontend_feed(fe, S._fp(x.view(np.float32)), n, 12000, len(ol), 10000)
    rl = np.empty((max(got, 1), N), np.float32)
    got = r.ref_frontend_lines(fe, S._fp(rl), got)
    r.ref_frontend_destroy(fe)
    assert got == len(ol) == 5
    assert np.array_equal(rl[:got], ol)


def test_af_resampler_and_deemphasis_bit_exact():
    """'next' row: RationalResampler 250k -> 48k and Deemphasis (radio_module.h:102-110)."""
    o, r = S.oracle(), S.ref()
    x = _noise(25000, 3)
    oh = o.orc_resampler_create(S.plans_handle(), 250000.0, 48000.0, 2)
    rh = r.ref_resampler_create(250000.0, 48000.0)
    info = [C.c_int() for _ in range(6)]
    o.orc_resampler_info(oh, *[C.byref(v) for v in info])
    assert [v.value for v in info][1:5] == [4, 96, 125, 9500]  # predec 4, 96/125, 9500 taps
    for b in range(2):
        blk = np.ascontiguousarray(x[b * 12500:(b + 1) * 12500])
        oo = np.empty(len(blk) + 64, np.complex64)
        ro = np.empty(len(blk) + 64, np.complex64)
        no = o.orc_resampler_process(oh, len(blk), S._fp(blk.view(np.float32)), S._fp(oo.view(np.float32)))
        nr = r.ref_resampler_process(rh, len(blk), S._fp(blk.view(np.float32)), S._fp(ro.view(np.float32)))
        assert no == nr and np.array_equal(oo[:no], ro[:nr])
    o.orc_resampler_destroy(oh)
    r.ref_resampler_destroy(rh)
    od, rd = o.orc_deemp_create(50e-6, 48000.0), r.ref_deemp_create(50e-6, 48000.0)
    a = np.ascontiguousarray(x[:4800].view(np.float32).reshape(-1, 2))
    oa, ra = np.empty_like(a), np.empty_like(a)
    o.orc_deemp_process(od, len(a), S._fp(a), S._fp(oa))
    r.ref_deemp_process(rd, len(a), S._fp(a), S._fp(ra))
    assert np.array_equal(oa, ra)
    o.orc_deemp_destroy(od)
    r.ref_deemp_destroy(rd)


# every (AF input rate, audio rate) pair tests/test_af_chain.py takes the oracle's AF chain to: (mode, pre-decimation, L, M) as RationalResampler::reconfigure settles them
AF_RATE_PAIRS = [
    (24000.0, 24000.0, 3, 1, 1, 1), (24000.0, 12000.0, 1, 2, 1, 1), (24000.0, 48000.0, 2, 1, 2, 1), (24000.0, 96000.0, 2, 1, 4, 1), (24000.0, 192000.0, 2, 1, 8, 1),
    (24000.0, 16000.0, 2, 1, 2, 3), (15000.0, 24000.0, 2, 1, 8, 5), (15000.0, 12000.0, 2, 1, 4, 5), (15000.0, 8000.0, 2, 1, 8, 15), (15000.0, 48000.0, 2, 1, 16, 5),
    (15000.0, 44100.0, 2, 1, 147, 50), (15000.0, 176400.0, 2, 1, 294, 25), (50000.0, 50000.0, 3, 1, 1, 1), (50000.0, 44100.0, 2, 1, 441, 500),
    (50000.0, 192000.0, 2, 1, 96, 25), (50000.0, 11025.0, 0, 4, 441, 500), (50000.0, 96000.0, 2, 1, 48, 25), (50000.0, 176400.0, 2, 1, 441, 125),
    (250000.0, 44100.0, 0, 4, 441, 625), (250000.0, 8000.0, 0, 16, 64, 125), (250000.0, 50000.0, 0, 4, 4, 5), (250000.0, 96000.0, 0, 2, 96, 125),
    (250000.0, 192000.0, 2, 1, 96, 125),
]


@pytest.mark.parametrize("in_sr,out_sr,mode,predec,interp,decim", AF_RATE_PAIRS, ids=["%d_%d" % (a, b) for a, b, *_ in AF_RATE_PAIRS])
def test_af_resampler_every_rate_pair_bit_exact(in_sr, out_sr, mode, predec, interp, decim):
    """RationalResampler at every AF rate pair of tests/test_af_chain.py, two uneven blocks: the plan figures (mode, pre-decimation, L / M, prototype taps, taps per
    phase) and every output sample, oracle restatement against the compiled reference."""
    o, r = S.oracle(), S.ref()
    if not hasattr(r, "ref_resampler_info"):
        pytest.skip("oracle/_ref was built before ref_resampler_info existed (rebuild it where /root/reference is)")
    x = _noise(6007, 31)
    oh = o.orc_resampler_create(S.plans_handle(), in_sr, out_sr, 2)
    rh = r.ref_resampler_create(in_sr, out_sr)
    oi, ri = [C.c_int() for _ in range(6)], [C.c_int() for _ in range(6)]
    o.orc_resampler_info(oh, *[C.byref(v) for v in oi])
    r.ref_resampler_info(rh, *[C.byref(v) for v in ri])
    oi, ri = [v.value for v in oi], [v.value for v in ri]
    assert oi[0] == ri[0] == mode, (oi, ri)
    if mode in (0, 1):
        assert oi[1] == ri[1] == predec, (oi, ri)
    if mode in (0, 2):
        assert oi[2:4] == ri[2:4] == [interp, decim] and oi[4:] == ri[4:] and oi[4] > 0, (oi, ri)
    grow = int(np.ceil(max(1.0, out_sr / in_sr)))
    for blk in (x[:2503], x[2503:]):
        blk = np.ascontiguousarray(blk)
        oo = np.empty(len(blk) * grow + 64, np.complex64)
        ro = np.empty(len(blk) * grow + 64, np.complex64)
        no = o.orc_resampler_process(oh, len(blk), S._fp(blk.view(np.float32)), S._fp(oo.view(np.float32)))
        nr = r.ref_resampler_process(rh, len(blk), S._fp(blk.view(np.float32)), S._fp(ro.view(np.float32)))
        assert no == nr > 0 and np.array_equal(oo[:no].view(np.uint32), ro[:nr].view(np.uint32))
    o.orc_resampler_destroy(oh)
    r.ref_resampler_destroy(rh)


@pytest.mark.parametrize("rate,ntaps", [(44100.0, 1675), (96000.0, 3648), (176400.0, 6703), (192000.0, 7296)])
def test_af_high_pass_taps_every_rate_bit_exact(rate, ntaps):
    """highPass(300, 100, audio rate) (radio_module.h:597) where the AF rows take it: tap count and taps."""
    o, r = S.oracle(), S.ref()
    a, b = np.zeros(8192, np.float32), np.zeros(8192, np.float32)
    na = o.orc_high_pass(300.0, 100.0, rate, 0, S._fp(a), len(a))
    nb = r.ref_high_pass(300.0, 100.0, rate, 0, S._fp(b), len(b))
    assert na == nb == ntaps and np.array_equal(a[:na].view(np.uint32), b[:nb].view(np.uint32))


@pytest.mark.parametrize("tau,rate", [(22e-6, 48000.0), (75e-6, 48000.0), (22e-6, 192000.0), (75e-6, 44100.0), (50e-6, 44100.0), (50e-6, 192000.0), (75e-6, 50000.0), (50e-6, 50000.0), (22e-6, 96000.0)])
def test_af_deemphasis_every_setting_bit_exact(tau, rate):
    """Deemphasis (filter/deephasis.h) at the 22 us and 75 us modes, at 44 100 and 192 000 Hz and at every other setting tests/test_af_chain.py uses, over two blocks (the state carries)."""
    o, r = S.oracle(), S.ref()
    a = np.ascontiguousarray(_noise(4800, 3).view(np.float32).reshape(-1, 2))
    od, rd = o.orc_deemp_create(tau, rate), r.ref_deemp_create(tau, rate)
    for blk in (a[:1777], a[1777:]):
        blk = np.ascontiguousarray(blk)
        oa, ra = np.empty_like(blk), np.empty_like(blk)
        o.orc_deemp_process(od, len(blk), S._fp(blk), S._fp(oa))
        r.ref_deemp_process(rd, len(blk), S._fp(blk), S._fp(ra))
        assert np.array_equal(oa.view(np.uint32), ra.view(np.uint32))
    o.orc_deemp_destroy(od)
    r.ref_deemp_destroy(rd)


@pytest.mark.parametrize("ratio,dc,conj", [(1, True, False), (2, True, True), (8, False, True), (64, True, False)])
def test_preproc_chain_bit_exact(ratio, dc, conj):
    """'next' row 2: IQFrontEnd's pre-processing chain (iq_frontend.cpp:32-39) = PowerDecimator<complex_t> -> DCBlocker<complex_t>
    -> Conjugate, restated in oracle.c, against the reference classes block by block (uneven blocks exercise the stage offsets)."""
    o, r = S.oracle(), S.ref()
    x = (_noise(60000, 9) + np.complex64(0.25 - 0.125j)).astype(np.complex64)
    rate = 50.0 / (2.4e6 / ratio)  # genDCBlockRate(effectiveSr), iq_frontend.h:55-57
    oh = o.orc_preproc_create(S.plans_handle(), ratio, int(dc), rate, int(conj))
    rh = r.ref_preproc_create(ratio, int(dc), rate, int(conj))
    pos = 0
    for n in (12000, 7, 20001, 27992):
        blk = np.ascontiguousarray(x[pos:pos + n])
        pos += n
        oo = np.empty(n + 8, np.complex64)
        ro = np.empty(n + 8, np.complex64)
        no = o.orc_preproc_process(oh, n, S._fp(blk.view(np.float32)), S._fp(oo.view(np.float32)))
        nr = r.ref_preproc_process(rh, n, S._fp(blk.view(np.float32)), S._fp(ro.view(np.float32)))
        assert no == nr and np.array_equal(oo[:no].view(np.uint32), ro[:nr].view(np.uint32))
    o.orc_preproc_destroy(oh)
    r.ref_preproc_destroy(rh)


@pytest.mark.parametrize("pcm", [0, 1, 2])
def test_sample_stream_compressor_bit_exact(pcm):
    """'next' row 4: the SDR++-server frame (SampleStreamCompressor::process, sample_stream_compressor.h:30-62) restated in oracle.c
    against the reference's own static function."""
    o, r = S.oracle(), S.ref()
    for seed, n in ((1, 1000), (2, 7), (3, 4096)):
        x = np.ascontiguousarray(_noise(n, seed, 0.3))
        a = np.zeros(8 + n * 8 + 16, np.uint8)
        b = np.zeros_like(a)
        u8 = C.POINTER(C.c_uint8)
        na = o.orc_compress(n, pcm, S._fp(x.view(np.float32)), a.ctypes.data_as(u8))
        nb = r.ref_compress(n, pcm, S._fp(x.view(np.float32)), b.ctypes.data_as(u8))
        assert na == nb and np.array_equal(a[:na], b[:nb])


# ---- waterfall widget arithmetic: oracle.c's restatement vs the reference's own functions, cut out of gui/widgets/waterfall.cpp at build
#      time (oracle/Makefile: _ref/waterfall_extract.inc + oracle/ref_waterfall.cpp) ----
def _refwf():
    import os
    path = os.path.join(S.ORACLE_DIR, "_ref", "libsdrpp_refwf.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref/libsdrpp_refwf.so not built")
    L = C.CDLL(path)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.ref_do_zoom.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, fp]
    L.ref_wf_create.restype = C.c_void_p
    L.ref_wf_create.argtypes = [C.c_int, C.c_int, C.c_int]
    L.ref_wf_destroy.argtypes = [C.c_void_p]
    L.ref_wf_set_view.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float]
    L.ref_wf_set_smoothing.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.ref_wf_set_hold.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.ref_wf_push.argtypes = [C.c_void_p, fp, ip]
    L.ref_wf_latest.argtypes = [C.c_void_p, fp, fp]
    L.ref_wf_signal_info.argtypes = [C.c_void_p, C.c_double, C.c_double, fp, fp]
    L.ref_wf_raster.argtypes = [C.c_void_p, ip]
    return L


@pytest.mark.parametrize("case", [(0, 65536, 65536, 1024), (1000, 30000, 65536, 600), (4000, 90, 4096, 600), (-5, 4096, 4096, 333), (60000, 9000, 65536, 1920),
                                  (0, 1 << 20, 1 << 20, 1024)])
def test_do_zoom_bit_exact(case):
    """doZoom (waterfall.cpp:65-90) incl. its quirks: float running index, ceil window, clip at the end of the line, offset < 0 -> 0,
    width clamp 524288, bins repeated when zoomed past one bin per pixel."""
    offset, width, n_in, n_out = case
    L = _refwf()
    r = np.random.default_rng(n_in + n_out)
    line = (r.standard_normal(n_in) * 20.0 - 80.0).astype(np.float32)
    a = S.oracle_do_zoom(offset, width, n_out, line)
    b = np.empty(n_out, np.float32)
    L.ref_do_zoom(offset, width, n_in, n_out, S._fp(line), S._fp(b))
    assert np.array_equal(a, b)


def test_waterfall_push_trace_raster_signal_info_bit_exact():
    """WaterFall::getFFTBuffer / pushFFT (ring order, zoom, palette index, smoothing as three separately rounded VOLK passes, hold from
    index 1), updateWaterfallFb (full re-raster, opaque rows), calculateVFOSignalInfo and the smoothing / hold setters: the oracle's
    restatement (oracle.c section 7) against the reference's own function bodies, bit for bit, over a wrapping ring and view changes."""
    from test_parity_fft import _OracleWf
    from sdrplusplus_amd import capi

    L = _refwf()
    sr, N, W, H = 10e6, 4096, 600, 5
    r = np.random.default_rng(5)
    owf = _OracleWf(H, N, W)
    h = L.ref_wf_create(H, N, W)
    view = (1.0e6, 4.0e6)
    wmin, wmax = -110.0, -10.0
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert owf.signal_info(0.5e6, 200e3, sr) is None
    sa, sb = C.c_float(), C.c_float()
    assert L.ref_wf_signal_info(h, 0.5e6, 200e3, C.byref(sa), C.byref(sb)) == 0
    for step in range(13):
        if step == 4:
            owf.o.orc_wf_set_smoothing(owf.h, 1, 0.25)
            L.ref_wf_set_smoothing(h, 1, 0.25)
        if step == 6:
            owf.o.orc_wf_set_hold(owf.h, 1, 1.5)
            L.ref_wf_set_hold(h, 1, 1.5)
        if step == 9:
            view, wmin, wmax = (-2.0e6, 1.5e6), -90.0, -20.0
        if step == 11:
            owf.o.orc_wf_set_smoothing(owf.h, 0, 0.25)
            L.ref_wf_set_smoothing(h, 0, 0.25)
        start, size = capi.design_waterfall_view(view[0], view[1], sr, N)
        L.ref_wf_set_view(h, view[0], view[1], sr, wmin, wmax)
        line = (r.standard_normal(N) * 15.0 - 70.0 + 30.0 * np.exp(-((np.arange(N) - 2300.0) / 40.0) ** 2)).astype(np.float32)
        oi = owf.push(line, start, size, wmin, wmax)
        ri = np.empty(W, np.int32)
        L.ref_wf_push(h, line.ctypes.data_as(fp), ri.ctypes.data_as(ip))
        assert np.array_equal(oi, ri), step
        ol, oh = owf.latest()
        rl, rh = np.empty(W, np.float32), np.empty(W, np.float32)
        L.ref_wf_latest(h, rl.ctypes.data_as(fp), rh.ctypes.data_as(fp))
        assert np.array_equal(ol, rl), step
        if step >= 6:
            assert np.array_equal(oh[1:], rh[1:]), step  # index 0 is never touched by the hold loop (starts at 1) on either side
        for centre, bw in ((0.55e6, 200e3), (-4.9e6, 300e3), (4.99e6, 50e3)):
            assert L.ref_wf_signal_info(h, centre, bw, C.byref(sa), C.byref(sb)) == 1
            os_, on_ = owf.signal_info(centre, bw, sr)
            if centre > 4.9e6:
                continue  # the reference reads fftLine[rawFFTSize] (one past the line) for a VFO touching the upper edge: not comparable
            assert (os_, on_) == (sa.value, sb.value), (step, centre)
        ofb, on = owf.raster(start, size, wmin, wmax)
        rfb = np.empty((H, W), np.int32)
        rn = L.ref_wf_raster(h, rfb.ctypes.data_as(ip))
        assert on == rn == min(step + 1, H)
        assert np.array_equal(ofb[:on], rfb[:rn]) and np.all(rfb[rn:] == -1), step
    L.ref_wf_destroy(h)
