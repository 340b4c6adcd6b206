"""The per-VFO control surface of the C-ABI as a caller sees it: which error an unknown id or a missing chain gives (code and message), which
stream every read-out call names, and that the packed reads convert what the float reads return.  Every comparison is an exact equality: the
calls under test only look up, select and copy."""
import ctypes as C

import numpy as np
import pytest

ERR_INVALID, ERR_NOT_FOUND = -2, -6  # SDRPP_ERR_INVALID, SDRPP_ERR_NOT_FOUND (include/sdrpp_gpu.h)
SR, B = 10e6, 40000
fp, vp = C.POINTER(C.c_float), C.c_void_p


def _signal(n, f0s, seed):
    """Carriers of amplitude 0.05 at `f0s` with a 1 kHz FM tone, 60 dB down after the first eighth, + noise."""
    r = np.random.default_rng(seed)
    t = np.arange(n) / SR
    g = np.where(np.arange(n) < n // 8, 1.0, 0.001)
    x = sum(0.05 * g * np.exp(1j * (2 * np.pi * f * t + 5.0 * np.sin(2 * np.pi * 1000.0 * t))) for f in f0s)
    return (x + 1e-4 * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64)


def _fails(ctx, rc, code, text):
    assert rc == code, (rc, code, ctx.L.sdrpp_last_error(ctx.h).decode())
    msg = ctx.L.sdrpp_last_error(ctx.h).decode()
    assert text in msg, (text, msg)


def _f32(n):
    return np.zeros((max(n, 1), 2), np.float32)


def _triple(ctx, prefix, vid=None):
    """<prefix>_count / _read / _device_buffer as calls that return the rc (the pre-processing chain's take no id and spell two names differently)"""
    L, buf, p, n = ctx.L, _f32(16), vp(), C.c_int()
    if vid is None:
        return [lambda: L.sdrpp_preproc_out_count(ctx.h), lambda: L.sdrpp_preproc_read(ctx.h, buf.ctypes.data_as(fp), 16),
                lambda: L.sdrpp_preproc_device_buffer(ctx.h, C.byref(p), C.byref(n))]
    f = lambda name: getattr(L, "sdrpp_vfo_%s_%s" % (prefix, name))
    return [lambda: f("count")(ctx.h, vid), lambda: f("read")(ctx.h, vid, buf.ctypes.data_as(fp), 16), lambda: f("device_buffer")(ctx.h, vid, C.byref(p), C.byref(n))]


def _read_many_rc(ctx, vids, which):
    n = len(vids)
    offs, cnts = (C.c_int64 * n)(), (C.c_int * n)()
    return ctx.L.sdrpp_vfo_read_many(ctx.h, n, (C.c_int * n)(*vids), (C.c_int * n)(*which), None, 0, offs, cnts)


def _from_device(ctx, ptr, n):
    """n complex samples at device address `ptr`, fetched with sdrpp_device_copy (device to host) once the context's stream is idle"""
    out = _f32(n)
    ctx.sync()
    if n:
        ctx._chk(ctx.L.sdrpp_device_copy(ctx.h, vp(out.ctypes.data), vp(ptr), n * 8, 2))
    return out[:n]


def _buffer(ctx, fn, vid):
    p, n = vp(), C.c_int()
    ctx._chk(fn(ctx.h, vid, C.byref(p), C.byref(n)))
    return _from_device(ctx, p.value, n.value)


def _same(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def _pairs(z):
    return np.ascontiguousarray(z).view(np.float32).reshape(-1, 2)


def _pcm(f, scale, dt):
    """volk_32f_s32f_convert_16i / _8i: float32 product, clamp to the integer range, round half to even"""
    info = np.iinfo(dt)
    r = np.ascontiguousarray(f, np.float32) * np.float32(scale)
    return np.rint(np.clip(r, np.float32(info.min), np.float32(info.max))).astype(dt)


@pytest.fixture
def bank(backend):
    """A WFM VFO with an AF chain and a RAW VFO whose squelch (reference blocks of half a push) passes the first half of a push (the carrier, which the chain's filters
    delay by about 55 of the 100 IF samples: -19 dB) and closes on the second (the noise floor: -43 dB)."""
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=B)
    ctx.set_reference_block(B // 2)
    d, keep = radio.vfo_desc(SR, 250e3, 150e3, 0.9e6, "WFM")
    wfm = ctx.vfo_add(d, keep)
    a, akeep = radio.af_desc(250e3, 48000.0, 50e-6, False)
    ctx.vfo_set_af(wfm, a, akeep)
    rd, rkeep = radio.vfo_desc(SR, 50e3, 50e3, -1.2e6, "RAW")
    raw = ctx.vfo_add(rd, rkeep)
    ctx.vfo_set_if(raw, radio.if_desc(50e3, squelch=-30.0))
    yield ctx, wfm, raw, (rd, rkeep)
    ctx.close()


def test_unknown_id_is_not_found_everywhere(bank):
    """Every entry point that takes a VFO id, with arguments that are otherwise valid: SDRPP_ERR_NOT_FOUND and "no VFO <id>" — before and after a push."""
    from sdrplusplus_amd import radio

    ctx, wfm, raw, (rd, _) = bank
    L, h = ctx.L, ctx.h
    bad = 4711
    buf, pcm, taps = _f32(64), np.zeros(1024, np.uint8), np.ones(3, np.float32)
    p, q, n, m, nid = vp(), vp(), C.c_int(), C.c_int(), C.c_int()
    ifd = radio.if_desc(50e3, squelch=-30.0)
    af, _ = radio.af_desc(250e3, 48000.0, 50e-6, False)
    calls = {
        "remove": lambda: L.sdrpp_vfo_remove(h, bad),
        "replace": lambda: L.sdrpp_vfo_replace(h, bad, C.byref(rd), 7, C.byref(nid)),
        "set_phase_delta": lambda: L.sdrpp_vfo_set_phase_delta(h, bad, 1.0, 0.0),
        "set_ssb_phase_delta": lambda: L.sdrpp_vfo_set_ssb_phase_delta(h, bad, 1.0, 0.0),
        "set_channel_taps": lambda: L.sdrpp_vfo_set_channel_taps(h, bad, taps.ctypes.data_as(fp), 3),
        "reset": lambda: L.sdrpp_vfo_reset(h, bad),
        "set_af": lambda: L.sdrpp_vfo_set_af(h, bad, C.byref(af)),
        "set_af(None)": lambda: L.sdrpp_vfo_set_af(h, bad, None),
        "set_if": lambda: L.sdrpp_vfo_set_if(h, bad, C.byref(ifd)),
        "set_if(None)": lambda: L.sdrpp_vfo_set_if(h, bad, None),
        "out_count": lambda: L.sdrpp_vfo_out_count(h, bad),
        "read": lambda: L.sdrpp_vfo_read(h, bad, buf.ctypes.data_as(fp), 64),
        "device_buffers": lambda: L.sdrpp_vfo_device_buffers(h, bad, C.byref(p), C.byref(n), C.byref(q), C.byref(m)),
        "af_count": lambda: L.sdrpp_vfo_af_count(h, bad),
        "af_read": lambda: L.sdrpp_vfo_af_read(h, bad, buf.ctypes.data_as(fp), 64),
        "af_device_buffer": lambda: L.sdrpp_vfo_af_device_buffer(h, bad, C.byref(p), C.byref(n)),
        "ifc_count": lambda: L.sdrpp_vfo_ifc_count(h, bad),
        "ifc_read": lambda: L.sdrpp_vfo_ifc_read(h, bad, buf.ctypes.data_as(fp), 64),
        "ifc_device_buffer": lambda: L.sdrpp_vfo_ifc_device_buffer(h, bad, C.byref(p), C.byref(n)),
        "read_pcm": lambda: L.sdrpp_vfo_read_pcm(h, bad, 0, 1, 32767.0, pcm.ctypes.data_as(vp), 64),
        "read_compressed": lambda: L.sdrpp_vfo_read_compressed(h, bad, 0, 1, pcm.ctypes.data_as(C.POINTER(C.c_uint8)), 1024),
        "read_many": lambda: _read_many_rc(ctx, [bad], [0]),
        "read_many (second element)": lambda: _read_many_rc(ctx, [wfm, bad, raw], [0, 0, 0]),
    }
    for pushed in (False, True):
        if pushed:
            ctx.push(_signal(B, (0.9e6, -1.2e6), 1))
        for name, call in calls.items():
            ctx.sync()  # (clears nothing: the message asserted below must come from the call itself)
            L.sdrpp_vfo_set_ssb_phase_delta(h, wfm, 1.0, 0.0)  # a different failure in between: "... has no SSB demodulator"
            rc = call()
            assert rc == ERR_NOT_FOUND, (name, rc)
            assert "no VFO %d" % bad in L.sdrpp_last_error(h).decode(), (name, L.sdrpp_last_error(h).decode())
    assert ctx.vfo_count() == 2  # the failed replace added nothing
    assert len(ctx.vfo_read(wfm)) > 0 and len(ctx.vfo_read(raw)) > 0


def test_missing_chain_is_invalid_with_its_own_message(bank):
    from sdrplusplus_amd import radio

    ctx, wfm, raw, (rd, rkeep) = bank
    L, h = ctx.L, ctx.h
    off = ctx.vfo_add(rd, rkeep)
    ctx.vfo_set_if(off, radio.if_desc(50e3, nb=False, squelch=None))  # attached, both blocks disabled
    ctx.push(_signal(B, (0.9e6, -1.2e6), 2))
    pcm = np.zeros(4096, np.uint8)
    for call in _triple(ctx, "af", raw):
        _fails(ctx, call(), ERR_INVALID, "VFO %d has no AF chain" % raw)
    for vid in (wfm, off):
        for call in _triple(ctx, "ifc", vid):
            _fails(ctx, call(), ERR_INVALID, "VFO %d has no active IF chain" % vid)
    for call in _triple(ctx, "preproc"):
        _fails(ctx, call(), ERR_INVALID, "no pre-processing chain configured")
    _fails(ctx, L.sdrpp_preproc_read_pcm(h, 1, 32767.0, pcm.ctypes.data_as(vp), 16), ERR_INVALID, "no pre-processing chain configured")
    for vid, which in ((raw, 2), (wfm, 3), (off, 2), (off, 3), (wfm, 4), (raw, 4), (raw, -1)):
        text = "VFO %d has no such stream (%d)" % (vid, which)
        for pcm_type in (0, 1):
            _fails(ctx, L.sdrpp_vfo_read_pcm(h, vid, which, pcm_type, 100.0, pcm.ctypes.data_as(vp), 16), ERR_INVALID, text)
        _fails(ctx, L.sdrpp_vfo_read_compressed(h, vid, which, 1, pcm.ctypes.data_as(C.POINTER(C.c_uint8)), 4096), ERR_INVALID, text)
        _fails(ctx, _read_many_rc(ctx, [vid], [which]), ERR_INVALID, text)
        _fails(ctx, _read_many_rc(ctx, [wfm, vid], [0, which]), ERR_INVALID, text)
    # the streams that do exist are unaffected by the refusals
    assert ctx.vfo_af_count(wfm) > 0 and ctx.vfo_ifc_count(raw) > 0 and ctx.vfo_out_count(off) > 0
    # a detached AF chain / a detached IF chain: the same refusals
    ctx.vfo_set_af(wfm, None)
    ctx.vfo_set_if(raw, None)
    for call in _triple(ctx, "af", wfm):
        _fails(ctx, call(), ERR_INVALID, "VFO %d has no AF chain" % wfm)
    for call in _triple(ctx, "ifc", raw):
        _fails(ctx, call(), ERR_INVALID, "VFO %d has no active IF chain" % raw)


def test_every_read_out_call_names_the_stream_it_should(bank):
    """which = 0: what the VFO delivers (the demodulator's output; a RAW VFO's IF stream, behind an active IF chain the chain's output), 1: the IF stream in
    front of the IF chain, 2: the AF chain's output, 3: the IF chain's output.  sdrpp_vfo_read / _device_buffers(out) are 0, _device_buffers(if_out) is 1,
    the af_* calls 2, the ifc_* calls 3."""
    ctx, wfm, raw, _ = bank
    L = ctx.L
    ctx.push(_signal(B, (0.9e6, -1.2e6), 3))

    def views(vid, whichs):
        got = {w: ctx.vfo_read_many([vid], which=[w])[0].copy() for w in whichs}
        for w, a in got.items():
            assert len(a) > 0 and np.any(a != 0), (vid, w)
            assert _same(a, ctx.vfo_read_many([wfm, raw, vid], which=[0, 0, w])[2]), (vid, w)  # ... at any place of a gather
        p, q, n, m = vp(), vp(), C.c_int(), C.c_int()
        ctx._chk(L.sdrpp_vfo_device_buffers(ctx.h, vid, C.byref(p), C.byref(n), C.byref(q), C.byref(m)))
        assert n.value == ctx.vfo_out_count(vid)
        return got, _from_device(ctx, p.value, n.value), _from_device(ctx, q.value, m.value)

    # WFM + AF chain: audio at 250 kS/s, IF at 250 kS/s, AF output at 48 kS/s
    w, dev_out, dev_if = views(wfm, (0, 1, 2))
    assert len(w[0]) == len(w[1]) > len(w[2])
    assert not _same(w[0], w[1])
    assert _same(ctx.vfo_read(wfm), w[0]) and _same(dev_out, w[0]) and _same(ctx.vfo_read_many([wfm])[0], w[0])
    assert _same(dev_if, w[1]) and _same(_pairs(ctx.vfo_read_if(wfm)), w[1])
    assert _same(ctx.vfo_af_read(wfm), w[2]) and _same(_buffer(ctx, L.sdrpp_vfo_af_device_buffer, wfm), w[2])
    assert ctx.vfo_af_count(wfm) == len(w[2])

    # RAW + squelch: the chain's output is what the VFO delivers; the IF in front of it stays readable
    r, dev_out, dev_if = views(raw, (0, 1, 3))
    assert len(r[3]) == len(r[1])
    k = int(np.argmax(np.all(r[3] == 0, axis=1) & np.any(r[1] != 0, axis=1)))  # open on the first reference block, closed on the second
    assert 0 < k < len(r[1]) and _same(r[3][:k], r[1][:k]) and not np.any(r[3][k:]) and np.all(np.any(r[1][k:] != 0, axis=1))
    assert _same(r[0], r[3]) and _same(ctx.vfo_read(raw), r[3]) and _same(dev_out, r[3])
    assert _same(_pairs(ctx.vfo_ifc_read(raw)), r[3]) and _same(ctx.vfo_read(raw), _pairs(ctx.vfo_ifc_read(raw)))
    assert _same(_buffer(ctx, L.sdrpp_vfo_ifc_device_buffer, raw), r[3]) and ctx.vfo_ifc_count(raw) == len(r[3])
    assert _same(dev_if, r[1])

    # chain detached: the VFO delivers its IF stream again — at once (the last push's) and after the next push
    ctx.vfo_set_if(raw, None)
    for again in (False, True):
        if again:
            ctx.push(_signal(B, (0.9e6, -1.2e6), 4))
        one = ctx.vfo_read_many([raw], which=[1])[0]
        assert len(one) > k and np.all(np.any(one[k:] != 0, axis=1))
        assert _same(ctx.vfo_read(raw), one) and _same(ctx.vfo_read_many([raw], which=[0])[0], one)
        assert ctx.vfo_out_count(raw) == len(one)
    assert _same(ctx.vfo_read(wfm), ctx.vfo_read_many([wfm], which=[0])[0])


def test_packed_reads_convert_what_the_float_reads_return(bank):
    ctx, wfm, raw, _ = bank
    ctx.push(_signal(B, (0.9e6, -1.2e6), 5))
    for vid, whichs in ((wfm, (0, 1, 2)), (raw, (0, 1, 3))):
        for which in whichs:
            f = ctx.vfo_read_many([vid], which=[which])[0].copy()
            if which == 0:
                assert _same(f, ctx.vfo_read(vid))
            for pcm_type, dt, scale in ((1, np.int16, 32767.0), (1, np.int16, 3.0e6), (0, np.int8, 100.0), (0, np.int8, 1.0e5)):  # (the large scales clamp)
                want = _pcm(f, scale, dt)
                assert len(np.unique(want)) > 2
                got = ctx.vfo_read_pcm(vid, which, pcm_type, scale, len(f))
                assert got.dtype == dt and got.shape == want.shape and np.array_equal(got, want), (vid, which, pcm_type, scale)
                k = len(f) // 3  # fewer frames than there are: the first k
                assert np.array_equal(ctx.vfo_read_pcm(vid, which, pcm_type, scale, k), want[:k])


def test_preproc_packed_read_converts_what_the_float_read_returns(backend):
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=B)
    ctx.preproc_configure(radio.plans().stages(2), 50.0 / (SR / 2), True)
    ctx.push(_signal(B, (0.9e6,), 6))
    z = ctx.preproc_read()
    assert len(z) == B // 2
    p, n = vp(), C.c_int()
    ctx._chk(ctx.L.sdrpp_preproc_device_buffer(ctx.h, C.byref(p), C.byref(n)))
    assert n.value == len(z) and _same(_from_device(ctx, p.value, n.value), _pairs(z))
    for pcm_type, dt, scale in ((1, np.int16, 32767.0), (0, np.int8, 100.0), (0, np.int8, 1.0e5)):
        want = _pcm(_pairs(z), scale, dt)
        assert len(np.unique(want)) > 2
        got = ctx.preproc_read_pcm(pcm_type, scale)
        assert got.dtype == dt and got.shape == want.shape and np.array_equal(got, want), (pcm_type, scale)
        assert np.array_equal(ctx.preproc_read_pcm(pcm_type, scale, 1000), want[:1000])
    ctx.close()
