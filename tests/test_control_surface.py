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


ERR_UNSUPPORTED = -5      # SDRPP_ERR_UNSUPPORTED
MAX_DECIM_STAGES = 4      # SDRPP_MAX_DECIM_STAGES
B_SMALL = 4000            # 100 IF samples at 250 kS/s behind the resampler, 125 in front of it


def _clone(d):
    c = type(d)()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(d))
    return c


def _stage_faults(n_stages):
    """(what, code, edit of a description's stage fields, the stage the message names or None): one fault each, in the last stage"""
    s = n_stages - 1
    return [
        ("n_stages -1", ERR_INVALID, lambda d: setattr(d, "n_stages", -1), None),
        ("n_stages max + 1", ERR_INVALID, lambda d: setattr(d, "n_stages", MAX_DECIM_STAGES + 1), None),
        ("decimation 3", ERR_UNSUPPORTED, lambda d: d.stage_decim.__setitem__(s, 3), s),
        ("no taps", ERR_UNSUPPORTED, lambda d: d.stage_ntaps.__setitem__(s, 0), s),
        ("null taps", ERR_UNSUPPORTED, lambda d: d.stage_taps.__setitem__(s, fp()), s),
    ]


def _poly_faults():
    return [
        ("resamp_ntaps 0", lambda d: setattr(d, "resamp_ntaps", 0)),
        ("resamp_taps null", lambda d: setattr(d, "resamp_taps", fp())),
        ("interp 0", lambda d: setattr(d, "interp", 0)),
    ]


def _through(n, decims):
    """outputs of power-of-two decimators that start at sample 0"""
    for D in decims:
        n = (n + D - 1) // D
    return n


def test_description_faults_name_their_chain(backend):
    """A decimator + resampler description with exactly one fault, at each of the four entry points that take one: the code, the chain's prefix and the stage
    in the message, and what the rejected call leaves behind — no VFO more, no AF chain (sdrpp_vfo_set_af detaches before it looks), the old RDS branch and the
    old pre-processing chain as they were (compared bit for bit with a twin that saw no rejected call)."""
    from sdrplusplus_amd import capi, radio

    ctx = capi.Context(0, max_push=B_SMALL)
    L, h = ctx.L, ctx.h
    vd, vkeep = radio.vfo_desc(SR, 250e3, 150e3, 0.9e6, "WFM")
    ad, akeep = radio.af_desc(250e3, 48000.0, 50e-6, False)
    rd, rkeep = radio.rds_desc(250e3)
    for d in (vd, ad, rd):
        assert d.n_stages >= 2 and d.interp != d.decim and d.resamp_ntaps > 0
    twins = [ctx.vfo_add(vd, vkeep) for _ in range(2)]  # the same VFO twice: every rejected call below goes to the first
    a, b = twins
    for v in twins:
        ctx.vfo_set_af(v, ad, akeep)
        ctx.vfo_set_rds(v, rd, True, rkeep)
    nid = C.c_int()
    entry = {
        "": lambda d: L.sdrpp_vfo_add(h, C.byref(d), C.byref(nid)),
        "af ": lambda d: L.sdrpp_vfo_set_af(h, a, C.byref(d)),
        "rds ": lambda d: L.sdrpp_vfo_set_rds(h, a, C.byref(d), 1),
    }
    for prefix, good in (("", vd), ("af ", ad), ("rds ", rd)):
        faults = [(w, code, e, (prefix + "n_stages %d" % (-1 if "-1" in w else MAX_DECIM_STAGES + 1)) if s is None else prefix + "stage %d:" % s)
                  for w, code, e, s in _stage_faults(good.n_stages)]
        faults += [(w, ERR_INVALID, e, "bad %spolyphase description" % prefix) for w, e in _poly_faults()]
        for what, code, edit, text in faults:
            bad = _clone(good)
            edit(bad)
            rc = entry[prefix](bad)
            _fails(ctx, rc, code, text)
            if not text.startswith("bad "):  # the message begins with the prefix (the front end's, which has none, with the text itself)
                assert L.sdrpp_last_error(h).decode().startswith(text), (prefix, what, L.sdrpp_last_error(h).decode())
            assert ctx.vfo_count() == 2, (prefix, what)
            if prefix == "af ":  # the chain the VFO had is gone; the next fault meets a VFO with a chain again
                assert L.sdrpp_vfo_af_count(h, a) == ERR_INVALID, what
                ctx.vfo_set_af(a, ad, akeep)
            if prefix == "rds ":
                assert L.sdrpp_vfo_rds_count(h, a) >= 0, what
    ctx.push(_signal(B_SMALL, (0.9e6,), 7))
    ra, rb = ctx.vfo_rds_read(a), ctx.vfo_rds_read(b)
    n_rds = -(-_through(100, list(rd.stage_decim)[:rd.n_stages]) * rd.interp // rd.decim)  # 100 IF samples through the decimators, then the resampler from phase 0
    assert len(ra) == n_rds > 0 and _same(_pairs(ra), _pairs(rb)) and np.any(ra != 0)
    assert ctx.vfo_af_count(a) == ctx.vfo_af_count(b) > 0 and _same(ctx.vfo_af_read(a), ctx.vfo_af_read(b))
    ctx.close()

    # the pre-processing chain: arrays, no polyphase part; its n_stages range check has no message
    stages = radio.plans().stages(4)
    assert len(stages) >= 2
    arrs = [np.ascontiguousarray(t, np.float32) for _, t in stages]

    class Pre:  # the call's three arrays under the descriptions' field names
        def __init__(self):
            self.n_stages = len(stages)
            self.stage_decim = (C.c_int * (MAX_DECIM_STAGES + 1))(*[int(d) for d, _ in stages])
            self.stage_ntaps = (C.c_int * (MAX_DECIM_STAGES + 1))(*[len(t) for t in arrs])
            self.stage_taps = (fp * (MAX_DECIM_STAGES + 1))(*[t.ctypes.data_as(fp) for t in arrs])

    pair = [capi.Context(0, max_push=B_SMALL) for _ in range(2)]
    x = _signal(2 * B_SMALL, (0.9e6,), 8)
    for p in pair:
        p.preproc_configure(stages, 50.0 / (SR / 4), True)
        p.push(x[:B_SMALL])
    p0 = pair[0]
    for what, code, edit, s in _stage_faults(len(stages)):
        bad = Pre()
        edit(bad)
        rc = p0.L.sdrpp_preproc_configure(p0.h, bad.n_stages, bad.stage_decim, bad.stage_ntaps, bad.stage_taps, 0.0, 0)
        if s is None:
            assert rc == code, (what, rc)
        else:
            _fails(p0, rc, code, "pre-processing stage %d:" % s)
    for p in pair:
        p.push(x[B_SMALL:])
    za, zb = pair[0].preproc_read(), pair[1].preproc_read()
    assert len(za) == B_SMALL // 4 and _same(_pairs(za), _pairs(zb)) and np.any(za != 0)
    for p in pair:
        p.close()

    # interp == decim and no resampler taps: accepted, and the chain ends behind its decimators
    ctx = capi.Context(0, max_push=B_SMALL)
    flat = []
    for good in (vd, ad, rd):
        d = _clone(good)
        d.interp, d.decim, d.resamp_ntaps, d.resamp_taps = 5, 5, 0, fp()
        flat.append(d)
    v = ctx.vfo_add(flat[0], vkeep)
    ctx.vfo_set_af(v, flat[1], akeep)
    ctx.vfo_set_rds(v, flat[2], True, rkeep)
    ctx.push(_signal(B_SMALL, (0.9e6,), 9))
    n_if = _through(B_SMALL, list(vd.stage_decim)[:vd.n_stages])
    assert n_if == 125 and ctx.vfo_out_count(v) == n_if
    assert ctx.vfo_af_count(v) == _through(n_if, list(ad.stage_decim)[:ad.n_stages])
    assert ctx.vfo_rds_count(v) == _through(n_if, list(rd.stage_decim)[:rd.n_stages])
    ctx.close()
