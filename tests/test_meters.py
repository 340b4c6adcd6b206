"""Signal meters for a table of bands on every raw line of every push (sdrpp_wf_set_meters / sdrpp_wf_meters_read / sdrpp_result_meters).

The truth is the oracle's orc_wf_signal_info (pinned bit for bit to the reference's calculateVFOSignalInfo by tests/test_oracle_vs_reference.py),
driven line by line through orc_wf_push.  Tolerances are those of tests/test_parity_fft.py: strength exact; |snr - oracle| < 1e-5 (the double
sums differ by ~1e-13 relative between the device's tree and the reference's bin order, the float difference max - avg is one rounding at
magnitudes under 128 dB); an empty pair of side bands gives NaN on both sides.  Every compared band ends below +sr/2 (beyond it the reference
reads one bin past the line and the device clamps: include/sdrpp_gpu.h)."""
import ctypes as C
import functools

import numpy as np
import pytest

import support as S

SR = 10e6
ERR_INVALID, ERR_UNSUPPORTED, ERR_NOT_FOUND = -2, -5, -6   # include/sdrpp_gpu.h
PUSHES = [512, 1024, 3 * 1024 + 17, 100, 5 * 1024]   # blocks of 0, 1 and several lines, one line straddles pushes
# wide | lower edge: the clamp to bin 0 empties the left side band | all four offsets in bin 614 of 1024: no side bands at all -> snr NaN | narrow
SPECIAL = [(1.0e6, 400e3), (-4.9e6, 200e3), (1.0028e6, 1e3), (-3.0e6, 12.5e3)]


def table(n):
    if n == 1:
        return SPECIAL[:1]
    t = list(SPECIAL[:3]) if n == 3 else list(SPECIAL)
    rng = np.random.default_rng(5)
    while len(t) < n:
        bw = float(rng.choice([12.5e3, 50e3, 150e3, 400e3, 1.2e6]))
        centre = float(rng.uniform(-SR / 2 + 1e3, SR / 2 - bw - 1e3))   # upper edge centre + bw stays below +sr/2
        t.append((centre, bw))
    assert all(c + b < SR / 2 for c, b in t)
    return t


@functools.lru_cache(maxsize=None)
def stream():
    from sdrplusplus_amd import workloads

    x = workloads.synth(2, sum(PUSHES), seed=31)
    x.setflags(write=False)
    return x


class OracleMeter:
    """orc_wf_push + orc_wf_signal_info: the reference's meter on the line pushed last."""

    def __init__(self, N):
        o = S.oracle()
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        o.orc_wf_create.restype = C.c_void_p
        o.orc_wf_create.argtypes = [C.c_int, C.c_int, C.c_int]
        o.orc_wf_destroy.argtypes = [C.c_void_p]
        o.orc_wf_push.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_float, C.c_float, ip]
        o.orc_wf_signal_info.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, fp, fp]
        self.o, self.N, self.h = o, N, o.orc_wf_create(2, N, 16)
        self.idx = np.empty(16, np.int32)

    def row(self, line, bands):
        line = np.ascontiguousarray(line, np.float32)
        self.o.orc_wf_push(self.h, line.ctypes.data_as(C.POINTER(C.c_float)), 0, self.N, -120.0, 0.0, self.idx.ctypes.data_as(C.POINTER(C.c_int32)))
        out = np.empty((len(bands), 2), np.float32)
        a, b = C.c_float(), C.c_float()
        for m, (centre, bw) in enumerate(bands):
            assert self.o.orc_wf_signal_info(self.h, centre, bw, SR, C.byref(a), C.byref(b)) == 1
            out[m] = a.value, b.value
        return out

    def __del__(self):
        self.o.orc_wf_destroy(self.h)


@functools.lru_cache(maxsize=None)
def oracle_rows(N, nz, n_meters, pushes):
    """-> per push: (oracle lines [k, N], oracle meters [k, n_meters, 2])"""
    from sdrplusplus_amd import capi

    spec = S.OracleSpectrum(N, nz, 0, capi.design_fft_window(2, nz))
    om = OracleMeter(N)
    bands, x, out, pos = table(n_meters), stream(), [], 0
    for n in pushes:
        lines = spec.push(x[pos:pos + n])
        pos += n
        out.append((lines, np.stack([om.row(ln, bands) for ln in lines]) if len(lines) else np.empty((0, n_meters, 2), np.float32)))
    return out


def check(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    assert np.array_equal(got[..., 0].view(np.uint32), want[..., 0].view(np.uint32)), "strength differs from the oracle"
    nan = np.isnan(want[..., 1])
    assert np.array_equal(np.isnan(got[..., 1]), nan), "NaN snr (empty side bands) in other places than the oracle's"
    err = float(np.max(np.abs(got[..., 1][~nan].astype(np.float64) - want[..., 1][~nan]))) if (~nan).any() else 0.0
    print("worst |snr - oracle| = %.3g dB" % err)
    assert err < 1e-5, err
    return err


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_ctx(N=1024, nz=None, max_push=None, ring=0):
    from sdrplusplus_amd import capi

    nz = nz or N
    ctx = capi.Context(0, max_push=max_push or max(PUSHES))
    ctx.fft_configure(N, nz, 0, capi.design_fft_window(2, nz))
    if ring:
        ctx.wf_configure(ring)
    return ctx


def test_single_bin_band_is_nan_in_the_oracle():
    """the case the parity test relies on, on the CPU: centre 1.0028e6, bandwidth 1e3 puts all four offsets into one bin of a 1024-point line"""
    rows = oracle_rows(1024, 1024, 3, tuple(PUSHES))
    for lines, met in rows:
        for f in range(len(lines)):
            assert np.isnan(met[f, 2, 1]) and met[f, 2, 0] == lines[f, 614]
            assert not np.isnan(met[f, 1, 1])   # the lower-edge band keeps its right side band


@pytest.mark.parametrize("n_meters", [1, 3, 130])
def test_parity_every_line_every_meter(backend, n_meters):
    """Ordinary passes: every (line, meter) against the oracle; the raw lines still equal the oracle's; with a history ring configured the row of
    the newest line is bit-identical to sdrpp_wf_signal_info for the same band (one arithmetic, two callers)."""
    bands = table(n_meters)
    ctx = make_ctx(ring=4)
    ctx.wf_set_meters(bands, SR)
    pos, x, total = 0, stream(), 0
    for n, (olines, omet) in zip(PUSHES, oracle_rows(1024, 1024, n_meters, tuple(PUSHES))):
        ctx.push(x[pos:pos + n])
        pos += n
        raw, _, _ = ctx.fft_read()
        assert same_bits(raw, olines)
        got = ctx.wf_meters()
        check(got, omet)
        total += len(got)
        if len(got):
            for m in list(range(min(n_meters, 6))) + [n_meters - 1]:
                s, q = ctx.wf_signal_info(bands[m][0], bands[m][1], SR)
                assert same_bits(np.array([s, q], np.float32), got[-1, m]), (m, s, q, got[-1, m])
    assert total == sum(PUSHES) // 1024
    ctx.close()


@pytest.mark.parametrize("N", [4096, 65536])
def test_both_line_producing_families(backend, N):
    """the same stream as ONE block at 4096 points (single-pass transform) and 65536 points (two passes; frames of 4096 samples, zero-padded):
    an ordinary pass and a pipelined block, both against the oracle"""
    whole = (sum(PUSHES),)
    (olines, omet), = oracle_rows(N, 4096, 130, whole)
    assert len(olines) == 2
    for pipelined in (False, True):
        ctx = make_ctx(N, 4096, max_push=whole[0])
        ctx.wf_set_meters(table(130), SR)
        if pipelined:
            ctx.set_pipelined(True, 4)
        ctx.push(stream())
        if pipelined:
            r = ctx.result_wait(ctx.ticket())
            got = ctx.result_meters(ctx.ticket())
            ctx.result_release(ctx.ticket())
            assert same_bits(r["raw"], olines)
            st = ctx.pipeline_stats()
            assert st["tick_blocks"] == 1 and st["pass_blocks"] == 0 and st["roles"].get("wf_ring", 0) > 0, st
        else:
            got = ctx.wf_meters()
        check(got, omet)
        ctx.close()


_pass_rows = {}


def pass_rows(backend, n_meters):
    """the ordinary pass on the stream, push by push (per backend, computed once): what every structure case must reproduce bit for bit"""
    key = (backend, n_meters)
    if key not in _pass_rows:
        ctx = make_ctx()
        ctx.wf_set_meters(table(n_meters), SR)
        pos, x, rows = 0, stream(), []
        for n in PUSHES:
            ctx.push(x[pos:pos + n])
            pos += n
            rows.append(ctx.wf_meters())
        ctx.close()
        _pass_rows[key] = rows
    return _pass_rows[key]


def run_pipelined(ctx, on_push=None):
    """pushes the stream, then collects every ticket -> [(n_lines, meters or None when the block carries none)]"""
    from sdrplusplus_amd import capi

    pos, x, tickets, out = 0, stream(), [], []
    for i, n in enumerate(PUSHES):
        if on_push:
            on_push(i)
        ctx.push(x[pos:pos + n])
        pos += n
        tickets.append(ctx.ticket())
    for t in tickets:
        r = ctx.result_wait(t)
        try:
            m = ctx.result_meters(t)
        except capi.SdrppError as e:
            assert e.code == ERR_NOT_FOUND, e
            m = None
        ctx.result_release(t)
        out.append((r["n_lines"], m))
    return out


@pytest.mark.parametrize("group", [1, 4])
def test_pipelined_equals_the_ordinary_pass(backend, group):
    """one block per launch, and launch groups of four (adaptive = 0: the first four pushes share a launch, every push gets the meters of the lines
    its own samples completed): bit-identical to the ordinary pass, whichever way the stream is cut"""
    want = pass_rows(backend, 130)
    ctx = make_ctx(max_push=sum(PUSHES))
    ctx.wf_set_meters(table(130), SR)
    ctx.set_pipelined(True, 4)
    if group > 1:
        ctx.set_pipeline_group(group, adaptive=False)
    got = run_pipelined(ctx)
    st = ctx.pipeline_stats()
    assert st["pass_blocks"] == 0 and st["roles"].get("wf_ring", 0) > 0, st
    if group > 1:
        assert ctx.pipeline_group_stats()["largest"] == 4
    for (nl, m), w in zip(got, want):
        assert nl == len(w) and m is not None and same_bits(m, w)
    ctx.close()


def test_results_without_any_result_flag(backend):
    """no new result flag: with result_flags = 0 a table alone makes every block deliver (and only) its meters"""
    want = pass_rows(backend, 3)
    ctx = make_ctx()
    ctx.wf_set_meters(table(3), SR)
    ctx.set_pipelined(True, 0)
    for (nl, m), w in zip(run_pipelined(ctx), want):
        assert nl == len(w) and same_bits(m, w)
    ctx.close()


def test_table_replaced_and_set_late(backend):
    """A table set in the middle of a run applies from the next push; blocks already pushed keep the table they were pushed with (rows AND
    n_meters) although nothing has been drained; blocks pushed before any table: SDRPP_ERR_NOT_FOUND."""
    a, b = pass_rows(backend, 3), pass_rows(backend, 130)
    ctx = make_ctx()
    ctx.set_pipelined(True, 4)

    def on_push(i):
        if i == 1:
            ctx.wf_set_meters(table(3), SR)
        if i == 3:
            ctx.wf_set_meters(table(130), SR)

    got = run_pipelined(ctx, on_push)
    assert got[0][1] is None
    for i in (1, 2):
        assert same_bits(got[i][1], a[i]) and got[i][1].shape[1] == 3
    for i in (3, 4):
        assert same_bits(got[i][1], b[i]) and got[i][1].shape[1] == 130
    assert got[4][0] == 5
    ctx.close()


def test_removal_limits_and_errors(backend):
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max(PUSHES))
    with pytest.raises(capi.SdrppError) as e:   # needs sdrpp_fft_configure
        ctx.wf_set_meters(table(1), SR)
    assert e.value.code == ERR_INVALID
    ctx.fft_configure(1024, 1024, 0, capi.design_fft_window(2, 1024))
    with pytest.raises(capi.SdrppError) as e:   # the documented limit
        ctx.wf_set_meters([(0.0, 1e3)] * (capi.MAX_METERS + 1), SR)
    assert e.value.code == ERR_UNSUPPORTED
    assert capi.MAX_METERS >= 1024
    ctx.wf_set_meters([(0.0, 1e3)] * capi.MAX_METERS, SR)
    ctx.wf_set_meters(table(3), SR)
    ctx.push(stream()[:2048])
    assert ctx.wf_meters().shape == (2, 3, 2)
    ctx.wf_set_meters([], SR)   # n = 0 removes the table
    ctx.push(stream()[2048:4096])
    assert ctx.wf_meters().shape == (0, 0, 2)
    ctx.set_pipelined(True, 31)   # every existing flag together is still accepted (there is no flag for the meters)
    ctx.push(stream()[4096:6144])
    t = ctx.ticket()
    assert ctx.result_wait(t)["n_lines"] == 2
    with pytest.raises(capi.SdrppError) as e:
        ctx.result_meters(t)
    assert e.value.code == ERR_NOT_FOUND
    ctx.result_release(t)
    with pytest.raises(capi.SdrppError) as e:   # valid between wait and release only
        ctx.result_meters(t)
    assert e.value.code == ERR_INVALID
    ctx.close()


def test_fft_size_change_keeps_the_table(backend):
    """the table is kept as frequencies: another FFT size recomputes the offsets"""
    from sdrplusplus_amd import capi

    ctx = make_ctx(4096, 4096, max_push=sum(PUSHES))
    ctx.wf_set_meters(table(3), SR)
    ctx.fft_configure(1024, 1024, 0, capi.design_fft_window(2, 1024))
    ctx.push(stream()[:PUSHES[0] + PUSHES[1]])
    _, omet = oracle_rows(1024, 1024, 3, (PUSHES[0] + PUSHES[1],))[0]
    check(ctx.wf_meters(), omet)
    ctx.close()


def test_bank_results_untouched_by_a_table(backend):
    """a bank with VFOs, result_flags = 3 (VFO blocks + zoomed lines): with a table set, the VFO blocks, lines and palette indices of every block are
    byte-identical to the same run without one — and the run without one plans no meter role"""
    from sdrplusplus_amd import radio

    def run(with_table):
        ctx = make_ctx()
        ctx.fft_set_view(0, 1024, 256, -120.0, 0.0)
        vfos = [(1.0e6, 150e3), (-2.0e6, 150e3)]
        for off, bw in vfos:
            d, keep = radio.vfo_desc(SR, 250e3, bw, off, "WFM")
            ctx.vfo_add(d, keep)
        if with_table:
            ctx.wf_set_meters(radio.meter_table(vfos), SR)
        ctx.set_pipelined(True, 3)
        pos, x, tickets, out = 0, stream(), [], []
        for n in PUSHES:
            ctx.push(x[pos:pos + n])
            pos += n
            tickets.append(ctx.ticket())
        for t in tickets:
            r = ctx.result_wait(t)
            m = ctx.result_meters(t) if with_table else None
            ctx.result_release(t)
            out.append((r, m))
        st = ctx.pipeline_stats()
        ctx.close()
        return out, st

    plain, st0 = run(False)
    metered, st1 = run(True)
    assert "wf_ring" not in st0["roles"]
    assert (st1["tick_blocks"], st1["pass_blocks"]) == (st0["tick_blocks"], st0["pass_blocks"])
    if st1["tick_blocks"]:
        assert st1["roles"].get("wf_ring", 0) > 0
    for (r0, _), (r1, m) in zip(plain, metered):
        assert r0["n_lines"] == r1["n_lines"] == len(m) and m.shape[1:] == (2, 2)
        assert sorted(r0["vfo"]) == sorted(r1["vfo"])
        for vid in r0["vfo"]:
            assert same_bits(r0["vfo"][vid], r1["vfo"][vid])
        if r0["n_lines"]:
            assert same_bits(r0["zoomed"], r1["zoomed"]) and np.array_equal(r0["index"], r1["index"])
