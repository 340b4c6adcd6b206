"""Raw wire formats on the device (sdrpp_push_raw / sdrpp_push_frame / sdrpp_design_u8_table; csrc/ingest_kernels.h): int8, int16 and table-converted
uint8 IQ as the reference's sources receive it, and the frames of its server protocol.  Every value is exactly specified — (float)x * (1.0f / scalar),
or table[b] — so nothing here has a tolerance: floats are compared through their bits."""
import os
import struct

import numpy as np
import pytest

from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_ref.npz")
SCALARS = [128.0, 32768.0, 8192.0, 32768.0 * 2.5, 0.37]
PUSHES = [25000, 1031, 10000, 7, 16667, 25000, 25000, 6000]  # tests/test_pipelined.py::test_grouped_launches_equal_block_by_block (doubled on the device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def restate(raw, type_, scalar=None, table=None):
    """The yardstick: what the reference's conversion gives, value by value, in numpy's float32."""
    from sdrplusplus_amd import capi

    raw = np.asarray(raw).reshape(-1)
    if type_ == capi.IQ_U8:
        return np.asarray(table, dtype=f32)[raw.astype(np.int64)]
    inv = f32(1) / f32(scalar)
    assert inv.dtype == f32
    out = raw.astype(f32) * inv
    assert out.dtype == f32
    return out


def _conj_expected(vals):
    v = np.asarray(vals, dtype=f32).reshape(-1, 2).copy()
    v[:, 1] = -v[:, 1]
    return v.reshape(-1)


def np_u8_table(source, gain=1.0):
    from sdrplusplus_amd import capi

    b = np.arange(256, dtype=np.uint8)
    if source == capi.U8_RTL_SDR:  # ((float)b - 127.4) / 128.0f: double arithmetic on the float of b, the store rounds
        return ((b.astype(f32).astype(f64) - 127.4) / f64(f32(128))).astype(f32)
    if source == capi.U8_RTL_TCP:
        return ((b.astype(f64) - 128.0) / 128.0).astype(f32)
    d = b.astype(f32) - f32(128)
    den = f32(gain) * f32(128)
    scale = f32(1) / den
    out = d * scale
    assert d.dtype == f32 and den.dtype == f32 and scale.dtype == f32 and out.dtype == f32
    return out


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_decompressor():
    """x.astype(f32) * (f32(1) / f32(scalar)) with scalar = f32(32768 or 128) / f32(scaler) IS what SampleStreamDecompressor::process wrote, bit for bit."""
    from sdrplusplus_amd import capi

    g = np.load(GOLDEN)
    seen = 0
    for name in g["names"]:
        fr = g[name + "_frame"].tobytes()
        typ, scaler = struct.unpack_from("<Hf", fr, 2)
        n = int(g[name + "_count"][0])
        if typ not in (0, 1) or n == 0:
            continue
        raw = np.frombuffer(fr, np.int16 if typ == 1 else np.int8, 2 * n, 8)
        scalar = f32(32768 if typ == 1 else 128) / f32(scaler)
        assert scalar.dtype == f32
        _same(restate(raw, capi.IQ_I16 if typ == 1 else capi.IQ_I8, scalar), g[name + "_out"].reshape(-1), name)
        seen += 1
    assert seen >= 6


def test_u8_tables_in_each_sources_own_arithmetic(built):
    from sdrplusplus_amd import capi

    _same(capi.design_u8_table(capi.U8_RTL_SDR), np_u8_table(capi.U8_RTL_SDR), "rtl_sdr")
    _same(capi.design_u8_table(capi.U8_RTL_TCP), np_u8_table(capi.U8_RTL_TCP), "rtl_tcp")
    for gain in (1.0, 2.5):
        _same(capi.design_u8_table(capi.U8_SPYSERVER, gain), np_u8_table(capi.U8_SPYSERVER, gain), "spyserver gain %g" % gain)
    # (the types matter: the three expressions at gain 1 do not give the same table)
    assert not np.array_equal(_bits(np_u8_table(capi.U8_RTL_SDR)), _bits(np_u8_table(capi.U8_RTL_TCP)))
    with pytest.raises(capi.SdrppError):
        capi.design_u8_table(3)
    assert capi.load().sdrpp_design_u8_table(0, 1.0, None) == -2


def test_abi_sizeof_iq_format(built):
    import ctypes as C

    from sdrplusplus_amd import capi

    assert capi.load().sdrpp_abi_sizeof_iq_format() == C.sizeof(capi.IqFormat) == 16
    assert {"sdrpp_push_raw", "sdrpp_push_frame", "sdrpp_design_u8_table", "sdrpp_abi_sizeof_iq_format"} <= set(capi.EXPORTED_SYMBOLS)


# ---- values, observed directly -------------------------------------------------------------------------------------------------------------
def _conj_ctx(max_push, pipelined):
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=max_push)
    ctx.preproc_configure(conjugate=True)  # the only thing between the landing buffer and preproc_read: (re, -im)
    if pipelined:
        ctx.set_pipelined(True, 0)
    return ctx


def _every_8bit_value(dtype):
    """256 x 16 values: every value of the type at every position modulo 16 (a 16-byte source vector holds 16 of them)."""
    i = np.arange(4096)
    return ((i // 16 + 17 * (i % 16)) & 255).astype(np.uint8).view(dtype)


@pytest.mark.parametrize("pipelined", [False, True], ids=["immediate", "pipelined"])
def test_every_value_of_every_format(backend, pipelined):
    """Every int16 value (32768 samples), every int8 and uint8 value at every position of a 16-byte vector, at scalars 128, 32768, 8192, 32768 * 2.5 and
    0.37: what arrives behind a chain that only conjugates is conj(restatement), bit for bit — through ingest_kernel behind the raw copy (immediate) and
    through the tick's converting landing copy (pipelined)."""
    from sdrplusplus_amd import capi

    ctx = _conj_ctx(32768, pipelined)
    all16 = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    all8 = _every_8bit_value(np.int8)
    allu8 = _every_8bit_value(np.uint8)
    for v in (all8.view(np.uint8), allu8):
        assert all(len(np.unique(v[p::16])) == 256 for p in range(16))
    for scalar in SCALARS:
        ctx.push_raw(all16, capi.IQ_I16, scalar)
        _same(ctx.preproc_read().view(f32), _conj_expected(restate(all16, capi.IQ_I16, scalar)), "int16, scalar %g" % scalar)
        ctx.push_raw(all8, capi.IQ_I8, scalar)
        _same(ctx.preproc_read().view(f32), _conj_expected(restate(all8, capi.IQ_I8, scalar)), "int8, scalar %g" % scalar)
    for tab in (capi.design_u8_table(capi.U8_RTL_SDR), capi.design_u8_table(capi.U8_RTL_TCP), capi.design_u8_table(capi.U8_SPYSERVER, 2.5)):
        ctx.push_raw(allu8, capi.IQ_U8, table=tab)
        _same(ctx.preproc_read().view(f32), _conj_expected(restate(allu8, capi.IQ_U8, table=tab)), "uint8")
    # push_int16 is push_raw {I16, 32768}
    ctx.push_int16(all16)
    _same(ctx.preproc_read().view(f32), _conj_expected(all16.astype(f32) / f32(32768)), "push_int16")
    if pipelined:
        assert ctx.pipeline_stats()["pass_blocks"] == 0, ctx.pipeline_stats()
    ctx.close()


# ---- equivalence: push_raw(raw) == push(restatement(raw)) on everything a context computes ---------------------------------------------------
def _bank_ctx(nv, max_push):
    from sdrplusplus_amd import capi, radio, workloads

    sr = workloads.CFG[3]["sr"]
    ctx = capi.Context(0, max_push=max_push)
    ctx.fft_configure(4096, 4096, 0, capi.design_fft_window(2, 4096))
    start, size = capi.design_waterfall_view(0.0, sr, sr, 4096)
    ctx.fft_set_view(start, size, 600, -120.0, 0.0)
    vids = []
    for mode, if_rate, bw, centre, _ in workloads.vfo_plan(3, nv):
        d, keep = radio.vfo_desc(sr, if_rate, bw, centre, mode)
        vids.append(ctx.vfo_add(d, keep))
    return ctx, vids


def _formats():
    from sdrplusplus_amd import capi

    return {
        "i8": (capi.IQ_I8, np.int8, dict(scalar=128.0)),
        "i16": (capi.IQ_I16, np.int16, dict(scalar=8192.0)),
        "u8": (capi.IQ_U8, np.uint8, dict(table=capi.design_u8_table(capi.U8_RTL_SDR))),
    }


def _raw_signal(n, nv, dtype, seed=5):
    from sdrplusplus_amd import workloads

    x = workloads.synth(3, n, seed=seed, nvfo=nv).view(f32)
    if dtype == np.int16:
        return np.clip(np.round(x * 5000.0), -32768, 32767).astype(np.int16)
    v = np.clip(np.round(x * 80.0), -128, 127)
    return v.astype(np.int8) if dtype == np.int8 else (v + 128).astype(np.uint8)


def _read_ordinary(ctx, vids):
    raw, zo, ix = ctx.fft_read()
    return {"vfo": {v: ctx.vfo_read(v).copy() for v in vids}, "raw": raw, "zoomed": zo, "index": ix, "n_lines": len(raw)}


def _compare(ref, got, what):
    for (va, a), (vb, b) in zip(ref["vfo"].items(), got["vfo"].items()):
        _same(a, b, "%s vfo %d" % (what, va))
    assert ref["n_lines"] == got["n_lines"], (what, ref["n_lines"], got["n_lines"])
    if ref["n_lines"]:
        _same(ref["raw"], got["raw"], what + " raw lines")
        _same(ref["zoomed"], got["zoomed"], what + " zoomed lines")
        assert np.array_equal(ref["index"], got["index"]), what + " palette indices"


@pytest.mark.parametrize("fmt", ["i8", "i16", "u8"])
@pytest.mark.parametrize("mode", ["immediate", "deferred", "pipelined", "group3"])
def test_push_raw_equals_push_of_the_restatement(backend, mode, fmt):
    """Two contexts in the SAME mode, one fed the raw bytes, one the floats numpy makes of them: raw lines, zoomed lines, palette indices and every
    VFO block agree bit for bit — pushed at once, deferred with three staged pushes per pass, pipelined, and three pushes per launch.

    Which loop of the converting copy a block reaches (tick_launch gives the landing job max(1, source bytes / 32768) workgroups of 256 work-items, a
    work-item takes the unrolled trip while 8 x 16 source bytes per work-item remain in front of it; emulator sizes, int8 / uint8 = 2 bytes per sample):
      pipelined  25000 (50000 B, 1 workgroup, 3125 vectors): the unrolled loop, then the single-vector loop; 16667: both again; 10000 and 6000: the
                 single-vector loop alone; 1031 (2062 B): 128 vectors and a 14-byte tail; 7 (14 B): head / tail values only.  int16 doubles the bytes:
                 25000 -> 3 workgroups, unrolled; 7 -> one vector and 12 bytes of tail.
      group3     25000 + 1031 + 10000 = 36031 samples in one copy (int8: 72062 B, 2 workgroups, 4503 vectors: unrolled, then single; int16: 4 workgroups, the same),
                 7 + 16667 + 25000 = 41674 (int8: 83348 B, 2 workgroups, unrolled) — and inside the STAGING slot the second push of that group starts 14 bytes (int8) / 28 bytes (int16)
                 behind a 16-byte boundary.  In deferred mode every staged push is converted by a launch of its own from a source 4 x (samples staged so far)
                 bytes into the raw landing buffer: behind the 7-sample push that is 28 bytes past the boundaries of 16 — a 4-byte head — and the DESTINATION is only
                 8-byte aligned (an odd number of samples in front).
    On the device the sizes are doubled, which moves 10000 -> 20000 (int8: 40000 B) into the unrolled loop as well."""
    type_, dtype, kw = _formats()[fmt]
    nv = 8 if backend == "gpu" else 3
    pushes = [2 * n for n in PUSHES] if backend == "gpu" else PUSHES
    raw = _raw_signal(sum(pushes), nv, dtype)
    flt = restate(raw, type_, **kw).view(np.complex64)
    cap = sum(pushes) if mode == "deferred" else max(pushes) * 2 + 2000
    (ca, va), (cb, vb) = _bank_ctx(nv, cap), _bank_ctx(nv, cap)
    for c in (ca, cb):
        if mode == "deferred":
            c.set_deferred(True)
        elif mode in ("pipelined", "group3"):
            c.set_pipelined(True, 7)
            if mode == "group3":
                c.set_pipeline_group(3)
    pos = 0
    for i, n in enumerate(pushes):
        ca.push(flt[pos:pos + n])
        cb.push_raw(raw[2 * pos:2 * (pos + n)], type_, **kw)
        pos += n
        if mode == "immediate" or (mode == "deferred" and (i % 3 == 2 or i == len(pushes) - 1)):
            _compare(_read_ordinary(ca, va), _read_ordinary(cb, vb), "%s push %d" % (mode, i))
    if mode in ("pipelined", "group3"):
        for t in range(1, len(pushes) + 1):
            _compare(ca.result_wait(t), cb.result_wait(t), "%s block %d" % (mode, t))
            ca.result_release(t)
            cb.result_release(t)
        st, gs = cb.pipeline_stats(), cb.pipeline_group_stats()
        assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(pushes), st
        assert gs["largest"] == (3 if mode == "group3" else 0), gs
    ca.close()
    cb.close()


def test_a_group_is_cut_where_the_format_changes(backend):
    """set_pipeline_group(4): I8 / I8 / I16 / I16 with another scalar / U8 with table A / U8 with table B — a launch converts with ONE format, so only the first two
    pushes share one; every push has its own ticket and the results of the block-by-block ordinary pass over the restated floats."""
    from sdrplusplus_amd import capi

    nv = 8 if backend == "gpu" else 3
    n = 12000 if backend == "gpu" else 6000
    ta, tb = capi.design_u8_table(capi.U8_RTL_SDR), capi.design_u8_table(capi.U8_SPYSERVER, 2.5)
    plan = [(capi.IQ_I8, np.int8, dict(scalar=128.0)), (capi.IQ_I8, np.int8, dict(scalar=128.0)), (capi.IQ_I16, np.int16, dict(scalar=32768.0)),
            (capi.IQ_I16, np.int16, dict(scalar=8192.0)), (capi.IQ_U8, np.uint8, dict(table=ta)), (capi.IQ_U8, np.uint8, dict(table=tb))]
    (ca, va), (cb, vb) = _bank_ctx(nv, 4 * n), _bank_ctx(nv, 4 * n)
    cb.set_pipelined(True, 7)
    cb.set_pipeline_group(4)
    refs = []
    for i, (type_, dtype, kw) in enumerate(plan):
        raw = _raw_signal(n, nv, dtype, seed=20 + i)
        ca.push(restate(raw, type_, **kw).view(np.complex64))
        refs.append(_read_ordinary(ca, va))
        cb.push_raw(raw, type_, **kw)
        assert cb.ticket() == i + 1
    for t, ref in enumerate(refs, start=1):
        _compare(ref, cb.result_wait(t), "block %d" % t)
        cb.result_release(t)
    gs, st = cb.pipeline_group_stats(), cb.pipeline_stats()
    assert gs["groups"] == 5 and gs["multi_groups"] == 1 and gs["multi_blocks"] == 2 and gs["largest"] == 2 and gs["held"] == 0, gs
    assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(plan), st
    ca.close()
    cb.close()


# ---- server frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True], ids=["immediate", "pipelined"])
def test_server_frames_as_the_reference_decompresses_them(backend, pipelined):
    """Every recorded frame through sdrpp_push_frame: the count SampleStreamDecompressor::process returned, and behind the conjugating chain the floats
    it wrote.  An unknown type, a header alone and data without a whole sample give 0 and push nothing; 5 bytes are no frame."""
    from sdrplusplus_amd import capi

    g = np.load(GOLDEN)
    ctx = _conj_ctx(2048, pipelined)
    pushed = 0
    for name in g["names"]:
        n = int(g[name + "_count"][0])
        got = ctx.push_frame(g[name + "_frame"].tobytes())
        assert got == n, (name, got, n)
        if n:
            pushed += 1
            _same(ctx.preproc_read().view(f32), _conj_expected(g[name + "_out"]), name)
        if pipelined:
            assert ctx.ticket() == pushed, (name, ctx.ticket(), pushed)
    assert pushed >= 10 and pushed < len(g["names"])
    with pytest.raises(capi.SdrppError) as e:
        ctx.push_frame(b"\x00\x00\x01\x00\x00")
    assert e.value.code == -2
    if pipelined:
        assert ctx.ticket() == pushed and ctx.pipeline_stats()["pass_blocks"] == 0
    ctx.close()


# ---- argument rules --------------------------------------------------------------------------------------------------------------------------
def test_push_raw_argument_errors(backend):
    from sdrplusplus_amd import capi

    ctx = capi.Context(0, max_push=1000)
    x8, x16 = np.zeros(64, np.int8), np.zeros(64, np.int16)
    bad = [lambda s=s: ctx.push_raw(x8, capi.IQ_I8, s) for s in (0.0, float("inf"), float("-inf"), float("nan"))]
    bad += [lambda s=s: ctx.push_raw(x16, capi.IQ_I16, s) for s in (0.0, float("inf"), float("nan"))]
    bad += [lambda: ctx.push_raw(x8.view(np.uint8), capi.IQ_U8), lambda: ctx.push_raw(x8, 7, 1.0), lambda: ctx.push_raw(x8, -1, 1.0),
            lambda: ctx.push_raw(np.zeros(2002, np.int8), capi.IQ_I8, 128.0)]
    for f in bad:
        with pytest.raises(capi.SdrppError) as e:
            f()
        assert e.value.code == -2, str(e.value)
    assert ctx.L.sdrpp_push_raw(ctx.h, x8.ctypes.data, 32, None) == -2
    ctx.push_raw(x8, capi.IQ_I8, 128.0)  # (and the context still works)
    ctx.push_raw(x8.view(np.uint8), capi.IQ_U8, table=capi.design_u8_table(capi.U8_RTL_TCP))
    ctx.close()
