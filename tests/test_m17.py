"""The M17 frame branch on the device: the symbol branch with M17's description (sdrpp_design_m17) and the framer behind it (sdrpp_vfo_set_framer) — 4FSK slicer,
sync search at every bit offset, descrambled and de-interleaved frames: M17Slice4FSK and M17FrameDemux of decoder_modules/m17_decoder/src/m17dsp.h.

YARDSTICKS: tests/golden/m17_ref.npz, recorded from the compiled reference by tests/golden/make_m17_golden.py, and tests/m17_ref.py, this project's restatement of
slicer and demux, which test 1 pins to the fixture.  The fixture's IF inputs reach the branch unchanged through a VFO that does nothing (14.4 kS/s in and out,
bandwidth = rate, offset 0); every such test first checks that the IF stream the device delivers is its input bit for bit.

BOUNDS against the fixture: symbol counts per block equal; soft values within the pager's bar, max(1e-5 * RMS, 4 x the recorded spread) per symbol and over the
case; ALL dibits equal — the recorder keeps every settled soft value 10 bars away from a decision level, and the 13 start-up symbols of a fresh chain are sums of a
few products whose signs both sides share; the frame counts per block and every record byte for byte.  Everywhere else the device is compared with the
restatement fed with the device's own soft values, or with itself along another path: bit for bit.

EXACT-SYMBOL ROWS: a description of a 1-tap shape [1], a 1 x 1 bank [1], omega 4, both gains 0 and inv_deviation 1 turns phase steps of +-1 and +-1/3 rad at every
fourth sample into exactly those soft values (to the discriminator's 3e-7), so any dibit stream can be built bit by bit."""
import ctypes as C
import os

import numpy as np
import pytest

import m17_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "m17_ref.npz")
RATE = 14400.0
NOT_FOUND, INVALID, UNSUPPORTED = -6, -2, -5
CHUNK_BITS = 2048  # SDRPP_FRAME_CHUNK_BITS (vfo_frame_kernels.h): new bits per chunk of the framer's LDS words
PACK = 64          # SDRPP_SYM_PACK: lanes of a loop job
STRIDE = 48
LEVEL = {(0, 1): 1.0, (0, 0): 1.0 / 3.0, (1, 0): -1.0 / 3.0, (1, 1): -1.0}
CASES = ["aligned_clean", "aligned_noise", "aligned_noisy", "delay_a", "delay_b", "cuts", "reset"]


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype.itemsize == 4 else np.array_equal(a, b)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case_input(z, name):
    return (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)


def make_ctx(max_push=16384):
    from sdrplusplus_amd import capi

    return capi.Context(0, max_push=max_push)


def add_transparent(ctx, mode="RAW"):
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, mode)
    return ctx.vfo_add(d, keep)


def exact_desc(inv_deviation=1.0):
    """one symbol per four samples, soft value = the phase step at the symbol's sample (times inv_deviation)"""
    from sdrplusplus_amd import capi

    taps, bank = np.ones(1, np.float32), np.ones(1, np.float32)
    d = capi.SymDesc()
    d.inv_deviation, d.shape_ntaps, d.shape_taps = inv_deviation, 1, taps.ctypes.data_as(capi.c_float_p)
    d.omega, d.mu_gain, d.omega_gain, d.min_omega, d.max_omega = 4.0, 0.0, 0.0, 3.5, 4.5
    d.interp_phases, d.interp_ntaps, d.interp_bank = 1, 1, bank.ctypes.data_as(capi.c_float_p)
    return d, [taps, bank]


def m17_frame_desc():
    from sdrplusplus_amd import radio

    _, fd, keep = radio.m17_desc(RATE)
    return fd, keep


def add_exact(ctx, framer=True, inv_deviation=1.0, enabled=True):
    vid = add_transparent(ctx)
    sd, sk = exact_desc(inv_deviation)
    ctx.vfo_set_symbols(vid, sd, True, sk)
    if framer:
        fd, fk = m17_frame_desc()
        ctx.vfo_set_framer(vid, fd, enabled, fk)
    return vid


def iq_of(bits):
    """a dibit stream as IQ: the symbol's level as the phase step at every fourth sample"""
    bits = np.asarray(bits, np.uint8).reshape(-1, 2)
    inc = np.zeros(4 * len(bits))
    inc[0::4] = [LEVEL[(int(a), int(b))] for a, b in bits]
    return np.exp(1j * np.cumsum(inc)).astype(np.complex64)


def sync_bits(t):
    return [(R.SYNC[t] >> (15 - b)) & 1 for b in range(16)]


def frame_bits(r, t, payload=None):
    return np.concatenate([sync_bits(t), r.integers(0, 2, 368) if payload is None else payload]).astype(np.uint8)


def even(bits):
    bits = np.asarray(bits, np.uint8)
    return np.append(bits, 0).astype(np.uint8) if len(bits) % 2 else bits


def schedule(n, sizes):
    out, pos, k = [], 0, 0
    while pos < n:
        s = min(sizes[k % len(sizes)], n - pos)
        out.append(s)
        pos += s
        k += 1
    return out


def run_cut(ctx, vids, x, cut):
    """push x in the pushes of `cut` -> per VFO the list of (soft, records) per push"""
    out, pos = {v: [] for v in vids}, 0
    for s in cut:
        ctx.push(x[pos:pos + s])
        for v in vids:
            out[v].append((ctx.vfo_sym_read(v)[0], ctx.vfo_frame_read(v)))
        pos += s
    return out


def expect(parts, demux=None):
    """the restatement over the device's own soft values, push by push -> the records of every push"""
    demux = demux or R.Demux()
    return [R.records(demux.run(R.slice4fsk(soft))) for soft, _ in parts]


def check_parts(parts, what, demux=None):
    exp = expect(parts, demux)
    for k, ((_, recs), e) in enumerate(zip(parts, exp)):
        assert recs.shape == e.shape and np.array_equal(recs, e), "%s: push %d delivers %d frames, the restatement %d%s" % (what, k, len(recs), len(e), "" if len(recs) != len(e) else ", bytes differ")
    return exp


def run_pipelined(ctx, vids, x, cut, group, flags=None):
    """the same pushes in pipelined mode with launch groups of `group`, result flag 512 alone -> per VFO the list of records per push"""
    from sdrplusplus_amd import capi

    ctx.set_pipelined(True, capi.RESULT_FRAMES if flags is None else flags)
    ctx.set_pipeline_group(group)
    pos = 0
    for s in cut:
        ctx.push(x[pos:pos + s])
        pos += s
    out = {v: [] for v in vids}
    for i in range(len(cut)):
        ctx.result_wait(i + 1)
        for v in vids:
            out[v].append(ctx.result_frames(i + 1, v))
        ctx.result_release(i + 1)
    ctx.set_pipelined(False)
    return out


# ---- 1. the restatement against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(golden, name):
    """reference soft values in, block by block with the fixture's resets: every recorded dibit and every frame (type, block, 368 positions) out"""
    z = golden
    soft, counts, fresh = z[name + "_soft"], z[name + "_counts"], z[name + "_reset"]
    assert np.array_equal(R.slice4fsk(soft), z[name + "_dibits"])
    dm, pos, frames = R.Demux(), 0, []
    for b, n in enumerate(counts):
        if b in fresh:
            dm = R.Demux()
        if n > 0:  # (the reference's GFSK swaps nothing out of a block without symbols: the slicer and the demux do not run)
            frames += [(t, b, f) for t, f in dm.run(R.slice4fsk(soft[pos:pos + n]))]
        pos += int(n)
    assert [f[0] for f in frames] == list(z[name + "_ftype"]) and [f[1] for f in frames] == list(z[name + "_fblock"]), name
    assert np.array_equal(np.asarray([f[2] for f in frames], np.uint8).reshape(-1, 368), z[name + "_frames"]), name
    assert all({0: 0, 1: 2, 2: 3}[t] == s for t, s in zip(z[name + "_ftype"], z[name + "_fstream"]))


def test_tables_equal_the_reference(golden):
    z = golden
    assert np.array_equal(R.SCRAMBLE, z["scramble"]) and np.array_equal(R.INTERLEAVE, z["interleave"])
    assert np.array_equal(np.asarray([[(w >> (15 - b)) & 1 for b in range(16)] for w in R.SYNC], np.uint8), z["sync"])
    assert sorted(R.INTERLEAVE) == list(range(368))


# ---- 2. design -----------------------------------------------------------------------------------------------------------------------------------
def test_design_equals_the_reference_bit_for_bit(golden):
    """sdrpp_design_m17 leaves the scalars GFSK::init leaves in its blocks, the 31 taps and the three tables of the reference, bit for bit; sizes; errors"""
    from sdrplusplus_amd import capi, radio

    z = golden
    sd, fd, keep = radio.m17_desc(RATE)
    name = CASES[0]
    mine = np.array([sd.omega, sd.min_omega, sd.max_omega, sd.mu_gain, sd.omega_gain, sd.inv_deviation], np.float32)
    assert bits_equal(mine, z[name + "_pcl"]), (mine, z[name + "_pcl"])
    assert (sd.shape_ntaps, sd.interp_phases, sd.interp_ntaps) == (31, 128, 8)
    taps, bank, scr, il = keep
    assert bits_equal(taps, z[name + "_taps"]) and bits_equal(bank, capi.design_mm_interp(128, 8))
    assert np.array_equal(scr, z["scramble"]) and np.array_equal(il, z["interleave"]) and scr.dtype == np.uint8 and il.dtype == np.uint16
    assert fd.n_sync == 3 and fd.frame_bits == 368 and list(fd.sync)[:3] == [int("".join(str(b) for b in row), 2) for row in z["sync"]] == [0x55F7, 0xFF5D, 0x75FF]
    assert np.float32(fd.high_cut).tobytes() == R.HIGH_CUT.tobytes()
    L = capi.load()
    assert L.sdrpp_abi_sizeof_frame_desc() == C.sizeof(capi.FrameDesc) == 40
    assert capi.frame_record_stride(368) == STRIDE and capi.frame_record_stride(8) == 4 and capi.frame_record_stride(16) == 4 and capi.frame_record_stride(24) == 8
    assert L.sdrpp_frame_record_stride(12) == INVALID and L.sdrpp_frame_record_stride(1032) == INVALID
    s2, f2 = capi.SymDesc(), capi.FrameDesc()
    t, a, b = np.empty(31, np.float32), np.empty(368, np.uint8), np.empty(368, np.uint16)
    args = lambda rate=RATE, sym=C.byref(s2), tp=t.ctypes.data_as(capi.c_float_p), mx=31, fr=C.byref(f2), sc=a.ctypes.data_as(C.POINTER(C.c_uint8)), ilv=b.ctypes.data_as(C.POINTER(C.c_uint16)): (rate, sym, tp, mx, fr, sc, ilv)
    assert L.sdrpp_design_m17(*args()) == 0
    for bad in (args(rate=0.0), args(rate=float("nan")), args(rate=float("inf")), args(rate=-1.0), args(sym=None), args(tp=None), args(mx=30), args(fr=None), args(sc=None), args(ilv=None)):
        assert L.sdrpp_design_m17(*bad) == INVALID


# ---- 3. against the reference fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_against_the_reference_fixture(backend, golden, name):
    """The fixture's IF input through the transparent VFO with the fixture's block schedule (both descriptions attached anew where the fixture starts a fresh chain)."""
    from sdrplusplus_amd import radio

    z = golden
    x, cut, fresh = case_input(z, name), z[name + "_cut"], z[name + "_reset"]
    ref_soft, ref_counts = z[name + "_soft"], z[name + "_counts"]
    ctx = make_ctx(4096)
    vid = add_transparent(ctx)
    sd, fd, keep = radio.m17_desc(RATE)
    ctx.vfo_set_symbols(vid, sd, True, keep)
    ctx.vfo_set_framer(vid, fd, True, keep)
    softs, recs, pos = [], [], 0
    for b, n in enumerate(cut):
        if b in fresh:
            ctx.vfo_set_symbols(vid, None)
            ctx.vfo_set_symbols(vid, sd, True, keep)
            ctx.vfo_set_framer(vid, fd, True, keep)
        ctx.push(x[pos:pos + n])
        assert bits_equal(ctx.vfo_read_if(vid).view(np.float32), x[pos:pos + n].view(np.float32)), "the VFO is not transparent"
        softs.append(ctx.vfo_sym_read(vid)[0])
        recs.append(ctx.vfo_frame_read(vid))
        assert ctx.vfo_frame_count(vid) == len(recs[-1])
        pos += int(n)
    ctx.close()
    soft = np.concatenate(softs)
    assert [len(s) for s in softs] == list(ref_counts), name                                               # (a) symbols per block
    err = soft.astype(np.float64) - ref_soft.astype(np.float64)                                            # (b) soft values inside the pager's bar
    Rm = rms(ref_soft)
    bar_each = np.maximum(1e-5 * Rm, 4.0 * z[name + "_dev_max"].astype(np.float64))
    bar_rms = max(1e-5 * Rm, 4.0 * float(z[name + "_dev_rms"]))
    print("[m17] %s (%s): %d symbols, soft error max %.3g (bar %.3g .. %.3g) rms %.3g (bar %.3g), reference RMS %.3f, %d frames" % (
        name, backend, len(soft), np.abs(err).max(), bar_each.min(), bar_each.max(), rms(err), bar_rms, Rm, sum(len(r) for r in recs)))
    assert np.all(np.abs(err) <= bar_each), (name, float(np.abs(err).max()))
    assert rms(err) <= bar_rms, (name, rms(err))
    start = z[name + "_settled"] == 0                                                                      # (c) ALL dibits; the start-up symbols' rest on signs the
    assert start.sum() == 13 * (1 + len(fresh)) and np.all(z[name + "_startup_sign"][~start] == 0)         #     recorder found stable over nine runs: the device shares them
    assert np.array_equal(np.where(soft[start] < np.float32(0.0), -1, 1), z[name + "_startup_sign"][start]), name
    assert np.array_equal(R.slice4fsk(soft), z[name + "_dibits"]), name
    want = [R.records([(int(t), f) for t, f, fb in zip(z[name + "_ftype"], z[name + "_frames"], z[name + "_fblock"]) if fb == b]) for b in range(len(cut))]
    assert [len(r) for r in recs] == [len(w) for w in want], name                                          # (d) frames per block
    for b, (r, w) in enumerate(zip(recs, want)):                                                           # (e) every record byte for byte
        assert r.shape == w.shape == (len(w), STRIDE) and np.array_equal(r, w), (name, b)


# ---- 4. exact-symbol rows --------------------------------------------------------------------------------------------------------------------
def rows_stream(seed=3):
    """filler of 7 bits (the first sync word at an ODD bit offset); a link-setup frame whose payload holds two sync words; back to back a stream frame; ONE bit; a
    packet frame (a sync word one bit behind a frame); filler; an even-aligned stream frame; filler -> (bits, per frame the index of the bit whose ARRIVAL completes
    it: the demux consumes a bit when the sixteenth behind it has arrived, so that is the frame's last bit + 16)"""
    r = np.random.default_rng(seed)
    pay = r.integers(0, 2, 368).astype(np.uint8)
    pay[40:56] = sync_bits(1)
    pay[201:217] = sync_bits(2)
    parts = [r.integers(0, 2, 7), frame_bits(r, 0, pay), frame_bits(r, 1), [1], frame_bits(r, 2), r.integers(0, 2, 21), frame_bits(r, 1), r.integers(0, 2, 40)]
    ends, pos = [], 0
    for p in parts:
        pos += len(p)
        if len(p) == 384:
            ends.append(pos - 1 + 16)
    return even(np.concatenate(parts)), ends


def test_rows_every_edge_of_the_walk(backend):
    """odd offsets, sync words inside a payload, frames back to back, a sync word one bit behind a frame, all three types: one push, then the same stream with a frame
    that ends on a push's last bit and one that ends on the next push's first bit"""
    bits, ends = rows_stream()
    x = iq_of(bits)
    ctx = make_ctx()
    vid = add_exact(ctx)
    parts = run_cut(ctx, [vid], x, [len(x)])[vid]
    assert np.array_equal(R.slice4fsk(parts[0][0]), bits), "the exact-symbol row does not deliver the dibits it was built from"
    exp = check_parts(parts, "one push")
    assert [int(r[0]) for r in exp[0]] == [0, 1, 2, 1] and exp[0][0, 1] == 0
    assert ends[0] % 2 == 0 and ends[2] % 2 == 1   # the first frame completes with the first bit of a dibit, the third with the second
    # symbol s starts in the push that holds sample 4 s: a push that ends BEHIND that sample has the symbol, one that ends AT it hands it to the next
    cut_last = [4 * (ends[2] // 2) + 1, len(x) - (4 * (ends[2] // 2) + 1)]    # the third frame's last bit is the first push's last bit
    cut_first = [4 * (ends[0] // 2), len(x) - 4 * (ends[0] // 2)]            # the first frame's last bit is the second push's first bit
    for cut, want in ((cut_last, [3, 1]), (cut_first, [0, 4])):
        ctx.vfo_set_symbols(vid, None)
        vid2 = vid
        sd, sk = exact_desc()
        ctx.vfo_set_symbols(vid2, sd, True, sk)
        fd, fk = m17_frame_desc()
        ctx.vfo_set_framer(vid2, fd, True, fk)
        parts = run_cut(ctx, [vid2], x, cut)[vid2]
        check_parts(parts, str(cut))
        assert [len(p[1]) for p in parts] == want, (cut, [len(p[1]) for p in parts])
        assert 2 * len(parts[0][0]) - 1 == (ends[2] if want == [3, 1] else ends[0] - 1)
    ctx.close()


def test_rows_pushes_of_one_symbol_and_less(backend):
    """pushes of one symbol and pushes too short for any symbol through whole sync words and frames"""
    bits, _ = rows_stream(seed=4)
    bits = bits[:7 + 384 + 384 + 1 + 384 + 18]
    x = iq_of(bits)
    ctx = make_ctx()
    vid = add_exact(ctx)
    one = run_cut(ctx, [vid], x, [len(x)])[vid]
    whole = check_parts(one, "one push")[0]
    assert len(whole) == 3
    for sizes in ([4], [1, 2, 3, 4, 1]):
        vid = add_exact(ctx)
        cut = schedule(len(x), sizes)
        parts = run_cut(ctx, [vid], x, cut)[vid]
        assert max(len(p[0]) for p in parts) == 1 and (sizes == [4] or min(len(p[0]) for p in parts) == 0)
        check_parts(parts, str(sizes))
        assert np.array_equal(np.concatenate([p[1] for p in parts]), whole), sizes
    ctx.close()


@pytest.mark.parametrize("group", [1, 2, 8, 32])
def test_rows_launch_groups_keep_every_pushs_own_count(backend, group):
    """pipelined with result flag 512 alone, launch groups of 1, 2, 8 and 32: every push's own count and slice equal the ordinary pushes'"""
    bits, _ = rows_stream(seed=5)
    x = iq_of(bits)
    cut = schedule(len(x), [97, 64, 3, 200, 1, 131])
    ctx = make_ctx()
    vid = add_exact(ctx)
    parts = run_cut(ctx, [vid], x, cut)[vid]
    exp = check_parts(parts, "ordinary")
    assert sum(len(e) for e in exp) == 4 and max(len(e) for e in exp) == 1
    vid2 = add_exact(ctx)
    ctx.vfo_remove(vid)
    got = run_pipelined(ctx, [vid2], x, cut, group)[vid2]
    ctx.close()
    assert [len(g) for g in got] == [len(e) for e in exp], group
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and np.array_equal(g, e), (group, k)


def test_rows_more_than_one_chunk_of_lds_words(backend):
    """one push of more than two chunks of bits, a frame across each chunk edge, and the same stream cut at the edges"""
    r = np.random.default_rng(6)
    parts = [r.integers(0, 2, CHUNK_BITS - 200), frame_bits(r, 1), r.integers(0, 2, CHUNK_BITS - 384 - 9), frame_bits(r, 2), r.integers(0, 2, 300), frame_bits(r, 0), r.integers(0, 2, 50)]
    bits = even(np.concatenate(parts))
    assert len(bits) > 2 * CHUNK_BITS
    x = iq_of(bits)
    ctx = make_ctx()
    vid = add_exact(ctx)
    one = run_cut(ctx, [vid], x, [len(x)])[vid]
    assert np.array_equal(R.slice4fsk(one[0][0]), bits)
    whole = check_parts(one, "one push")[0]
    assert [int(t) for t in whole[:, 0]][-3:] == [1, 2, 0]
    vid = add_exact(ctx)
    cut = schedule(len(x), [2 * CHUNK_BITS, 2 * CHUNK_BITS + 4, 2 * CHUNK_BITS - 4])  # (four samples per symbol, two bits per symbol)
    parts = run_cut(ctx, [vid], x, cut)[vid]
    check_parts(parts, "cut at the chunk edges")
    ctx.close()
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole)


def test_rows_other_descriptions(backend):
    """a general block: one sync word and 8-bit frames, four sync words and 1024-bit frames, another threshold — against the restatement with the same tables"""
    from sdrplusplus_amd import capi

    r = np.random.default_rng(7)
    ctx = make_ctx()
    for nbits, sync, cutv in ((8, (0xA5C3,), 0.5), (1024, (0x1234, 0xFEDC, 0x0F0F, 0x8001), 0.9), (40, (0xFFFF, 0x0001), 0.2)):
        scr, il = r.integers(0, 2, nbits).astype(np.uint8), r.permutation(nbits).astype(np.uint16)
        fd = capi.FrameDesc()
        fd.high_cut, fd.n_sync, fd.frame_bits = cutv, len(sync), nbits
        for k, w in enumerate(sync):
            fd.sync[k] = w
        fd.scramble, fd.interleave = scr.ctypes.data_as(C.POINTER(C.c_uint8)), il.ctypes.data_as(C.POINTER(C.c_uint16))
        parts = [r.integers(0, 2, 5)]
        for k in range(6):
            w = sync[k % len(sync)]
            parts += [[(w >> (15 - b)) & 1 for b in range(16)], r.integers(0, 2, nbits), r.integers(0, 2, int(r.integers(0, 4)))]
        bits = even(np.concatenate(parts))
        vid = add_exact(ctx, framer=False)
        ctx.vfo_set_framer(vid, fd, True)
        x, pos, dm, total = iq_of(bits), 0, R.Demux(sync, scr, il), 0
        stride = capi.frame_record_stride(nbits)
        for s in schedule(len(x), [301, 7, 1024]):
            ctx.push(x[pos:pos + s])
            soft = ctx.vfo_sym_read(vid)[0]
            got = ctx.vfo_frame_read(vid, nbits)
            exp = R.records(dm.run(R.slice4fsk(soft, np.float32(cutv))), nbits)
            assert exp.shape[1] == stride and got.shape == exp.shape and np.array_equal(got, exp), (nbits, pos)
            total += len(exp)
            pos += s
        assert total >= 3, (nbits, total)
    ctx.close()


# ---- 5. banks ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 2, 64, 65])
def test_banks_across_the_loops_pack_edge(backend, nch):
    """1, 2, 64 and 65 channels (the loop packs 64 to a job; the framer is a job per channel): channels alternate between the stream and its inversion, every
    channel against the restatement over its own soft values; the tables exist once"""
    bits, _ = rows_stream(seed=8)
    x = iq_of(bits)
    ctx = make_ctx()
    vids = [add_exact(ctx, inv_deviation=1.0 if k % 2 == 0 else -1.0) for k in range(nch)]
    assert ctx.frame_table_count() == 1
    out = run_cut(ctx, vids, x, schedule(len(x), [700, 1, 1300]))
    for k, v in enumerate(vids):
        exp = check_parts(out[v], "channel %d of %d" % (k, nch))
        assert sum(len(e) for e in exp) == (4 if k % 2 == 0 else 0), (k, nch)
        assert np.array_equal(R.slice4fsk(np.concatenate([p[0] for p in out[v]]))[0::2], bits[0::2] ^ (k % 2))
    for v in vids:
        ctx.vfo_remove(v)
    assert ctx.frame_table_count() == 0
    ctx.close()


def test_banks_mixed_and_every_other_output_unchanged(backend):
    """framer channels beside pager channels, a branch without a framer and plain VFOs: with and without the framers every other output is the same bit for bit"""
    from sdrplusplus_amd import radio

    bits, _ = rows_stream(seed=9)
    x = iq_of(bits)
    cut = schedule(len(x), [900, 333])
    runs = []
    for with_framer in (False, True):
        ctx = make_ctx()
        a = add_exact(ctx, framer=with_framer)
        nfm = add_transparent(ctx, "NFM")
        p = add_transparent(ctx)
        pd, pk = radio.pager_desc(RATE, 1200.0)
        ctx.vfo_set_symbols(p, pd, True, pk)
        b = add_exact(ctx, framer=with_framer, inv_deviation=-1.0)
        raw = add_transparent(ctx)
        c = add_exact(ctx, framer=False)
        outs, pos = [], 0
        for s in cut:
            ctx.push(x[pos:pos + s])
            row = [ctx.vfo_read_if(v).view(np.float32).copy() for v in (a, nfm, p, b, raw, c)] + [ctx.vfo_read(nfm).copy()]
            for v in (a, p, b, c):
                row += list(ctx.vfo_sym_read(v))
            if with_framer:
                row.append([ctx.vfo_frame_read(v) for v in (a, b)])
            outs.append(row)
            pos += s
        if with_framer:
            for k in range(2):
                check_parts([(row[7 + (0 if k == 0 else 4)], row[-1][k]) for row in outs], "mixed bank, framer %d" % k)
            assert sum(len(row[-1][0]) for row in outs) == 4
            lib = ctx.L
            assert lib.sdrpp_vfo_frame_count(ctx.h, c) == INVALID and lib.sdrpp_vfo_frame_count(ctx.h, raw) == INVALID
        ctx.close()
        runs.append(outs)
    for r0, r1 in zip(*runs):
        assert len(r1) == len(r0) + 1
        for k, (u, w) in enumerate(zip(r0, r1)):
            assert bits_equal(u, w), k


# ---- 6. control --------------------------------------------------------------------------------------------------------------------------------
def control_stream():
    r = np.random.default_rng(10)
    bits = even(np.concatenate([r.integers(0, 2, 30), frame_bits(r, 0), r.integers(0, 2, 10), frame_bits(r, 1), r.integers(0, 2, 12), frame_bits(r, 2), r.integers(0, 2, 44)]))
    return bits, iq_of(bits)


def test_control_freeze_and_continue(backend):
    """switched off in the middle of a frame — the framer alone, then the branch — the state freezes; switched on it continues: the output equals a run over
    the pushes it was switched on for"""
    bits, x = control_stream()
    a, b, c, d = 400, 1000, 1600, 2100  # sample positions inside the first, the second and the third frame
    ctx = make_ctx()
    vid = add_exact(ctx)
    fd, fk = m17_frame_desc()
    sd, sk = exact_desc()
    ctx.push(x[:a])
    p0 = (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))
    ctx.vfo_set_framer(vid, fd, False, fk)
    ctx.push(x[a:b])                                   # the branch runs on, the framer does not
    skipped = ctx.vfo_sym_read(vid)[0]
    assert len(skipped) == (b - a) // 4 and ctx.vfo_frame_count(vid) == 0 and len(ctx.vfo_frame_read(vid)) == 0
    ctx.vfo_set_framer(vid, fd, True, fk)
    ctx.push(x[b:c])
    p1 = (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))
    ctx.vfo_set_symbols(vid, sd, False, sk)            # now the branch: nothing runs
    ctx.push(x[c:d])
    assert ctx.vfo_frame_count(vid) == 0 and ctx.vfo_sym_count(vid) == 0
    ctx.vfo_set_symbols(vid, sd, True, sk)
    ctx.push(x[d:])
    p2 = (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))
    ctx.close()
    check_parts([p0, p1, p2], "freeze and continue")   # ONE restatement over the three pushes the framer saw
    assert len(p0[1]) == 0 and len(p1[1]) + len(p2[1]) >= 1   # (the frame the first switch fell into is completed with the bits behind the gap, as the reference would)
    dm = R.Demux()
    dm.run(R.slice4fsk(p0[0]))
    assert dm.detect                                    # (the switch fell inside a frame)


def test_control_new_description_reset_detach_and_vfo_reset(backend):
    from sdrplusplus_amd import capi

    bits, x = control_stream()
    a = 400
    ctx = make_ctx()
    fd, fk = m17_frame_desc()
    sd, sk = exact_desc()
    lib = ctx.L
    # (a) sdrpp_vfo_framer_reset inside a frame: the rest of the stream is decoded from the cleared state
    vid = add_exact(ctx)
    ctx.push(x[:a])
    ctx.vfo_framer_reset(vid)
    ctx.push(x[a:])
    check_parts([(ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))], "framer reset")
    assert ctx.vfo_frame_count(vid) == 2
    # (b) another description inside a frame starts cleared as well; the same description does not
    vid = add_exact(ctx)
    ctx.push(x[:a])
    fd2, fk2 = m17_frame_desc()
    fd2.high_cut = 0.6
    ctx.vfo_set_framer(vid, fd2, True, fk2)
    ctx.push(x[a:])
    soft = ctx.vfo_sym_read(vid)[0]
    exp = R.records(R.Demux().run(R.slice4fsk(soft, np.float32(0.6))))
    assert len(exp) == 2 and np.array_equal(ctx.vfo_frame_read(vid), exp)
    vid = add_exact(ctx)
    ctx.push(x[:a])
    p0 = (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))
    ctx.vfo_set_framer(vid, fd, True, fk)
    ctx.push(x[a:])
    exp = check_parts([p0, (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))], "the same description")
    assert sum(len(e) for e in exp) == 3
    # (c) sdrpp_vfo_reset leaves the framer alone, as it leaves the loop
    vid = add_exact(ctx)
    ctx.push(x[:a])
    p0 = (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))
    ctx.vfo_reset(vid)
    ctx.push(x[a:])
    exp = check_parts([p0, (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))], "sdrpp_vfo_reset")
    assert sum(len(e) for e in exp) >= 2
    # (c2) ANOTHER branch description replaces the branch, and the framer goes with it: the calls say so (SDRPP_ERR_INVALID) until it is attached again
    sd2, sk2 = exact_desc(-1.0)
    ctx.vfo_set_symbols(vid, sd2, True, sk2)
    assert lib.sdrpp_vfo_frame_count(ctx.h, vid) == INVALID and lib.sdrpp_vfo_framer_reset(ctx.h, vid) == INVALID and ctx.vfo_sym_count(vid) == 0
    ctx.vfo_set_framer(vid, fd, True, fk)
    assert ctx.vfo_frame_count(vid) == 0
    # (d) detaching the branch detaches the framer; the framer's own detach leaves the branch
    tabs = ctx.frame_table_count()
    ctx.vfo_set_symbols(vid, None)
    assert lib.sdrpp_vfo_frame_count(ctx.h, vid) == INVALID and lib.sdrpp_vfo_framer_reset(ctx.h, vid) == INVALID
    assert lib.sdrpp_vfo_set_framer(ctx.h, vid, C.byref(fd), 1) == INVALID      # no branch
    ctx.vfo_set_symbols(vid, sd, True, sk)
    ctx.vfo_set_framer(vid, fd, True, fk)
    ctx.vfo_set_framer(vid, None)
    assert lib.sdrpp_vfo_frame_count(ctx.h, vid) == INVALID and ctx.vfo_sym_count(vid) == 0
    assert ctx.frame_table_count() == tabs
    ctx.close()


def test_control_replace_moves_the_framer_with_the_branch(backend):
    """sdrpp_vfo_replace with keep & 2 inside a frame: the new handle continues (the same stream capacity) — without it the new handle has neither"""
    from sdrplusplus_amd import radio

    bits, x = control_stream()
    a = 400
    ctx = make_ctx()
    vid = add_exact(ctx)
    ctx.push(x[:a])
    p0 = (ctx.vfo_sym_read(vid)[0], ctx.vfo_frame_read(vid))
    d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
    nid = ctx.vfo_replace(vid, d, 2, keep)
    ctx.push(x[a:])
    exp = check_parts([p0, (ctx.vfo_sym_read(nid)[0], ctx.vfo_frame_read(nid))], "replace, keep & 2")
    assert sum(len(e) for e in exp) == 3
    nid2 = ctx.vfo_replace(nid, d, 0, keep)
    assert ctx.L.sdrpp_vfo_frame_count(ctx.h, nid2) == INVALID and ctx.L.sdrpp_vfo_sym_count(ctx.h, nid2) == INVALID
    assert ctx.frame_table_count() == 0
    ctx.close()


def test_control_replace_to_another_capacity_attaches_the_framer_afresh(backend):
    """sdrpp_vfo_replace with keep & 2 inside a frame to a handle with another stream capacity (half the IF rate): branch and framer are attached afresh from the
    descriptions the old handle held — the framer starts CLEARED (the restatement from a fresh demux over the new handle's own soft values; a framer that had kept
    its open frame would complete it 384 steps on) — and the tables still exist once, then not at all"""
    from sdrplusplus_amd import radio

    bits, x = control_stream()
    a = 400
    ctx = make_ctx()
    vid = add_exact(ctx)
    ctx.push(x[:a])
    dm = R.Demux()
    dm.run(R.slice4fsk(ctx.vfo_sym_read(vid)[0]))
    assert dm.detect and ctx.frame_table_count() == 1          # (the replace falls inside a frame)
    d, keep = radio.vfo_desc(RATE, RATE / 2, RATE / 2, 0.0, "RAW")
    nid = ctx.vfo_replace(vid, d, 2, keep)
    assert ctx.frame_table_count() == 1 and ctx.vfo_frame_count(nid) == 0 and ctx.L.sdrpp_vfo_frame_count(ctx.h, vid) == NOT_FOUND
    ctx.push(x[a:])
    part = (ctx.vfo_sym_read(nid)[0], ctx.vfo_frame_read(nid))
    assert len(part[0]) > 192 + 16                             # more symbols than an open frame would have needed
    check_parts([part], "replace to another capacity", R.Demux())
    ctx.vfo_remove(nid)
    assert ctx.frame_table_count() == 0
    ctx.close()


def test_control_argument_checks(backend):
    from sdrplusplus_amd import capi

    ctx = make_ctx()
    lib = ctx.L
    vid = add_exact(ctx, framer=False)
    plain = add_transparent(ctx)
    fd, fk = m17_frame_desc()
    assert lib.sdrpp_vfo_set_framer(ctx.h, plain, C.byref(fd), 1) == INVALID and b"symbol branch" in lib.sdrpp_last_error(ctx.h)
    assert lib.sdrpp_vfo_set_framer(ctx.h, 12345, C.byref(fd), 1) == NOT_FOUND

    def attempt(**kw):
        f, keep = m17_frame_desc()
        scr, il = keep[2].copy(), keep[3].copy()
        for k, v in kw.items():
            if k == "scr":
                scr[v[0]] = v[1]
            elif k == "il":
                il[v[0]] = v[1]
            else:
                setattr(f, k, v)
        f.scramble = scr.ctypes.data_as(C.POINTER(C.c_uint8)) if kw.get("scramble", 1) is not None else None
        f.interleave = il.ctypes.data_as(C.POINTER(C.c_uint16)) if kw.get("interleave", 1) is not None else None
        return lib.sdrpp_vfo_set_framer(ctx.h, vid, C.byref(f), 1)

    assert attempt() == 0
    ctx.vfo_set_framer(vid, None)
    for bad in (dict(il=(5, 6)), dict(il=(0, 368)), dict(frame_bits=0), dict(frame_bits=4), dict(frame_bits=364), dict(frame_bits=1032), dict(n_sync=0), dict(n_sync=5),
                dict(high_cut=float("nan")), dict(high_cut=float("inf")), dict(scr=(9, 2)), dict(scramble=None), dict(interleave=None)):
        assert attempt(**bad) == INVALID, bad
        assert lib.sdrpp_vfo_frame_count(ctx.h, vid) == INVALID, bad   # nothing was attached
    assert ctx.frame_table_count() == 0
    assert lib.sdrpp_vfo_frame_read(ctx.h, vid, None, -1) == INVALID
    assert lib.sdrpp_pipeline_set_frame_results(ctx.h, 1) == INVALID    # outside pipelined mode
    ctx.close()


def test_control_tickets_without_the_flag_or_the_framer(backend):
    """flag 512 is its own: a block pushed without it, and a VFO without a framer, hold nothing of a framer (SDRPP_ERR_NOT_FOUND); flag 64 is not needed and not
    touched: the symbols of the same block are the ordinary run's"""
    from sdrplusplus_amd import capi

    bits, x = control_stream()
    cut = schedule(len(x), [1000])
    ctx = make_ctx()
    vid = add_exact(ctx)
    other = add_exact(ctx, framer=False)
    parts = run_cut(ctx, [vid], x, cut)[vid]
    exp = check_parts(parts, "ordinary")
    lib = ctx.L
    recs, n = C.POINTER(C.c_uint8)(), C.c_int(0)
    # without the flag
    vid, other = add_exact(ctx), add_exact(ctx, framer=False)
    ctx.set_pipelined(True, capi.RESULT_SYM)
    ctx.push(x[:1000])
    t = ctx.ticket()
    ctx.result_wait(t)
    assert lib.sdrpp_result_frames(ctx.h, t, vid, C.byref(recs), C.byref(n)) == NOT_FOUND
    assert bits_equal(ctx.result_sym(t, vid)[0], parts[0][0])
    ctx.result_release(t)
    assert lib.sdrpp_result_frames(ctx.h, t, vid, C.byref(recs), C.byref(n)) == INVALID   # not held
    ctx.set_pipelined(False)
    # with both flags, and a VFO without a framer
    vid, other = add_exact(ctx), add_exact(ctx, framer=False)
    ctx.set_pipelined(True, capi.RESULT_SYM | capi.RESULT_FRAMES)
    pos, tickets = 0, []
    for s in cut:
        ctx.push(x[pos:pos + s])
        tickets.append(ctx.ticket())
        pos += s
    for k, t in enumerate(tickets):
        ctx.result_wait(t)
        assert np.array_equal(ctx.result_frames(t, vid), exp[k]) and bits_equal(ctx.result_sym(t, vid)[0], parts[k][0])
        assert lib.sdrpp_result_frames(ctx.h, t, other, C.byref(recs), C.byref(n)) == NOT_FOUND
        assert lib.sdrpp_result_frames(ctx.h, t, vid, None, None) == 0
        ctx.result_release(t)
    ctx.set_pipelined(False)
    ctx.close()
