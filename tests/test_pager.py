"""The symbol branch of a RAW VFO on the device (sdrpp_vfo_set_symbols): FSK discriminator -> shaping FIR -> Mueller-Mueller clock recovery -> soft symbols and
bits, the pager decoder's POCSAGDSP (decoder_modules/pager_decoder/src/pocsag/dsp.h, core/src/dsp/clock_recovery/mm.h).

YARDSTICK: tests/golden/pager_ref.npz, recorded from the reference's own POCSAGDSP by tests/golden/make_pager_golden.py.  Its IF inputs reach the branch
unchanged through a VFO that does nothing (24 kS/s in, 24 kS/s out, bandwidth = rate, offset 0: no stage, no resampler, no channel filter, a translation
by exactly (1, 0)) — every such test first checks that the IF stream the device delivers is its input bit for bit.

BOUNDS (test 2): symbol counts per push equal; every bit equal where |soft_ref| >= 0.05, at most 1 % of a case's symbols below that; soft values within
max(1e-5 * RMS, 4 x the spread the reference shows under a one-ulp change of its input: <case>_dev_max per symbol, <case>_dev_rms over the case).  The device's
discriminator is not the reference's atan2f (|error| <= 3e-7 rad), hence the factor.  Everywhere else two paths of the device compute the same thing: bit for bit.
Every other description sym_apply takes, and every tile, job, block, clamp, control and bank edge against a restatement of the reference symbol by symbol: test_pager_rows.py."""
import ctypes as C
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pager_ref.npz")
SR, IF_RATE, BW = 240e3, 24e3, 12.5e3  # wideband shape: one RAW VFO at 24 kS/s / 12.5 kHz, ratio 10
B = 5000                               # one push = 500 IF samples = about 50 symbols at 2400 baud
NOT_FOUND, INVALID, UNSUPPORTED = -6, -2, -5
TILE, SEG = 256, 1024                  # SDRPP_SYM_TILE, SDRPP_SYM_SEG (vfo_sym_kernels.h): outputs per tile and samples per job of the front
PACK = 64                              # SDRPP_SYM_PACK: lanes of a loop job


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype.itemsize == 4 else np.array_equal(a, b)


def same(a, b):
    """(soft, bits) pairs equal bit for bit"""
    return bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])


def cat(parts):
    return (np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.float32), np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.uint8))


def fsk(n, seed, sr=SR, baud=2400.0, f0=0.0, amp=0.3, noise=0.003):
    """2FSK at +-4500 Hz around f0, random bits"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / sr
    bits = r.integers(0, 2, int(n / sr * baud) + 2)
    f = f0 + np.where(bits[(t * baud).astype(np.int64)] == 1, 4500.0, -4500.0)
    x = amp * np.exp(1j * 2 * np.pi * np.cumsum(f) / sr) + noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return x.astype(np.complex64)


def make_ctx(max_push=60000):
    from sdrplusplus_amd import capi

    return capi.Context(0, max_push=max_push)


def add_raw(ctx, baud=2400.0, f0=30e3, sr=SR, if_rate=IF_RATE, bw=BW, sym=True, enabled=True):
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(sr, if_rate, bw, f0, "RAW")
    vid = ctx.vfo_add(d, keep)
    if sym:
        sd, skeep = radio.pager_desc(if_rate, baud)
        ctx.vfo_set_symbols(vid, sd, enabled, skeep)
    return vid


def add_transparent(ctx, baud=2400.0):
    """24 kS/s in and out, bandwidth = rate, offset 0: RxVFO does nothing, the branch sees the pushed samples themselves"""
    return add_raw(ctx, baud, 0.0, IF_RATE, IF_RATE, IF_RATE)


def run_cut(ctx, vids, x, sizes):
    """push x in pushes of `sizes` (cycled) -> per VFO the list of (soft, bits) per push"""
    out, pos, k = {v: [] for v in vids}, 0, 0
    while pos < len(x):
        s = min(sizes[k % len(sizes)], len(x) - pos)
        ctx.push(x[pos:pos + s])
        for v in vids:
            out[v].append(ctx.vfo_sym_read(v))
        pos += s
        k += 1
    return out


def run_pipelined(ctx, vids, x, sizes, group):
    """the same in pipelined mode with launch groups of `group` -> per VFO the list of (soft, bits) per push"""
    from sdrplusplus_amd import capi

    ctx.set_pipelined(True, capi.RESULT_SYM)
    ctx.set_pipeline_group(group)
    pos, k = 0, 0
    while pos < len(x):
        s = min(sizes[k % len(sizes)], len(x) - pos)
        ctx.push(x[pos:pos + s])
        pos += s
        k += 1
    out = {v: [] for v in vids}
    for i in range(k):
        ctx.result_wait(i + 1)
        for v in vids:
            out[v].append(ctx.result_sym(i + 1, v))
        ctx.result_release(i + 1)
    st = ctx.pipeline_stats()
    ctx.set_pipelined(False)
    return out, st


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def stream():
    return fsk(40000, seed=21, f0=30e3)


def case_input(z, name):
    return (z[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)


# ---- 1. design -----------------------------------------------------------------------------------------------------------------------------
def test_design_equals_the_reference_bit_for_bit(golden):
    """sdrpp_design_mm_interp(128, 8) is MM::generateInterpTaps' bank and sdrpp_design_pager's scalars are what POCSAGDSP::init leaves in its blocks (pcl.freq,
    the frequency limits, alpha, beta, Quadrature's 1 / deviation), bit for bit, at 2400, 1200 and 512 baud; the structure's size is the binding's."""
    from sdrplusplus_amd import capi, radio

    z = golden
    bank = capi.design_mm_interp(128, 8)
    assert bank.shape == (128, 8) and bits_equal(bank, z["bank"])
    seen = set()
    for name in z["names"]:
        baud = float(z[name + "_baud"])
        seen.add(baud)
        d, keep = radio.pager_desc(24000.0, baud)
        mine = np.array([d.omega, d.min_omega, d.max_omega, d.mu_gain, d.omega_gain, d.inv_deviation], np.float32)
        assert bits_equal(mine, z[name + "_pcl"]), (name, mine, z[name + "_pcl"])
        assert (d.shape_ntaps, d.interp_phases, d.interp_ntaps) == (10, 128, 8)
        assert bits_equal(keep[0], np.full(10, np.float32(0.1), np.float32)) and bits_equal(keep[1], z["bank"])
    assert seen == {2400.0, 1200.0, 512.0}
    L = capi.load()
    assert L.sdrpp_abi_sizeof_sym_desc() == C.sizeof(capi.SymDesc) == 56
    assert L.sdrpp_design_mm_interp(0, 8, bank.ctypes.data_as(capi.c_float_p)) == INVALID
    assert L.sdrpp_design_mm_interp(128, 17, bank.ctypes.data_as(capi.c_float_p)) == INVALID
    assert L.sdrpp_design_mm_interp(128, 8, None) == INVALID
    assert L.sdrpp_design_pager(24000.0, 0.0, C.byref(capi.SymDesc())) == INVALID


# ---- 2. against the reference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steady_2400", "steady_1200", "steady_512", "noisy_2400", "cuts", "reset"])
def test_against_the_reference_fixture(backend, golden, name):
    """The fixture's IF input through the transparent VFO with the fixture's block schedule (a fresh attach where the fixture starts a fresh POCSAGDSP)."""
    from sdrplusplus_amd import radio

    z = golden
    x, cut, fresh = case_input(z, name), z[name + "_cut"], z[name + "_reset"]
    ref_soft, ref_bits, ref_counts = z[name + "_soft"], z[name + "_bits"], z[name + "_counts"]
    ctx = make_ctx(4096)
    vid = add_transparent(ctx, float(z[name + "_baud"]))
    sd, skeep = radio.pager_desc(IF_RATE, float(z[name + "_baud"]))
    parts, pos = [], 0
    for b, n in enumerate(cut):
        if b in fresh:
            ctx.vfo_set_symbols(vid, None)
            ctx.vfo_set_symbols(vid, sd, True, skeep)
        ctx.push(x[pos:pos + n])
        assert bits_equal(ctx.vfo_read_if(vid).view(np.float32), x[pos:pos + n].view(np.float32)), "the VFO is not transparent"
        parts.append(ctx.vfo_sym_read(vid))
        pos += int(n)
    ctx.close()
    soft, bits = cat(parts)
    assert [len(p[0]) for p in parts] == list(ref_counts), name                       # (a)
    strong = np.abs(ref_soft) >= 0.05
    assert np.array_equal(bits[strong], ref_bits[strong]), name                       # (b)
    assert np.array_equal(bits, (soft > 0.0).astype(np.uint8))
    weak = int((~strong).sum())
    assert weak <= 0.01 * len(ref_soft), (name, weak, len(ref_soft))                  # (c)
    err = soft.astype(np.float64) - ref_soft.astype(np.float64)                       # (d)
    R = rms(ref_soft)
    bar_each = np.maximum(1e-5 * R, 4.0 * z[name + "_dev_max"].astype(np.float64))
    bar_rms = max(1e-5 * R, 4.0 * float(z[name + "_dev_rms"]))
    print("[pager] %s (%s): %d symbols, %d weak, soft error max %.3g (bar %.3g .. %.3g) rms %.3g (bar %.3g), reference RMS %.3f, recorded spread max %.3g rms %.3g" % (
        name, backend, len(soft), weak, np.abs(err).max(), bar_each.min(), bar_each.max(), rms(err), bar_rms, R, z[name + "_dev_max"].max(), float(z[name + "_dev_rms"])))
    assert np.all(np.abs(err) <= bar_each), (name, float(np.abs(err).max()))
    assert rms(err) <= bar_rms, (name, rms(err))


# ---- 3. cut independence, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_push_emu_and_gpu():
    return {}


def one_push(backend, cache, stream):
    if backend not in cache:
        ctx = make_ctx()
        vid = add_raw(ctx)
        cache[backend] = run_cut(ctx, [vid], stream, [len(stream)])[vid][0]
        ctx.close()
    return cache[backend]


@pytest.mark.parametrize("sizes", [[9970, 70, 10, 12500], [2500], [10]], ids=["cuts", "quarter", "one_if_sample"])
def test_cut_independence_ordinary(backend, stream, one_push_emu_and_gpu, sizes):
    """One push of 40 000 samples (4 000 IF samples, 400 symbols) against the `cuts` schedule (at the wideband rate: 997, 7, 1 and 1 250 IF samples), against
    pushes of 250 IF samples and — over the first 6 000 samples — against pushes of ONE IF sample: soft values, bits and the concatenated counts."""
    x = stream if sizes != [10] else stream[:6000]
    want = one_push(backend, one_push_emu_and_gpu, stream)
    ctx = make_ctx()
    vid = add_raw(ctx)
    parts = run_cut(ctx, [vid], x, sizes)[vid]
    ctx.close()
    got = cat(parts)
    n = len(got[0])
    assert n == (len(want[0]) if len(x) == len(stream) else n) and n > 50
    assert same(got, (want[0][:n], want[1][:n]))
    if sizes == [10]:
        counts = [len(p[0]) for p in parts]
        assert set(counts) == {0, 1} and counts.count(0) > 400  # pushes shorter than a symbol: most yield none


@pytest.mark.parametrize("group", [1, 2, 8])
def test_cut_independence_pipelined_and_grouped(backend, stream, one_push_emu_and_gpu, group):
    """Pipelined mode, alone and in launch groups of 2 and 8, pushes of the `cuts` schedule: every ticket's symbols are the ordinary path's of that push, the
    concatenation is the one push's."""
    sizes = [9970, 70, 10, 12500, 2500, 2500]
    want = one_push(backend, one_push_emu_and_gpu, stream)
    ctx = make_ctx()
    vid = add_raw(ctx)
    plain = run_cut(ctx, [vid], stream, sizes)[vid]
    ctx.close()
    ctx = make_ctx()
    vid = add_raw(ctx)
    piped, st = run_pipelined(ctx, [vid], stream, sizes, group)
    ctx.close()
    assert len(piped[vid]) == len(plain)
    for i, (p, q) in enumerate(zip(piped[vid], plain)):
        assert same(p, q), (i, len(p[0]), len(q[0]))
    assert same(cat(piped[vid]), want)
    assert st["pass_blocks"] == 0, st  # every block ran as a tick: the kinds are roles of the tick kernel


# ---- 4. edges on purpose --------------------------------------------------------------------------------------------------------------------
def test_front_tile_and_job_edges(backend):
    """IF counts of tile - 1, tile, tile + 1 and job - 1, job, job + 1 samples (and blocks shorter than the interpolator's and the filter's lines) in one run
    against the same samples in one push — through the transparent VFO, where a push of n samples is n IF samples."""
    ifs = [TILE - 1, TILE, TILE + 1, 3, SEG - 1, 5, SEG, SEG + 1, 2 * SEG + TILE + 1]
    x = fsk(sum(ifs), seed=22, sr=IF_RATE)
    ctx = make_ctx(len(x))
    vid = add_transparent(ctx)
    want = run_cut(ctx, [vid], x, [len(x)])[vid][0]
    ctx.close()
    ctx = make_ctx(len(x))
    vid = add_transparent(ctx)
    parts, pos = [], 0
    for n in ifs:
        ctx.push(x[pos:pos + n])
        assert len(ctx.vfo_read_if(vid)) == n
        parts.append(ctx.vfo_sym_read(vid))
        pos += n
    ctx.close()
    assert same(cat(parts), want) and len(want[0]) > 500


@pytest.mark.parametrize("nvfo", [1, 2, PACK, PACK + 1])
def test_banks_at_the_pack_edge(backend, nvfo):
    """1, 2, 64 and 65 identical branch VFOs (one loop job up to 64, two of 33 and 32 lanes for 65): every channel gives what a single VFO gives."""
    x = fsk(3 * B, seed=23, f0=30e3)
    ctx = make_ctx()
    one = add_raw(ctx)
    want = run_cut(ctx, [one], x, [B])[one]
    ctx.close()
    ctx = make_ctx()
    vids = [add_raw(ctx) for _ in range(nvfo)]
    got = run_cut(ctx, vids, x, [B])
    assert ctx.sym_bank_count() == 1
    ctx.close()
    for v in vids:
        for p, q in zip(got[v], want):
            assert same(p, q), v
    assert sum(len(p[0]) for p in want) > 140


def test_mixed_baud_rates_in_one_job(backend):
    """2400, 1200 and 512 baud in one loop job (lanes that finish a block at different symbol counts): each equals the same VFO alone."""
    x = fsk(4 * B, seed=24, f0=30e3, baud=1200.0)
    alone = {}
    for baud in (2400.0, 1200.0, 512.0):
        ctx = make_ctx()
        v = add_raw(ctx, baud)
        alone[baud] = run_cut(ctx, [v], x, [B])[v]
        ctx.close()
    ctx = make_ctx()
    vids = {baud: add_raw(ctx, baud) for baud in (2400.0, 1200.0, 512.0)}
    got = run_cut(ctx, list(vids.values()), x, [B])
    assert ctx.sym_bank_count() == 1  # three descriptions, one bank
    ctx.close()
    totals = {}
    for baud, v in vids.items():
        for p, q in zip(got[v], alone[baud]):
            assert same(p, q), baud
        totals[baud] = sum(len(p[0]) for p in got[v])
    assert totals[2400.0] > totals[1200.0] > totals[512.0] > 30, totals


@pytest.mark.parametrize("pipelined", [False, True])
def test_a_mixed_bank_keeps_every_other_output(backend, pipelined):
    """Branch VFOs beside a WFM VFO with the stereo decoder, an NFM VFO behind an IF chain and a WFM VFO with the RDS branch, 1 MS/s: the others' outputs are
    bit-identical to the same bank without any symbol branch, the branch's to the branch VFO alone; a RAW VFO's own IF output does not move either."""
    from sdrplusplus_amd import capi, radio

    sr, push, npush = 1e6, 20000, 3
    x = (fsk(npush * push, seed=25, sr=sr, f0=-400e3) + fsk(npush * push, seed=26, sr=sr, f0=200e3, baud=1187.5, amp=0.2)).astype(np.complex64)

    def bank(ctx, sym):
        ids = {}
        ids["pager"] = add_raw(ctx, 2400.0, -400e3, sr, sym=sym)
        d, keep = radio.vfo_desc(sr, 250e3, 150e3, 200e3, "WFM")
        ids["stereo"] = ctx.vfo_add(d, keep)
        s, skeep = radio.stereo_desc(250e3)
        ctx.vfo_set_stereo(ids["stereo"], s, skeep)
        d, keep = radio.vfo_desc(sr, 50e3, 12.5e3, -300e3, "NFM")
        ids["nfm"] = ctx.vfo_add(d, keep)
        ctx.vfo_set_if(ids["nfm"], radio.if_desc(50e3, nb=True, squelch=-60.0))
        d, keep = radio.vfo_desc(sr, 250e3, 150e3, -100e3, "WFM")
        ids["rds"] = ctx.vfo_add(d, keep)
        rd, rkeep = radio.rds_desc(250e3)
        ctx.vfo_set_rds(ids["rds"], rd, True, rkeep)
        ids["pager2"] = add_raw(ctx, 1200.0, -400e3, sr, sym=sym)
        return ids

    def run(sym):
        ctx = make_ctx(push)
        ids = bank(ctx, sym)
        out = []
        if pipelined:
            ctx.set_pipelined(True, 1 | capi.RESULT_RDS | (capi.RESULT_SYM if sym else 0))
        for i in range(npush):
            ctx.push(x[i * push:(i + 1) * push])
            if pipelined:
                res = ctx.result_wait(i + 1)
                o = {k: res["vfo"][v] for k, v in ids.items()}
                o["rds_out"] = ctx.result_rds(i + 1, ids["rds"])
                if sym:
                    o["sym"], o["sym2"] = ctx.result_sym(i + 1, ids["pager"]), ctx.result_sym(i + 1, ids["pager2"])
                ctx.result_release(i + 1)
            else:
                o = {k: ctx.vfo_read(v) for k, v in ids.items()}
                o["rds_out"] = ctx.vfo_rds_read(ids["rds"])
                if sym:
                    o["sym"], o["sym2"] = ctx.vfo_sym_read(ids["pager"]), ctx.vfo_sym_read(ids["pager2"])
            out.append(o)
        if pipelined:
            ctx.set_pipelined(False)
        ctx.close()
        return out

    without, with_ = run(False), run(True)
    for i in range(npush):
        for k in ("pager", "stereo", "nfm", "rds", "pager2", "rds_out"):
            assert len(without[i][k]) > 0 and bits_equal(without[i][k].view(np.float32), with_[i][k].view(np.float32)), (i, k)
    for baud, key in ((2400.0, "sym"), (1200.0, "sym2")):
        ctx = make_ctx(push)
        v = add_raw(ctx, baud, -400e3, sr)
        alone = run_cut(ctx, [v], x, [push])[v]
        ctx.close()
        for i in range(npush):
            assert same(with_[i][key], alone[i]), (key, i)
        assert sum(len(p[0]) for p in alone) > 60


# ---- 5. control surface ----------------------------------------------------------------------------------------------------------------------
def pushes_of(x, n):
    return [x[i:i + n] for i in range(0, len(x), n)]


def test_disable_freezes_and_enable_continues(backend):
    """Through the transparent VFO: pushes 0 .. 3, three pushes with the branch off (other samples: the VFO's stream moves on), pushes 4 .. 8 — the outputs
    equal an uninterrupted run over the nine pushes the branch was on for, bit for bit; nothing is delivered while it is off."""
    from sdrplusplus_amd import radio

    x, other = fsk(9 * 500, seed=27, sr=IF_RATE), fsk(3 * 470, seed=28, sr=IF_RATE)
    sd, skeep = radio.pager_desc(IF_RATE, 2400.0)
    ctx = make_ctx(4096)
    vid = add_transparent(ctx)
    want = run_cut(ctx, [vid], x, [500])[vid]
    ctx.close()
    ctx = make_ctx(4096)
    vid = add_transparent(ctx)
    got = []
    for i, blk in enumerate(pushes_of(x, 500)):
        if i == 4:
            ctx.vfo_set_symbols(vid, sd, False, skeep)
            for o in pushes_of(other, 470):
                ctx.push(o)
                assert ctx.vfo_sym_count(vid) == 0 and len(ctx.vfo_read_if(vid)) == 470
            ctx.vfo_set_symbols(vid, sd, True, skeep)
        ctx.push(blk)
        got.append(ctx.vfo_sym_read(vid))
    ctx.close()
    for i, (p, q) in enumerate(zip(got, want)):
        assert same(p, q), i
    assert sum(len(p[0]) for p in want) > 400


def test_a_new_description_and_a_fresh_attach_start_cleared(backend):
    """Another description (1200 baud) and back, and detach + attach: the next push gives what a new context gives for it; the bank is shared and freed."""
    from sdrplusplus_amd import radio

    x = fsk(4 * 500, seed=29, sr=IF_RATE)
    sd, skeep = radio.pager_desc(IF_RATE, 2400.0)
    sd2, skeep2 = radio.pager_desc(IF_RATE, 1200.0)
    blocks = pushes_of(x, 500)
    fresh = []
    for blk in blocks:
        ctx = make_ctx(4096)
        vid = add_transparent(ctx)
        ctx.push(blk)
        fresh.append(ctx.vfo_sym_read(vid))
        ctx.close()
    ctx = make_ctx(4096)
    vid = add_transparent(ctx)
    ctx.push(blocks[0])
    assert same(ctx.vfo_sym_read(vid), fresh[0])
    ctx.vfo_set_symbols(vid, sd2, True, skeep2)
    ctx.vfo_set_symbols(vid, sd, True, skeep)
    ctx.push(blocks[1])
    assert same(ctx.vfo_sym_read(vid), fresh[1])
    ctx.vfo_set_symbols(vid, None)
    assert ctx.sym_bank_count() == 0
    assert ctx.L.sdrpp_vfo_sym_count(ctx.h, vid) == INVALID
    ctx.vfo_set_symbols(vid, sd, True, skeep)
    ctx.push(blocks[2])
    assert same(ctx.vfo_sym_read(vid), fresh[2])
    ctx.vfo_set_symbols(vid, sd, True, skeep)  # the same description again: nothing changes, the next push continues
    ctx.push(blocks[3])
    cont = ctx.vfo_sym_read(vid)
    ctx.close()
    ctx = make_ctx(4096)
    vid = add_transparent(ctx)
    two = run_cut(ctx, [vid], np.concatenate(blocks[2:4]), [500])[vid]
    ctx.close()
    assert same(cont, two[1]) and not same(cont, fresh[3])


def test_reset_and_replace(backend):
    """sdrpp_vfo_reset: the discriminator's previous phase becomes 0, everything else stays — with a sample of phase exactly 0 in front of the reset the run
    equals the run without it, with any other sample it does not.  sdrpp_vfo_replace: keep & 2 moves the branch (the run continues bit for bit), without
    the bit the new handle has none."""
    from sdrplusplus_amd import radio

    x = fsk(6 * 500, seed=30, sr=IF_RATE)
    x0 = x.copy()
    x0[999] = np.complex64(0.25 + 0j)
    d, keep = radio.vfo_desc(IF_RATE, IF_RATE, IF_RATE, 0.0, "RAW")

    def run(xs, reset_at=None, replace_at=None):
        ctx = make_ctx(4096)
        vid = add_transparent(ctx)
        out = []
        for i, blk in enumerate(pushes_of(xs, 500)):
            if i == reset_at:
                ctx.vfo_reset(vid)
            if i == replace_at:
                old, vid = vid, ctx.vfo_replace(vid, d, 3, keep)
                assert ctx.L.sdrpp_vfo_sym_count(ctx.h, old) == NOT_FOUND
            ctx.push(blk)
            out.append(ctx.vfo_sym_read(vid))
        return ctx, vid, out

    c0, _, plain0 = run(x0)
    c1, _, reset0 = run(x0, reset_at=2)
    c2, _, plain = run(x)
    c3, _, reset = run(x, reset_at=2)
    c4, vid, moved = run(x, replace_at=3)
    for i in range(6):
        assert same(plain0[i], reset0[i]), i
        assert same(plain[i], moved[i]), i
    assert same(plain[1], reset[1]) and not same(plain[2], reset[2])
    assert len(reset[2][0]) == len(plain[2][0])  # (one discriminator value differs: the symbols move a little, their number does not)
    new2 = c4.vfo_replace(vid, d, 1, keep)
    assert c4.L.sdrpp_vfo_sym_count(c4.h, new2) == INVALID and c4.sym_bank_count() == 0
    for c in (c0, c1, c2, c3, c4):
        c.close()


def test_argument_checks(backend):
    """Every error the header names."""
    from sdrplusplus_amd import capi, radio

    ctx = make_ctx()
    raw = add_raw(ctx, sym=False)
    d, keep = radio.vfo_desc(SR, 50e3, 12.5e3, 10e3, "NFM")
    nfm = ctx.vfo_add(d, keep)
    L, h = ctx.L, ctx.h
    good, gkeep = radio.pager_desc(IF_RATE, 2400.0)

    def code(vid=raw, **changes):
        s, k = radio.pager_desc(IF_RATE, 2400.0)
        for name, value in changes.items():
            setattr(s, name, value)
        return L.sdrpp_vfo_set_symbols(h, vid, C.byref(s), 1)

    assert code(nfm) == UNSUPPORTED                      # only RAW VFOs
    assert L.sdrpp_vfo_set_symbols(h, 9999, C.byref(good), 1) == NOT_FOUND
    assert L.sdrpp_vfo_set_symbols(None, raw, C.byref(good), 1) == INVALID
    for bad in (float("nan"), float("inf")):
        for field in ("inv_deviation", "omega", "mu_gain", "omega_gain", "min_omega", "max_omega"):
            assert code(**{field: bad}) == INVALID, (field, bad)
    assert code(min_omega=11.0, max_omega=11.0) == INVALID and code(min_omega=12.0, max_omega=11.0) == INVALID
    assert code(min_omega=0.5) == INVALID                # the loop advances at least one sample per symbol ...
    assert code(min_omega=1.5, mu_gain=1.0) == INVALID   # ... whatever the error term takes away: min_omega - |mu_gain| >= 1
    assert code(min_omega=2.0, mu_gain=-1.0) == 0
    assert code(max_omega=4096.0, mu_gain=1.0) == INVALID and code(max_omega=4095.0, mu_gain=1.0) == 0
    assert code(shape_ntaps=0) == INVALID and code(shape_ntaps=65) == INVALID and code(shape_taps=capi.c_float_p()) == INVALID
    assert code(interp_ntaps=0) == INVALID and code(interp_ntaps=17) == INVALID
    assert code(interp_phases=0) == INVALID and code(interp_phases=1025) == INVALID and code(interp_bank=capi.c_float_p()) == INVALID
    assert L.sdrpp_vfo_set_symbols(h, raw, None, 0) == 0  # detach
    assert L.sdrpp_vfo_sym_count(h, raw) == INVALID and L.sdrpp_vfo_sym_read(h, raw, None, None, 0) == INVALID
    assert L.sdrpp_vfo_sym_device_buffers(h, raw, None, None, None) == INVALID
    assert L.sdrpp_vfo_sym_count(h, 9999) == NOT_FOUND
    assert L.sdrpp_vfo_set_symbols(h, raw, C.byref(good), 0) == 0
    assert L.sdrpp_vfo_sym_count(h, raw) == 0            # attached, switched off
    assert L.sdrpp_vfo_sym_read(h, raw, None, None, -1) == INVALID
    assert L.sdrpp_pipeline_set_sym_results(h, 1) == INVALID  # outside pipelined mode
    assert L.sdrpp_set_pipelined(h, 1, 64) == INVALID and L.sdrpp_set_pipelined(h, 0, 0) == 0  # (the flag has its own call)
    assert L.sdrpp_result_sym(h, 1, raw, None, None, None) == INVALID  # nothing held
    assert L.sdrpp_sym_bank_count(None) == INVALID
    ctx.close()


def test_results_of_tickets_without_the_branch_or_the_flag(backend, stream):
    """Pipelined: a ticket pushed without flag 64, a VFO without the branch and one whose branch is switched off give SDRPP_ERR_NOT_FOUND; a released ticket
    SDRPP_ERR_INVALID; device buffers name the last ordinary push."""
    from sdrplusplus_amd import capi

    ctx = make_ctx()
    a, off, none = add_raw(ctx), add_raw(ctx, enabled=False), add_raw(ctx, sym=False)
    ctx.push(stream[:B])
    want = ctx.vfo_sym_read(a)
    soft, bits, n = C.c_void_p(), C.c_void_p(), C.c_int()
    assert ctx.L.sdrpp_vfo_sym_device_buffers(ctx.h, a, C.byref(soft), C.byref(bits), C.byref(n)) == 0 and n.value == len(want[0]) and soft.value and bits.value
    ctx.close()
    ctx = make_ctx()
    a, off, none = add_raw(ctx), add_raw(ctx, enabled=False), add_raw(ctx, sym=False)
    ctx.set_pipelined(True, 1)
    ctx.push(stream[:B])
    ctx.pipeline_flush()
    assert ctx.L.sdrpp_pipeline_set_sym_results(ctx.h, 1) == 0
    ctx.push(stream[:B])
    ctx.result_wait(1)
    assert ctx.L.sdrpp_result_sym(ctx.h, 1, a, None, None, None) == NOT_FOUND
    ctx.result_release(1)
    ctx.result_wait(2)
    assert len(ctx.result_sym(2, a)[0]) > 40
    assert ctx.L.sdrpp_result_sym(ctx.h, 2, off, None, None, None) == NOT_FOUND
    assert ctx.L.sdrpp_result_sym(ctx.h, 2, none, None, None, None) == NOT_FOUND
    ctx.result_release(2)
    assert ctx.L.sdrpp_result_sym(ctx.h, 2, a, None, None, None) == INVALID
    ctx.set_pipelined(False)
    ctx.close()
