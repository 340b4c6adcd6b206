"""The recorder sink on the device (sdrpp_vfo_set_rec / sdrpp_vfo_rec_read / sdrpp_result_rec, result flag 16): what misc_modules/recorder does to a
radio's audio stream — dsp::audio::Volume (audio/volume.h:14,22,37) -> dsp::bench::PeakLevelMeter<stereo_t> (bench/peak_level_meter.h:52-57) ->
optionally dsp::convert::StereoToMono (convert/stereo_to_mono.h:13-15) -> wav::Writer::write (utils/wav.cpp:158-180) with "ignore silence"
(recorder/src/main.cpp:28, 533-561).

The yardstick is the float32 restatement of those four pieces below.  Every operation is an elementwise float32 product / sum or a maximum, so the
device's bytes and record are a bit-exact function of the float frames the library delivers for the same block: every comparison applies the
restatement to frames the device itself delivered and asserts equality.  There is no tolerance anywhere in this file."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import support as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recorder_ref.npz")
f32 = np.float32
U8, I16, I32, F32 = 0, 1, 2, 3  # wav::SampleType (utils/wav.h:25-30)
SR = 2.4e6
WFM_F, NFM_F, AM_F = 0.6e6, -0.5e6, 0.2e6

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


# ---- the float32 restatement ----------------------------------------------------------------------------------------------------------
def gain_of(volume):
    """Volume::init / setVolume (audio/volume.h:14,22): _volume = powf(volume, 2), a float"""
    return f32(_libm.powf(float(f32(volume)), 2.0))


def convert(w, stype):
    """wav::Writer::write (utils/wav.cpp:166-178) on float32 values"""
    w = np.ascontiguousarray(w, f32)
    if stype == I16:  # volk_32f_s32f_convert_16i, generic: product, clamp, rintf, cast
        r = w * f32(32767.0)
        return np.rint(np.clip(r, f32(-32768.0), f32(32767.0))).astype(np.int16)
    if stype == U8:  # bufU8[i] = (samples[i] * 127.0f) + 128.0f: product, sum, truncation toward zero; outside [0, 256) saturated (the library's definition)
        t = (w * f32(127.0)) + f32(128.0)
        assert t.dtype == f32
        inside = np.trunc(np.clip(t, f32(0.0), f32(255.0)))
        return inside.astype(np.uint8)
    assert stype == F32
    return w.copy()


def restate(frames, volume, mono, stype, ignore_silence):
    """-> (samples [n, channels] in the file's type, record) for one block of stereo float frames"""
    x = np.ascontiguousarray(frames, f32).reshape(-1, 2)
    v = x * gain_of(volume)  # volk_32f_s32f_multiply_32f
    assert v.dtype == f32
    n = len(v)
    peak_l = f32(np.max(np.abs(v[:, 0]))) if n else f32(0)
    peak_r = f32(np.max(np.abs(v[:, 1]))) if n else f32(0)
    w = ((v[:, 0] + v[:, 1]) / f32(2.0)).reshape(-1, 1) if mono else v  # StereoToMono: (l + r) / 2.0f
    assert w.dtype == f32
    abs_max = f32(np.max(np.abs(w))) if n else f32(0)
    silent = int(bool(n > 0 and ignore_silence and float(abs_max) < 10e-6))  # a float against the double SILENCE_LVL; an empty block is never silent
    info = dict(frames=n, channels=1 if mono else 2, sample_type=stype, silent=silent, peak_l=peak_l, peak_r=peak_r, abs_max=abs_max)
    return convert(w, stype), info


def assert_same(got, want, what):
    ga, gi = got
    wa, wi = want
    assert ga.dtype == wa.dtype and ga.shape == wa.shape, (what, ga.dtype, ga.shape, wa.dtype, wa.shape)
    assert np.array_equal(ga.view(np.uint8), wa.view(np.uint8)), (what, "bytes differ", int(np.sum(ga != wa)))
    for k in ("frames", "channels", "sample_type", "silent"):
        assert gi[k] == wi[k], (what, k, gi[k], wi[k])
    for k in ("peak_l", "peak_r", "abs_max"):
        assert f32(gi[k]).view(np.uint32) == f32(wi[k]).view(np.uint32), (what, k, gi[k], wi[k])


# ---- inputs, banks ------------------------------------------------------------------------------------------------------------------------
def signal(n, seed):
    """Two FM carriers (a broadcast one at WFM_F, deviation 50 kHz, 1 kHz tone + its third harmonic; a narrow one at NFM_F, 4 kHz, 700 Hz tone) + noise"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / SR
    a = 0.3 * np.exp(1j * (2 * np.pi * WFM_F * t + 50.0 * np.sin(2 * np.pi * 1e3 * t) + 6.0 * np.sin(2 * np.pi * 3e3 * t + 1.0)))
    b = 0.2 * np.exp(1j * (2 * np.pi * NFM_F * t + (4e3 / 700.0) * np.sin(2 * np.pi * 700.0 * t)))
    x = a + b + 0.002 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return x.astype(np.complex64)


class Bank:
    """A WFM VFO with an AF chain to 48 kHz, an NFM VFO without one and (optionally) an AM VFO that never gets a sink"""

    def __init__(self, max_push, third=False, deemph=True):
        from sdrplusplus_amd import capi, radio

        self.ctx = capi.Context(0, max_push=max_push)
        d, keep = radio.vfo_desc(SR, 250e3, 150e3, WFM_F, "WFM")
        self.wfm = self.ctx.vfo_add(d, keep)
        self.wfm_desc = (d, keep)
        self.af = radio.af_desc(250e3, 48000.0, 50e-6 if deemph else None, False)
        self.ctx.vfo_set_af(self.wfm, *self.af)
        d, keep = radio.vfo_desc(SR, 50e3, 12500.0, NFM_F, "NFM")
        self.nfm = self.ctx.vfo_add(d, keep)
        self.other = None
        if third:
            d, keep = radio.vfo_desc(SR, 15e3, 10e3, AM_F, "AM")
            self.other = self.ctx.vfo_add(d, keep)

    def frames(self, vid):
        """the float frames the sink of `vid` read in the most recent push: the AF chain's output where one is attached, else the demodulator's"""
        return self.ctx.vfo_af_read(vid) if (vid == self.wfm and self.af_on()) else self.ctx.vfo_read(vid)

    def af_on(self):
        try:
            self.ctx.vfo_af_count(self.wfm)
            return True
        except Exception:
            return False

    def close(self):
        self.ctx.close()


# pushes of at most 24 000 samples at 2.4 MS/s; the AF chain delivers one frame per 50 input samples: 1, 3 (odd), 63 / 64 / 65, 259 (> 256, no multiple of 4)
PUSHES = [50, 150, 3150, 3200, 3250, 12950]
WANT_COUNTS = {1, 3, 63, 64, 65, 259}


def cut(x, sizes):
    out, pos = [], 0
    for n in sizes:
        out.append(x[pos:pos + n])
        pos += n
    assert pos <= len(x)
    return out


# ---- 0. the restatement itself (passes without the feature) ------------------------------------------------------------------------------
def test_restatement_int16_leg_equals_oracle_and_saturation_rules():
    r = np.random.default_rng(5)
    w = np.concatenate([r.standard_normal(4096).astype(f32) * f32(0.7), np.asarray([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, 1e-9, 40.0, -40.0], f32)])
    o = S.oracle()
    fp = C.POINTER(C.c_float)
    ref = np.empty(len(w), np.int16)
    o.orc_convert_16i.argtypes = [fp, C.c_float, C.c_int, C.c_void_p]
    o.orc_convert_16i(w.ctypes.data_as(fp), 32767.0, len(w), ref.ctypes.data_as(C.c_void_p))
    assert np.array_equal(convert(w, I16), ref)
    # UINT8: truncation toward zero inside [0, 256), saturation outside (the reference's cast is undefined there)
    t = np.asarray([0.0, 1.0, -1.0, 0.999, -0.999, 0.5 / 127, -0.5 / 127, -128.5 / 127, 126.9 / 127, 127.0 / 127, 127.5 / 127, 3.0, -3.0], f32)
    assert convert(t, U8).tolist() == [128, 255, 1, 254, 1, 128, 127, 0, 254, 255, 255, 255, 0]
    assert gain_of(0.5) == f32(0.25) and gain_of(8.0) == f32(64.0)
    a, info = restate(np.zeros((0, 2), f32), 1.0, True, I16, True)
    assert a.shape == (0, 1) and info["silent"] == 0 and info["abs_max"] == 0


def test_restatement_equals_reference_fixture():
    """tests/golden/recorder_ref.npz (tests/golden/make_recorder_golden.py: volume.h, stereo_to_mono.h and peak_level_meter.h compiled unmodified): the volume's
    output, the mono fold and the meter's running level, bit for bit; the restatement's record per block agrees with them."""
    z = np.load(GOLDEN)
    assert len(z["names"]) >= 5
    bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)  # noqa: E731
    for name in z["names"]:
        x, vol, cutv = z[name + "_x"], float(z[name + "_vol"][0]), z[name + "_cut"]
        v = x * gain_of(vol)
        assert np.array_equal(bits(v), bits(z[name + "_v"])), name
        m = (v[:, 0] + v[:, 1]) / f32(2.0)
        assert np.array_equal(bits(m), bits(z[name + "_m"])), name
        level, pos = np.zeros(2, f32), 0
        for b, n in enumerate(cutv):
            samples, info = restate(x[pos:pos + n], vol, True, F32, True)
            assert np.array_equal(bits(samples.reshape(-1)), bits(z[name + "_m"][pos:pos + n])), (name, b)
            assert info["abs_max"] == f32(np.max(np.abs(z[name + "_m"][pos:pos + n])))
            level = np.maximum(level, np.asarray([info["peak_l"], info["peak_r"]], f32))
            assert np.array_equal(bits(level), bits(z[name + "_lvl"][b])), (name, b)
            pos += n
    assert restate(z["tiny_x"], 0.31, True, I16, True)[1]["silent"] == 1 and restate(z["unity_x"], 1.0, True, I16, True)[1]["silent"] == 0


# ---- 1. ordinary pass ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
@pytest.mark.parametrize("stype", [U8, I16, F32], ids=["u8", "i16", "f32"])
def test_ordinary_pass_equals_restatement(backend, stype, mono):
    """Every push of an ordinary pass, WFM + AF chain and NFM without one: bytes and record equal the restatement of the float frames read from the same push;
    the frame counts cover 1, an odd count, 63 / 64 / 65, 259 and an empty block."""
    bank = Bank(24000)
    ctx = bank.ctx
    ctx.vfo_set_rec(bank.wfm, 0.8, mono, stype, False)
    ctx.vfo_set_rec(bank.nfm, 1.3, mono, stype, True)
    sizes = [10, 10, 30] + PUSHES  # (the second push ends inside the first 50 samples: no AF frame)
    x = signal(sum(sizes), 1)
    seen = {bank.wfm: set(), bank.nfm: set()}
    for i, blk in enumerate(cut(x, sizes)):
        ctx.push(blk)
        for vid, vol, ign in ((bank.wfm, 0.8, False), (bank.nfm, 1.3, True)):
            fr = bank.frames(vid)
            seen[vid].add(len(fr))
            assert_same(ctx.vfo_rec_read(vid), restate(fr, vol, mono, stype, ign), ("push", i, "vfo", vid))
    assert WANT_COUNTS | {0} <= seen[bank.wfm], sorted(seen[bank.wfm])
    assert len(seen[bank.nfm]) >= 5, sorted(seen[bank.nfm])
    bank.close()


# ---- 2. clipping ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stype", [U8, I16], ids=["u8", "i16"])
def test_clipping(backend, stype):
    """A volume above 1 (2: the gain is 4, the audio swings to about +-2.8): INT16 clamps, UINT8 saturates at both ends, and samples in between stay what they are."""
    VOL = 2.0
    bank = Bank(24000)
    ctx = bank.ctx
    x = signal(24000 + 9950, 2)
    clipped = 0
    for mono in (False, True):
        ctx.vfo_set_rec(bank.wfm, VOL, mono, stype, False)
        for blk in cut(x, [24000, 9950]):
            ctx.push(blk)
            fr = bank.frames(bank.wfm)
            want = restate(fr, VOL, mono, stype, False)
            assert_same(ctx.vfo_rec_read(bank.wfm), want, (stype, mono))
            # the yardstick's side: this block really clips, at both ends, and not everywhere
            v = fr * gain_of(VOL)
            w = ((v[:, 0] + v[:, 1]) / f32(2.0)) if mono else v
            lim = f32(1.0) if stype == I16 else f32(127.5 / 127.0)
            assert np.any(w > lim) and np.any(w < -lim) and np.any(np.abs(w) < f32(0.5)), (stype, mono)
            lo, hi = (0, 255) if stype == U8 else (-32768, 32767)
            assert np.any(want[0] == lo) and np.any(want[0] == hi)
            clipped += int(np.sum((want[0] == lo) | (want[0] == hi)))
    assert clipped > 100
    bank.close()


# ---- 3. silence ----------------------------------------------------------------------------------------------------------------------------
def test_ignore_silence(backend):
    bank = Bank(24000)
    ctx, wfm = bank.ctx, bank.wfm
    ctx.vfo_set_rec(wfm, 1.0, True, I16, True)
    ctx.push(np.zeros(12950, np.complex64))  # exact zeros into a VFO whose delay lines are clear: exact zeros out
    fr = bank.frames(wfm)
    assert len(fr) >= 259 and not np.any(fr)
    got = ctx.vfo_rec_read(wfm)
    assert got[1]["silent"] == 1 and got[1]["abs_max"] == 0 and got[1]["frames"] == len(fr) and not np.any(got[0])
    assert_same(got, restate(fr, 1.0, True, I16, True), "zeros, ignore_silence on")
    ctx.vfo_set_rec(wfm, 1.0, True, I16, False)  # the same block with the switch off
    got = ctx.vfo_rec_read(wfm)
    assert got[1]["silent"] == 0
    assert_same(got, restate(fr, 1.0, True, I16, False), "zeros, ignore_silence off")
    ctx.vfo_set_rec(wfm, 1.0, True, I16, True)
    x = signal(12950 + 3250, 3)
    ctx.push(x[:12950])
    fr = bank.frames(wfm)
    got = ctx.vfo_rec_read(wfm)
    assert got[1]["silent"] == 0 and got[1]["abs_max"] > 1e-3
    assert_same(got, restate(fr, 1.0, True, I16, True), "signal")
    # a block that is quiet, not zero: the volume takes it under SILENCE_LVL, abs_max stays exact
    for stereo_vol in (1e-3, 3e-3):
        ctx.vfo_set_rec(wfm, stereo_vol, False, F32, True)
        ctx.push(x[12950:])
        fr = bank.frames(wfm)
        want = restate(fr, stereo_vol, False, F32, True)
        got = ctx.vfo_rec_read(wfm)
        assert_same(got, want, "quiet")
        assert got[1]["abs_max"] > 0
        x = np.roll(x, 17)
    assert 0 < float(gain_of(1e-3)) * 1.0 < 10e-6
    ctx.vfo_set_rec(wfm, 1e-3, False, F32, True)
    ctx.push(x[:3250])
    assert ctx.vfo_rec_read(wfm)[1]["silent"] == 1
    bank.close()


# ---- 4. pipelined: result flag 16 alone and next to flag 1, one block per launch ------------------------------------------------------------
SINKS = lambda b: ((b.wfm, 0.9, True, I16, True), (b.nfm, 1.2, False, U8, False))  # noqa: E731


def _run_ordinary(sizes, x, sinks_of=SINKS):
    bank = Bank(4 * 24000, third=True)
    for vid, vol, mono, st, ign in sinks_of(bank):
        bank.ctx.vfo_set_rec(vid, vol, mono, st, ign)
    out = []
    for blk in cut(x, sizes):
        bank.ctx.push(blk)
        row = {}
        for vid, vol, mono, st, ign in sinks_of(bank):
            fr = bank.frames(vid).copy()
            got = bank.ctx.vfo_rec_read(vid)
            assert_same(got, restate(fr, vol, mono, st, ign), "ordinary")
            row[vid] = (fr, got)
        out.append(row)
    bank.close()
    return out


def _run_pipelined(sizes, x, flags, group=1, sinks_of=SINKS, deemph=True):
    """-> per push {vid: (float frames or None, (samples, record))}, the bank's statistics"""
    from sdrplusplus_amd import capi

    bank = Bank(4 * 24000, third=True, deemph=deemph)
    ctx = bank.ctx
    for vid, vol, mono, st, ign in sinks_of(bank):
        ctx.vfo_set_rec(vid, vol, mono, st, ign)
    ctx.set_pipelined(True, flags)
    if group > 1:
        ctx.set_pipeline_group(group, adaptive=False)
    for blk in cut(x, sizes):
        ctx.push(blk)
    out = []
    for tk in range(1, len(sizes) + 1):
        res = ctx.result_wait(tk)
        row = {}
        if flags & 1:
            assert set(res["vfo"]) == {bank.wfm, bank.nfm, bank.other}
        else:
            assert res["vfo"] == {}  # flag 16 alone: no float frames cross the bus
        for vid, vol, mono, st, ign in sinks_of(bank):
            row[vid] = (res["vfo"].get(vid), ctx.result_rec(tk, vid))
        info = capi.RecInfo()
        assert ctx.L.sdrpp_result_rec(ctx.h, tk, bank.other, None, C.byref(info)) == -6  # SDRPP_ERR_NOT_FOUND: a VFO without a sink
        ctx.result_release(tk)
        assert ctx.L.sdrpp_result_rec(ctx.h, tk, bank.wfm, None, C.byref(info)) < 0  # only between wait and release
        out.append(row)
    st = ctx.pipeline_stats()
    gs = ctx.pipeline_group_stats()
    ctx.set_pipelined(False)
    bank.close()
    return out, st, gs


@pytest.mark.parametrize("flags", [16, 17])
def test_pipelined_results_equal_ordinary_pass(backend, flags):
    sizes = [10, 10, 30] + PUSHES + [24000]
    x = signal(sum(sizes), 4)
    want = _run_ordinary(sizes, x)
    got, st, _ = _run_pipelined(sizes, x, flags)
    assert st["tick_blocks"] == len(sizes) and st["pass_blocks"] == 0, st
    for i, (w, g) in enumerate(zip(want, got)):
        for (vid, vol, mono, stype, ign), wv, gv in zip(SINKS(Ids(w)), w.values(), g.values()):
            assert_same(gv[1], wv[1], ("ticket", i + 1, vid))
            if flags & 1:  # the restatement of the float frames the same ticket delivered
                assert np.array_equal(gv[0].view(np.uint32), wv[0].view(np.uint32))
                assert_same(gv[1], restate(gv[0], vol, mono, stype, ign), ("ticket", i + 1, vid, "own frames"))
    assert {len(w[list(w)[0]][0]) for w in want} >= WANT_COUNTS | {0}


class Ids:
    """the VFO ids of a result row under the names SINKS uses (both runs add their VFOs in the same order)"""

    def __init__(self, row):
        self.wfm, self.nfm = list(row)[:2]


def test_pipelined_slow_path_fills_the_same_layout(backend):
    """a block of a pipelined run that falls back to an ordinary pass (here: the retune hand-over of a VFO) delivers its recorder results like any other"""
    from sdrplusplus_amd import capi

    sizes = [3250, 3250, 3250]
    x = signal(sum(sizes), 6)
    bank = Bank(24000)
    ctx = bank.ctx
    ctx.vfo_set_rec(bank.wfm, 0.9, True, I16, False)
    ctx.set_pipelined(True, 17)
    blocks = cut(x, sizes)
    ctx.push(blocks[0])
    re, im = capi.design_phase_delta(-(WFM_F + 1e3), SR)
    ctx.vfo_set_phase_delta(bank.wfm, re, im)
    ctx.push(blocks[1])
    ctx.push(blocks[2])
    for tk in (1, 2, 3):
        res = ctx.result_wait(tk)
        assert_same(ctx.result_rec(tk, bank.wfm), restate(res["vfo"][bank.wfm], 0.9, True, I16, False), ("ticket", tk))
        assert len(res["vfo"][bank.wfm]) > 0
        ctx.result_release(tk)
    assert ctx.pipeline_stats()["pass_blocks"] >= 1, ctx.pipeline_stats()
    ctx.set_pipelined(False)
    bank.close()


# ---- 5. launch groups ------------------------------------------------------------------------------------------------------------------------
def test_launch_groups_equal_block_by_block(backend):
    """Groups of four pushes, mono INT16 and mono UINT8: every push's bytes and record equal the one-block-per-launch run; the shares start at odd frames
    of the group's block (AF frames 3 | 65 | 1 | 259 of a fresh chain: boundaries at 3, 68, 69), so their bytes are element aligned only.
    The AF chain runs without its de-emphasis here: that recursion is evaluated as a scan whose segments start where a launch starts, so its FLOAT frames differ
    in the last bit between the two runs (tests/test_pipelined.py::test_grouped_launches_equal_block_by_block) — the sink's bytes then follow the frames they were
    made from, which the third comparison below (each push against the restatement of its own frames) covers for any chain."""
    sinks = lambda b: ((b.wfm, 0.9, True, I16, True), (b.nfm, 1.2, True, U8, False))  # noqa: E731
    sizes = [100, 3250, 50, 12950, 3150, 50, 3250, 150]
    x = signal(sum(sizes), 7)
    one, _, _ = _run_pipelined(sizes, x, 17, 1, sinks, deemph=False)
    grp, st, gs = _run_pipelined(sizes, x, 17, 4, sinks, deemph=False)
    assert gs["multi_groups"] >= 2 and gs["largest"] == 4, gs
    assert st["pass_blocks"] == 0, st
    bounds = np.cumsum([len(r[list(r)[0]][0]) for r in one[:4]])
    assert bounds[0] % 2 == 1 and bounds[2] % 2 == 1, bounds
    for i, (a, b) in enumerate(zip(one, grp)):
        for (vid, vol, mono, stype, ign), av, bv in zip(sinks(Ids(a)), a.values(), b.values()):
            assert np.array_equal(av[0].view(np.uint32), bv[0].view(np.uint32)), ("frames", i)
            assert_same(bv[1], av[1], ("push", i, vid))
            assert_same(bv[1], restate(bv[0], vol, mono, stype, ign), ("push", i, vid, "own frames"))
    g16, _, gs16 = _run_pipelined(sizes, x, 16, 4, sinks, deemph=False)
    assert gs16["multi_groups"] >= 2
    for i, (a, b) in enumerate(zip(one, g16)):
        for av, bv in zip(a.values(), b.values()):
            assert_same(bv[1], av[1], ("flag 16 alone, push", i))


def test_launch_groups_with_deemphasis_equal_restatement_of_own_frames(backend):
    """The same groups with the AF chain's de-emphasis ON: its float frames depend on where a launch starts (see above), so there is no block-by-block run to
    equal — every push's bytes and record equal the restatement of the float frames the SAME ticket delivered (flag 1 next to flag 16)."""
    sinks = lambda b: ((b.wfm, 0.9, True, I16, True), (b.nfm, 1.2, True, U8, False))  # noqa: E731
    sizes = [100, 3250, 50, 12950, 3150, 50, 3250, 150]
    grp, st, gs = _run_pipelined(sizes, signal(sum(sizes), 7), 17, 4, sinks, deemph=True)
    assert gs["multi_groups"] >= 2 and gs["largest"] == 4 and st["pass_blocks"] == 0, (gs, st)
    for i, row in enumerate(grp):
        for (vid, vol, mono, stype, ign), (frames, got) in zip(sinks(Ids(row)), row.values()):
            assert_same(got, restate(frames, vol, mono, stype, ign), ("push", i, vid))
    assert sum(len(row[list(row)[0]][0]) for row in grp) >= 380


# ---- 6. the control surface ----------------------------------------------------------------------------------------------------------------
def test_parameter_changes_reattachment_and_refusals(backend):
    from sdrplusplus_amd import capi, radio

    bank = Bank(24000)
    ctx, wfm = bank.ctx, bank.wfm
    L = ctx.L
    sizes = [3250] * 9
    blocks = cut(signal(sum(sizes), 8), sizes)
    info = capi.RecInfo()
    assert L.sdrpp_vfo_rec_read(ctx.h, wfm, None, 0, C.byref(info)) == -2  # no sink yet
    steps = [(0.7, False, I16), (1.4, False, I16), (1.4, False, U8), (1.4, True, U8)]  # volume, then type, then mono
    for blk, (vol, mono, st) in zip(blocks, steps):
        ctx.vfo_set_rec(wfm, vol, mono, st, False)
        ctx.push(blk)
        assert_same(ctx.vfo_rec_read(wfm), restate(bank.frames(wfm), vol, mono, st, False), (vol, mono, st))
    ctx.vfo_set_rec(wfm, attach=False)
    ctx.push(blocks[4])
    assert L.sdrpp_vfo_rec_read(ctx.h, wfm, None, 0, C.byref(info)) == -2
    ctx.vfo_set_rec(wfm, 0.6, True, F32, False)
    assert_same(ctx.vfo_rec_read(wfm), restate(bank.frames(wfm), 0.6, True, F32, False), "re-attached")
    # the AF chain moves what the sink reads
    ctx.vfo_set_af(wfm, None)
    ctx.push(blocks[5])
    fr = ctx.vfo_read(wfm)
    assert len(fr) > 300  # the demodulator's rate now
    assert_same(ctx.vfo_rec_read(wfm), restate(fr, 0.6, True, F32, False), "AF chain detached")
    ctx.vfo_set_af(wfm, *bank.af)
    ctx.push(blocks[6])
    fr = ctx.vfo_af_read(wfm)
    assert 60 < len(fr) < 70  # the audio rate again
    assert_same(ctx.vfo_rec_read(wfm), restate(fr, 0.6, True, F32, False), "AF chain attached behind the sink")
    # sdrpp_vfo_replace leaves the new handle without a sink
    d, keep = bank.wfm_desc
    new = ctx.vfo_replace(wfm, d, 3, keep)
    ctx.push(blocks[7])
    assert L.sdrpp_vfo_rec_read(ctx.h, new, None, 0, C.byref(info)) == -2
    ctx.vfo_set_rec(new, 0.6, False, I16, False)
    assert_same(ctx.vfo_rec_read(new), restate(ctx.vfo_read(new), 0.6, False, I16, False), "new handle")
    # refusals
    bad = capi.RecDesc(1.0, 0, I32, 0)
    assert L.sdrpp_vfo_set_rec(ctx.h, new, C.byref(bad)) == -5  # INT32: SDRPP_ERR_UNSUPPORTED
    assert L.sdrpp_vfo_set_rec(ctx.h, new, C.byref(capi.RecDesc(1.0, 0, 4, 0))) == -2
    assert L.sdrpp_vfo_set_rec(ctx.h, 4711, C.byref(capi.RecDesc(1.0, 0, I16, 0))) == -6
    assert_same(ctx.vfo_rec_read(new), restate(ctx.vfo_read(new), 0.6, False, I16, False), "a refused call changes nothing")
    rd, rkeep = radio.vfo_desc(SR, 50e3, 50e3, 0.9e6, "RAW")
    raw = ctx.vfo_add(rd, rkeep)
    assert L.sdrpp_vfo_set_rec(ctx.h, raw, C.byref(capi.RecDesc(1.0, 0, I16, 0))) == -5  # RAW: SDRPP_ERR_UNSUPPORTED
    assert L.sdrpp_set_pipelined(ctx.h, 1, 32) == -2 and L.sdrpp_set_pipelined(ctx.h, 1, 31) == 0 and L.sdrpp_set_pipelined(ctx.h, 0, 0) == 0
    bank.close()


def test_pipelined_parameter_change_applies_from_the_next_block(backend):
    """blocks already pushed keep the parameters they were pushed with; a sink attached in the middle of a run delivers from the next block on"""
    from sdrplusplus_amd import capi

    bank = Bank(24000)
    ctx, wfm, nfm = bank.ctx, bank.wfm, bank.nfm
    sizes = [3250, 3200, 3150, 12950]
    blocks = cut(signal(sum(sizes), 9), sizes)
    ctx.set_pipelined(True, 17)
    ctx.vfo_set_rec(wfm, 0.7, False, I16, False)
    ctx.push(blocks[0])
    ctx.vfo_set_rec(wfm, 1.1, True, U8, True)
    ctx.push(blocks[1])
    ctx.vfo_set_rec(nfm, 1.0, True, I16, False)
    ctx.push(blocks[2])
    ctx.vfo_set_rec(wfm, attach=False)
    ctx.push(blocks[3])
    par = [(0.7, False, I16, False), (1.1, True, U8, True), (1.1, True, U8, True), None]
    info = capi.RecInfo()
    for tk in (1, 2, 3, 4):
        res = ctx.result_wait(tk)
        if par[tk - 1]:
            assert_same(ctx.result_rec(tk, wfm), restate(res["vfo"][wfm], *par[tk - 1]), ("wfm", tk))
        else:
            assert ctx.L.sdrpp_result_rec(ctx.h, tk, wfm, None, C.byref(info)) == -6
        if tk >= 3:
            assert_same(ctx.result_rec(tk, nfm), restate(res["vfo"][nfm], 1.0, True, I16, False), ("nfm", tk))
        else:
            assert ctx.L.sdrpp_result_rec(ctx.h, tk, nfm, None, C.byref(info)) == -6  # pushed before the sink was attached
        ctx.result_release(tk)
    ctx.set_pipelined(False)
    bank.close()
