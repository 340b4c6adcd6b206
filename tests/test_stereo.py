"""The WFM demodulator's stereo branch on the device (sdrpp_vfo_set_stereo): pilot filter -> PLL -> L-R matrix -> L / R low-pass, the `_stereo` path of
dsp::demod::BroadcastFM (core/src/dsp/demod/broadcast_fm.h:147-191).

YARDSTICK: tests/golden/stereo_ref*.npz (tests/golden/make_stereo_golden.py): the reference's own BroadcastFM, compiled unmodified, over IF-rate inputs.  The VFOs
here are fed AT the IF rate (250 kS/s in, 250 kS/s out, offset 0, no channel filter: the translation multiplies by (1, 0), every sample reaches the
demodulator bit for bit), with the fixture's deviation.

BOUNDS: 1e-5 of the reference's RMS (BASELINE.json's audio bar) per channel and, separately, for l - r against rms(l - r), over the whole stream from the first
sample; bit for bit wherever two paths of the device compute the same thing."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IF_RATE = 250e3
D = 159              # the branch's delay at 250 kS/s: (317 - 1) / 2 + 1
PACK = 8             # SDRPP_ST_PACK: VFOs a loop job packs (vfo_stereo_kernels.h)
INVALID, UNSUPPORTED = -2, -5
BAR = 1e-5


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a ** 2))) if a.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_gold = {}


def gold():
    """the three fixture files as one dictionary, loaded once and left unchanged"""
    if not _gold:
        for fn in ("stereo_ref.npz", "stereo_ref_cuts.npz", "stereo_ref_toggle.npz"):
            _gold.update(np.load(os.path.join(GOLD, fn)))
    return _gold


def case_x(name):
    return (gold()[name + "_x"].astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)


def add_wfm(ctx, low_pass=True, stereo=True, if_rate=IF_RATE, mode="WFM"):
    """a VFO fed at its IF rate; WFM with the fixture's deviation (75 kHz)"""
    from sdrplusplus_amd import radio

    d, keep = radio.vfo_desc(if_rate, if_rate, if_rate, 0.0, mode, low_pass=low_pass)
    if mode == "WFM":
        d.inv_deviation = np.float32(1.0 / radio.hz_to_rads(75000.0, if_rate))
    vid = ctx.vfo_add(d, keep)
    if stereo:
        sd, skeep = radio.stereo_desc(if_rate)
        ctx.vfo_set_stereo(vid, sd, skeep)
    return vid


def make_ctx(max_push=16384):
    from sdrplusplus_amd import capi

    return capi.Context(0, max_push=max_push)


def run_case(name, cut=None, ops=True):
    """the fixture's case on one stereo VFO with the fixture's block schedule (or `cut`) and operations -> frames per push"""
    from sdrplusplus_amd import radio

    z = gold()
    x = case_x(name)
    ctx = make_ctx()
    vid = add_wfm(ctx, low_pass=bool(z[name + "_lp"]))
    sd, skeep = radio.stereo_desc(IF_RATE)
    out, pos = [], 0
    sched = z[name + "_cut"] if cut is None else cut
    for b, n in enumerate(sched):
        op = int(z[name + "_ops"][b]) if (ops and cut is None) else 0
        if op in (1, 2):
            sd.enabled = int(op == 2)
            ctx.vfo_set_stereo(vid, sd, skeep)
        elif op == 3:
            ctx.vfo_reset(vid)
        ctx.push(x[pos:pos + int(n)])
        pos += int(n)
        out.append(ctx.vfo_read(vid).copy())
    assert pos == len(x)
    ctx.close()
    return out


def distances(got, want):
    """-> (l, r, l - r) distances, each relative to the reference's RMS of that quantity"""
    gd, wd = got[:, 0] - got[:, 1], want[:, 0] - want[:, 1]
    return rms(got[:, 0] - want[:, 0]) / rms(want[:, 0]), rms(got[:, 1] - want[:, 1]) / rms(want[:, 1]), rms(gd - wd) / rms(wd)


def schedule(n, sizes):
    out, pos, k = [], 0, 0
    while pos < n:
        s = min(sizes[k % len(sizes)], n - pos)
        out.append(s)
        pos += s
        k += 1
    return out


# ---- 1. host design ------------------------------------------------------------------------------------------------------------------------
def test_host_design_equals_the_reference_bit_for_bit():
    """sdrpp_design_band_pass_complex and sdrpp_design_pll give the 317 pilot taps and the loop constants the compiled reference computed, bit for bit; the
    description radio.stereo_desc builds carries them, the delay of 159 and the three frequencies as floats."""
    from sdrplusplus_amd import capi, radio

    z = gold()
    taps = capi.design_band_pass_complex(18750.0, 19250.0, 3000.0, IF_RATE, True)
    assert len(taps) == 317
    assert bits_equal(taps.view(np.float32).reshape(-1, 2), z["pilot_taps"])
    a, b = capi.design_pll(25000.0 / IF_RATE)
    assert bits_equal(np.float32([a, b]), np.float32([z["alpha"], z["beta"]]))
    assert abs(a - 0.245647) < 1e-6 and abs(b - 0.0347397) < 1e-7
    assert len(capi.design_band_pass_complex(18750.0, 19250.0, 3000.0, 240e3, True)) == 305  # (an even estimate made odd)
    sd, _ = radio.stereo_desc(IF_RATE)
    assert (sd.pilot_ntaps, sd.delay, sd.enabled) == (317, int(z["delay"]), 1) and sd.delay == D
    assert sd.alpha == np.float32(a) and sd.beta == np.float32(b)
    want = [np.float32(2.0 * np.pi * (f / IF_RATE)) for f in (19000.0, 18750.0, 19250.0)]
    assert [sd.init_freq, sd.min_freq, sd.max_freq] == want
    assert C.sizeof(capi.StereoDesc) == capi.load().sdrpp_abi_sizeof_stereo_desc()


# ---- 2. parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["steady", "cuts", "nolp"])
def test_parity_with_the_reference(backend, name):
    """The fixture's inputs in the fixture's blocks: l, r and l - r each within 1e-5 of the reference's RMS of that quantity, over the whole stream,
    acquisition included; frame counts per push equal the block sizes.
    Measured (l, r, l - r), emulator: steady 1.54e-7, 2.25e-7, 2.17e-7; cuts 1.57e-7, 2.27e-7, 2.20e-7; nolp 3.00e-7, 4.27e-7, 3.69e-7.
    Measured on an MI355X: steady 1.60e-7, 2.31e-7, 2.26e-7; cuts 1.62e-7, 2.33e-7, 2.28e-7; nolp 3.06e-7, 4.38e-7, 3.79e-7."""
    z = gold()
    out = run_case(name)
    assert [len(o) for o in out] == [int(n) for n in z[name + "_cut"]]
    got, want = np.concatenate(out), z[name + "_audio"]
    dl, dr, dd = distances(got, want)
    print("[stereo] %s %s: l %.3g r %.3g l-r %.3g of the reference's RMS" % (backend, name, dl, dr, dd))
    assert np.all(np.isfinite(got))
    assert dl < BAR and dr < BAR and dd < BAR, (name, dl, dr, dd)
    assert rms(got[:, 0] - got[:, 1]) > 0.1 * rms(got)  # (there is a difference channel to compare)


# ---- 3. no pilot ---------------------------------------------------------------------------------------------------------------------------
def test_without_a_pilot_the_sum_channel_is_the_delayed_mono_audio(backend):
    """Without the 19 kHz tone the loop follows filtered noise and l - r is sensitive to the last bit: not compared.  (l + r) / 2 equals the same VFO's mono
    audio delayed by 159 samples within 1e-5 of its RMS, and every value is finite.  Measured: 3.54e-7 (emulator), 3.53e-7 (MI355X)."""
    x = case_x("nopilot")
    ctx = make_ctx()
    st, mono = add_wfm(ctx), add_wfm(ctx, stereo=False)
    g, m = [], []
    for lo in range(0, len(x), 1250):
        ctx.push(x[lo:lo + 1250])
        g.append(ctx.vfo_read(st).copy())
        m.append(ctx.vfo_read(mono).copy())
    ctx.close()
    g, m = np.concatenate(g), np.concatenate(m)
    assert np.all(np.isfinite(g)) and len(g) == len(x)
    assert np.array_equal(m[:, 0], m[:, 1])
    want = np.concatenate([np.zeros(D, np.float32), m[:-D, 0]])
    rel = rms((g[:, 0] + g[:, 1]) / np.float32(2.0) - want) / rms(want)
    print("[stereo] %s no pilot: (l + r) / 2 against the mono audio delayed by %d: %.3g of its RMS" % (backend, D, rel))
    assert rel < BAR, rel


# ---- 4. switching --------------------------------------------------------------------------------------------------------------------------
def test_switching_follows_setstereo_and_reset(backend):
    """Case toggle: setStereo(false) in front of block 3, setStereo(true) in front of block 5, reset() in front of block 8.  Same bar over the whole stream and
    over the first 159 + 317 frames behind every switch on their own (against the RMS of the whole reference); same frame counts.
    Measured over the stereo stretches (l, r, l - r): emulator 1.86e-7, 2.74e-7, 2.61e-7; MI355X 1.92e-7, 2.80e-7, 2.69e-7."""
    z = gold()
    out = run_case("toggle")
    cut = [int(n) for n in z["toggle_cut"]]
    assert [len(o) for o in out] == cut
    got, want = np.concatenate(out), z["toggle_audio"]
    on = np.repeat(z["toggle_stereo"], cut).astype(bool)
    for k in (0, 1):
        assert rms(got[:, k] - want[:, k]) < BAR * rms(want[:, k]), k
    gd, wd = got[:, 0] - got[:, 1], want[:, 0] - want[:, 1]
    assert rms((gd - wd)[on]) < BAR * rms(wd[on])
    assert np.array_equal(got[~on, 0], got[~on, 1]) and np.any(~on)  # switched off: two copies of L + R
    print("[stereo] %s toggle: l %.3g r %.3g l-r %.3g" % ((backend,) + distances(got[on], want[on])))
    starts = np.cumsum([0] + cut)
    for b in np.nonzero(z["toggle_ops"])[0]:
        w = slice(int(starts[b]), int(starts[b]) + D + 317)
        for k in (0, 1):
            assert rms(got[w, k] - want[w, k]) < BAR * rms(want[:, k]), (int(b), k)
        # the demodulator really started over there: the frames in front of the first full window differ from a run without the operation
    through = np.concatenate(run_case("toggle", ops=False))
    assert rms(through[starts[8]:starts[8] + D + 317] - want[starts[8]:starts[8] + D + 317]) > 100 * BAR * rms(want)


def test_the_same_description_again_changes_nothing(backend):
    """A call with the same description and the same `enabled` in the middle of a stream: bit-identical frames to a run without it."""
    from sdrplusplus_amd import radio

    x = case_x("steady")[:5000]
    runs = []
    for again in (False, True):
        ctx = make_ctx()
        vid = add_wfm(ctx)
        sd, skeep = radio.stereo_desc(IF_RATE)
        out = []
        for lo in range(0, len(x), 1250):
            if again:
                ctx.vfo_set_stereo(vid, sd, skeep)
            ctx.push(x[lo:lo + 1250])
            out.append(ctx.vfo_read(vid).copy())
        ctx.close()
        runs.append(np.concatenate(out))
    assert bits_equal(runs[0], runs[1])


# ---- 5. cuts, bit for bit ------------------------------------------------------------------------------------------------------------------
_one_push = {}


def one_push(backend):
    """case cuts in ONE push, once per backend, shared unchanged"""
    if backend not in _one_push:
        _one_push[backend] = np.concatenate(run_case("cuts", cut=[len(case_x("cuts"))]))
    return _one_push[backend]


@pytest.mark.parametrize("sizes", [[1250], [997, 7, 1], [100], [300]], ids=lambda s: "-".join(map(str, s)))
def test_cuts_give_identical_bits(backend, sizes):
    """One push against pushes of 1250, of 997 / 7 / 1, of 100 (shorter than the delay) and of 300 (shorter than the pilot filter): identical bits."""
    n = len(case_x("cuts"))
    got = np.concatenate(run_case("cuts", cut=schedule(n, sizes)))
    assert bits_equal(got, one_push(backend))


# ---- 6. bank shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nst", [1, 2, 3, PACK, PACK + 1])
def test_bank_shapes_bit_for_bit_per_vfo(backend, nst):
    """1, 2, 3, as many stereo VFOs as a loop job packs and one more, mixed with a mono WFM and an NFM VFO: every stereo VFO gives the bits of a bank of one, the mono and
    NFM VFOs those of the same bank with no stereo VFO.  (The stereo VFOs get the input with different block phases: VFO k runs with its low-pass on for even k.)"""
    x = case_x("cuts")[:4000]
    sched = schedule(len(x), [1250, 333])

    def run(stereos, others=True):
        ctx = make_ctx()
        ids = [add_wfm(ctx, low_pass=(k % 2 == 0)) for k in stereos]
        if others:
            ids += [add_wfm(ctx, stereo=False), add_wfm(ctx, stereo=False, mode="NFM")]
        outs, pos = [[] for _ in ids], 0
        for n in sched:
            ctx.push(x[pos:pos + n])
            pos += n
            for o, v in zip(outs, ids):
                o.append(ctx.vfo_read(v).copy())
        ctx.close()
        return [np.concatenate(o) for o in outs]

    bank = run(range(nst))
    single = {k: run([k], others=False)[0] for k in (0, 1)}
    plain = run([])
    for k in range(nst):
        assert bits_equal(bank[k], single[k % 2]), k
    assert bits_equal(bank[nst], plain[0]) and bits_equal(bank[nst + 1], plain[1])
    assert not np.array_equal(bank[0][:, 0], bank[0][:, 1])


# ---- 7. modes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 4])
def test_pipelined_and_grouped_equal_the_ordinary_pass(backend, group):
    """Two stereo VFOs (one without low-pass), a mono WFM and an NFM VFO: every ticket's frames equal the ordinary pass's of that push bit for bit, with
    results delivered and no block run as an ordinary pass; the role list is still the 54 names ending in `ifc`, whose role ran."""
    from sdrplusplus_amd import capi

    x = case_x("cuts")[:6000]
    sched = schedule(len(x), [1250, 400, 1250, 7])

    def bank(ctx):
        return [add_wfm(ctx), add_wfm(ctx, low_pass=False), add_wfm(ctx, stereo=False), add_wfm(ctx, stereo=False, mode="NFM")]

    ctx = make_ctx()
    ids = bank(ctx)
    want, pos = [], 0
    for n in sched:
        ctx.push(x[pos:pos + n])
        pos += n
        want.append([ctx.vfo_read(v).copy() for v in ids])
    ctx.close()
    ctx = make_ctx()
    ids = bank(ctx)
    ctx.set_pipelined(True, 1)
    if group > 1:
        ctx.set_pipeline_group(group)
    before = ctx.pipeline_stats()["roles"].get("ifc", 0)
    pos = 0
    for n in sched:
        ctx.push(x[pos:pos + n])
        pos += n
    for i in range(len(sched)):
        res = ctx.result_wait(i + 1)
        for k, v in enumerate(ids):
            assert bits_equal(res["vfo"][v], want[i][k]), (i, k)
        ctx.result_release(i + 1)
    st = ctx.pipeline_stats()
    assert st["pass_blocks"] == 0 and st["roles"].get("ifc", 0) > before, st
    L = capi.load()
    L.sdrpp_pipeline_role_name.restype = C.c_char_p
    L.sdrpp_pipeline_role_name.argtypes = [C.c_int]
    roles = []
    while L.sdrpp_pipeline_role_name(len(roles)) is not None:
        roles.append(L.sdrpp_pipeline_role_name(len(roles)).decode())
    assert roles[-1] == "ifc" and len(roles) == 54, roles
    ctx.set_pipelined(False)
    ctx.close()


def test_a_bank_with_the_branch_off_plans_what_it_planned(backend):
    """A WFM VFO with the branch attached but switched off, and one it was detached from, give the bits of a VFO that never had one — through the same pass
    forms (the planner files no job of the branch)."""
    from sdrplusplus_amd import radio

    x = case_x("steady")[:5000]
    res, forms = [], []
    for how in ("never", "off", "detached"):
        ctx = make_ctx()
        vid = add_wfm(ctx, stereo=False)
        if how != "never":
            sd, skeep = radio.stereo_desc(IF_RATE, enabled=False)
            ctx.vfo_set_stereo(vid, sd, skeep)
        if how == "detached":
            ctx.vfo_set_stereo(vid, None)
        out = []
        for lo in range(0, len(x), 1250):
            ctx.push(x[lo:lo + 1250])
            out.append(ctx.vfo_read(vid).copy())
        res.append(np.concatenate(out))
        forms.append({k: v for k, v in ctx.pass_form_stats().items() if v})
        ctx.close()
    assert bits_equal(res[0], res[1]) and bits_equal(res[0], res[2])
    assert forms[0] == forms[1] == forms[2], forms


# ---- 8. behind it --------------------------------------------------------------------------------------------------------------------------
def test_af_chain_and_recorder_behind_the_branch(backend):
    """With the AF chain attached (250 kS/s -> 48 kS/s, de-emphasis 50 us) each channel of the AF output is within the project's RMS bar (1e-5, as
    tests/test_af_chain.py keeps it) of the oracle's AF chain fed the FIXTURE's audio, and within test_af_chain's per-sample bar — MARGIN x the oracle chain's
    own float32 distance from a float64 restatement, both fed the device's frames — per channel.  The recorder sink's mono fold of the stereo blocks is
    bit-exact by test_recorder's rule: a function of the frames the library delivers for the same block."""
    from sdrplusplus_amd import capi, radio
    from test_af_chain import af_parts, restate_af64
    from test_kernel_forms import BASELINE_MAX, MARGIN, dist
    from test_parity_vfo import _OracleAf
    from test_recorder import assert_same, restate

    z = gold()
    x, ref = case_x("steady"), z["steady_audio"]
    ctx = make_ctx()
    vid = add_wfm(ctx)
    af, akeep = radio.af_desc(IF_RATE, 48000.0, 50e-6)
    ctx.vfo_set_af(vid, af, akeep)
    ctx.vfo_set_rec(vid, 0.8, True, capi.REC_FLOAT32, False)
    dem, got = [], []
    for lo in range(0, len(x), 1250):
        ctx.push(x[lo:lo + 1250])
        dem.append(ctx.vfo_read(vid).copy())
        got.append(ctx.vfo_af_read(vid).copy())
        assert_same(ctx.vfo_rec_read(vid), restate(got[-1], 0.8, True, capi.REC_FLOAT32, False), ("push", lo))
    ctx.close()
    dem, got = np.concatenate(dem), np.concatenate(got)
    want = _OracleAf(IF_RATE, 48000.0, 50e-6, False).process(ref)
    own = _OracleAf(IF_RATE, 48000.0, 50e-6, False).process(dem)
    assert len(want) == len(got) == len(own) > 2000
    assert not np.array_equal(got[:, 0], got[:, 1])
    parts = af_parts(af)
    for k in (0, 1):
        rel = rms(got[:, k] - want[:, k]) / rms(want[:, k])
        r64 = restate_af64(parts, dem[:, k])
        base, e = dist(own[:, k], r64), dist(got[:, k], r64)
        print("[stereo] %s AF channel %d: %.3g of the oracle chain's RMS; per sample %.3g against a baseline of %.3g" % (backend, k, rel, e, base))
        assert rel < BAR, (k, rel)
        assert base < BASELINE_MAX and e <= MARGIN * base, (k, e, base)


# ---- 9. errors, reset, replace -------------------------------------------------------------------------------------------------------------
def test_argument_checks(backend):
    from sdrplusplus_amd import capi, radio

    ctx = make_ctx()
    wfm = add_wfm(ctx, stereo=False)
    nfm = add_wfm(ctx, stereo=False, mode="NFM")
    raw = add_wfm(ctx, stereo=False, mode="RAW")
    sd, skeep = radio.stereo_desc(IF_RATE)
    call = lambda v, d: ctx.L.sdrpp_vfo_set_stereo(ctx.h, v, C.byref(d) if d is not None else None)  # noqa: E731
    assert call(nfm, sd) == UNSUPPORTED and call(raw, sd) == UNSUPPORTED
    assert call(12345, sd) == -6
    for field, value in (("pilot_ntaps", 0), ("pilot_ntaps", 316), ("pilot_ntaps", -3), ("delay", 0), ("delay", -159)):
        bad, _ = radio.stereo_desc(IF_RATE)
        setattr(bad, field, value)
        assert call(wfm, bad) == INVALID, (field, value)
    bad, _ = radio.stereo_desc(IF_RATE)
    bad.pilot_taps = None
    assert call(wfm, bad) == INVALID
    bad, _ = radio.stereo_desc(IF_RATE)
    bad.min_freq, bad.max_freq = bad.max_freq, bad.min_freq
    assert call(wfm, bad) == INVALID
    # the loop's description: everything finite, the limits an interval within +-pi, a phase step the wrap ends on (include/sdrpp_gpu.h)
    inf, pi = float("inf"), float(np.pi)
    for field, value in (("alpha", inf), ("alpha", -inf), ("alpha", 1e9), ("alpha", float("nan")), ("alpha", 4.0), ("beta", inf), ("beta", float("nan")),
                         ("max_freq", inf), ("max_freq", 1e30), ("max_freq", 3.2), ("min_freq", -inf), ("min_freq", -3.2), ("min_freq", float("nan")),
                         ("init_freq", inf), ("init_freq", 4.0), ("init_freq", float("nan"))):
        bad, _ = radio.stereo_desc(IF_RATE)
        setattr(bad, field, value)
        assert call(wfm, bad) == INVALID, (field, value)
    ok, _ = radio.stereo_desc(IF_RATE)
    ok.alpha, ok.min_freq, ok.max_freq, ok.enabled = 2.9, -3.0, 3.0, 0  # (just inside: 2.9 pi + 3 <= 4 pi)
    assert call(wfm, ok) == 0 and call(wfm, None) == 0
    long_taps = np.zeros(2 * 577, np.float32)
    bad, _ = radio.stereo_desc(IF_RATE)
    bad.pilot_taps, bad.pilot_ntaps = long_taps.ctypes.data_as(capi.c_float_p), 577
    assert call(wfm, bad) == UNSUPPORTED
    # nothing of that left a branch behind: the VFO still delivers mono frames; then the real thing, then a detach
    x = case_x("steady")[:2500]
    ctx.push(x[:1250])
    a = ctx.vfo_read(wfm)
    assert np.array_equal(a[:, 0], a[:, 1])
    assert call(wfm, sd) == 0
    ctx.push(x[1250:])
    b = ctx.vfo_read(wfm)
    assert not np.array_equal(b[:, 0], b[:, 1])
    assert call(wfm, None) == 0 and call(wfm, None) == 0
    ctx.push(x[:1250])
    a2 = ctx.vfo_read(wfm)
    assert bits_equal(a, a2)  # (a detach of a running branch is a switch: the demodulator started over, so the first block's bits again)
    ctx.close()


def test_reset_and_replace(backend):
    """sdrpp_vfo_reset clears the branch with the rest of the demodulator: the stream again gives the bits of a fresh VFO.  sdrpp_vfo_replace with keep & 2 and
    the same description moves parameters and state: the frames continue bit for bit; without the bit the new handle is mono."""
    from sdrplusplus_amd import radio

    x = case_x("steady")[:5000]
    ctx = make_ctx()
    vid = add_wfm(ctx)
    out = []
    for lo in range(0, 5000, 1250):
        ctx.push(x[lo:lo + 1250])
        out.append(ctx.vfo_read(vid).copy())
    fresh = np.concatenate(out)
    ctx.vfo_reset(vid)
    out = []
    for lo in range(0, 2500, 1250):
        ctx.push(x[lo:lo + 1250])
        out.append(ctx.vfo_read(vid).copy())
    assert bits_equal(np.concatenate(out), fresh[:2500])
    d, keep = radio.vfo_desc(IF_RATE, IF_RATE, IF_RATE, 0.0, "WFM")
    d.inv_deviation = np.float32(1.0 / radio.hz_to_rads(75000.0, IF_RATE))
    new = ctx.vfo_replace(vid, d, 3, keep)
    out = []
    for lo in range(2500, 5000, 1250):
        ctx.push(x[lo:lo + 1250])
        out.append(ctx.vfo_read(new).copy())
    assert bits_equal(np.concatenate(out), fresh[2500:])
    new2 = ctx.vfo_replace(new, d, 1, keep)
    ctx.push(x[:1250])
    m = ctx.vfo_read(new2)
    assert np.array_equal(m[:, 0], m[:, 1])
    ctx.close()


def test_replace_with_another_audio_filter_starts_from_the_reset_state(backend):
    """sdrpp_vfo_replace with keep & 2 onto a handle whose audio filter has another length (low-pass off): the branch's streams do not fit, the description is
    attached afresh and the demodulator starts over as a whole — the new handle gives the bits of a fresh VFO with that description fed the same samples."""
    from sdrplusplus_amd import radio

    x = case_x("steady")[:3750]
    ctx = make_ctx()
    vid = add_wfm(ctx)
    ctx.push(x[:1250])
    d, keep = radio.vfo_desc(IF_RATE, IF_RATE, IF_RATE, 0.0, "WFM", low_pass=False)
    d.inv_deviation = np.float32(1.0 / radio.hz_to_rads(75000.0, IF_RATE))
    new = ctx.vfo_replace(vid, d, 3, keep)
    fresh = add_wfm(ctx, low_pass=False)
    for lo in (1250, 2500):
        ctx.push(x[lo:lo + 1250])
        a, b = ctx.vfo_read(new), ctx.vfo_read(fresh)
        assert len(a) == 1250 and not np.array_equal(a[:, 0], a[:, 1])
        assert bits_equal(a, b), lo
    ctx.close()


def test_switching_leaves_the_rds_branch_alone(backend):
    """A VFO that carries the RDS branch and the stereo branch: setStereo(false) in front of block 2 and setStereo(true) in front of block 3 clear what the
    demodulator reads, and the RDS branch keeps its own state.  Its baseband equals, bit for bit, that of a VFO WITHOUT a stereo branch whose demodulator is
    reset at the same two places (sdrpp_vfo_reset: the same one discriminator value differs, as in the reference, where setStereo calls reset()); and once that
    value has left the branch's filters (5 052 IF samples: 44 + 8 x 11 + 16 x 68 + 32 x 119 taps' reach), bit for bit that of a VFO nothing was done to."""
    from sdrplusplus_amd import radio

    x = case_x("steady")
    rd, rkeep = radio.rds_desc(IF_RATE)
    sd, skeep = radio.stereo_desc(IF_RATE)
    runs = {}
    for how in ("stereo", "reset", "untouched"):
        ctx = make_ctx()
        vid = add_wfm(ctx, stereo=(how == "stereo"))
        ctx.vfo_set_rds(vid, rd, True, rkeep)
        out = []
        for b, lo in enumerate(range(0, len(x), 1250)):
            if b in (2, 3):
                if how == "stereo":
                    sd.enabled = int(b == 3)
                    ctx.vfo_set_stereo(vid, sd, skeep)
                elif how == "reset":
                    ctx.vfo_reset(vid)
            ctx.push(x[lo:lo + 1250])
            out.append(ctx.vfo_rds_read(vid).copy())
        ctx.close()
        runs[how] = out
    assert [len(o) for o in runs["stereo"]] == [len(o) for o in runs["untouched"]] and sum(len(o) for o in runs["stereo"]) >= 250
    for b in range(len(runs["stereo"])):
        assert bits_equal(runs["stereo"][b], runs["reset"][b]), b
    for b in (0, 1, 8, 9):  # in front of the first switch, and from 3 750 + 5 052 samples on
        assert bits_equal(runs["stereo"][b], runs["untouched"][b]), b
