"""The FFT roles of the tick as they walk their tiles: pass 1 takes the tiles of its columns from consecutive frames with the window values and
inter-pass twiddles of those columns in registers, pass 2 takes PAIRS of adjacent row tiles of one frame and stores both tiles' dB values
together.  Neither changes an arithmetic operation, so every comparison is bit-exact (`array_equal`): raw dB lines, the group maxima as the zoomed
lines show them (views of >= 2 groups per pixel) and the palette indices — against the oracle, and pipelined against ordinary passes of the same
pushes.  Runs on the real device under `-m gpu` and on the CPU fiber emulator of the same kernel sources otherwise.

Shapes: the smallest at which the walks can go wrong.  N = 2^13 has two row tiles per frame, i.e. exactly one pair; 2^14 .. 2^16 two, four and
eight pairs (2^16 is the headline's transform).  Pushes of 1, 2, 3 (and for the small sizes 4) frames: a single tile, a pair of frames for pass
1, an odd one left over; no push is a multiple of N, so frames begin in the history of the previous push and take the general loader."""
import functools

import numpy as np
import pytest

import support as S

LO, HI = -110.0, -15.0


def _view(N):
    """ragged at both ends, >= 2 doZoom groups of the widest kind (32 bins) per pixel at every size: the pixels read pass 2's group maxima"""
    return (3, N - 5, 61, LO, HI)


def _signal(n, seed):
    r = np.random.default_rng(seed)
    t = np.arange(n)
    x = (r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.01 + 0.3 * np.exp(2j * np.pi * 0.1003 * t) + 1e-3 * np.exp(-2j * np.pi * 0.31 * t)
    return x.astype(np.complex64)


def _geometry(lg):
    """(tiles of pass 1 per frame, pairs of pass 2 per frame, role names) of a 2^lg-point transform: fft_split and the launch tables of plan_fft.h"""
    lg1 = lg // 2 if lg <= 16 else lg - 12
    lg2 = lg - lg1
    cols = {5: 128, 6: 64, 7: 32, 8: 16, 9: 8, 10: 4}[lg1]
    p1 = (1 << lg2) // cols
    if lg2 == 12:
        return p1, None, ("fft_p1_%d" % lg1, None)
    rows = {7: 32, 8: 16, 9: 8, 10: 4}[lg2]
    return p1, ((1 << lg1) // rows) // 2, ("fft_p1_%d" % lg1, "fft_p2_%d" % lg2)


def _walk_grid(units, per_frame, cap):
    """plan_fft.h: fft_walk_grid"""
    if cap <= 0 or units <= cap:
        return units
    return max(per_frame, (cap // per_frame) * per_frame)


@functools.lru_cache(maxsize=None)
def _case(lg, padded, nframes):
    """signal, pushes, framing and the oracle's lines / zoomed lines / indices per push: computed once, shared, read only"""
    from sdrplusplus_amd import capi

    N = 1 << lg
    nz, skip = (N - 1000, 37) if padded else (N, 0)
    stride = nz + skip
    tails = [11, 5, -7, 3]
    pushes = [(nz if i == 0 else f * stride) + tails[i] for i, f in enumerate(nframes)]
    w = capi.design_fft_window(2, nz)
    x = _signal(sum(pushes), lg)
    sp = S.OracleSpectrum(N, nz, skip, w)
    want, pos = [], 0
    for n, f in zip(pushes, nframes):
        ol = sp.push(x[pos:pos + n])
        pos += n
        assert len(ol) == f, (len(ol), f)
        oz = np.stack([S.oracle_do_zoom(_view(N)[0], _view(N)[1], _view(N)[2], l) for l in ol])
        oi = np.stack([S.oracle_palette_index(z, LO, HI) for z in oz])
        for a in (ol, oz, oi):
            a.setflags(write=False)
        want.append((ol, oz, oi))
    x.setflags(write=False)
    return x, tuple(pushes), (N, nz, skip, w), tuple(want)


def _ctx(case):
    from sdrplusplus_amd import capi

    _, pushes, (N, nz, skip, w), _ = case
    ctx = capi.Context(0, max_push=sum(pushes))
    ctx.fft_configure(N, nz, skip, w)
    ctx.fft_set_view(*_view(N))
    return ctx


_ORDINARY = {}


def _ordinary(backend, key, case):
    """ordinary passes of the case's pushes (stand-alone kernels: single row tiles, twiddles fetched in the store loop), once per backend"""
    if (backend, key) not in _ORDINARY:
        x, pushes, _, _ = case
        ctx = _ctx(case)
        got, pos = [], 0
        for n in pushes:
            ctx.push(x[pos:pos + n])
            pos += n
            got.append(ctx.fft_read())
        ctx.close()
        _ORDINARY[(backend, key)] = got
    return _ORDINARY[(backend, key)]


def _check(got, want, ordinary, what):
    for name, g, o, p in zip(("raw", "zoomed", "index"), (got["raw"], got["zoomed"], got["index"]), want, ordinary):
        assert g.shape == o.shape == p.shape, (what, name, g.shape, o.shape, p.shape)
        assert np.array_equal(g, o), (what, name, "differs from the oracle")
        assert np.array_equal(g, p), (what, name, "differs from the ordinary pass")


def _run_pipelined(case, ordinary, group=1):
    x, pushes, _, want = case
    ctx = _ctx(case)
    ctx.set_pipelined(True, 2 | 4)
    if group > 1:
        ctx.set_pipeline_group(group)
    pos = 0
    for n in pushes:
        ctx.push(x[pos:pos + n])
        pos += n
    for t in range(1, len(pushes) + 1):
        got = ctx.result_wait(t)
        _check(got, want[t - 1], ordinary[t - 1], "push %d" % t)
        ctx.result_release(t)
    st = ctx.pipeline_stats()
    gs = ctx.pipeline_group_stats() if group > 1 else None
    ctx.close()
    assert st["pass_blocks"] == 0, st
    return st, gs


# cap on the workgroups of a role, in pass-1 tiles per frame (P1; pass 2 has P1 / 2 pairs per frame): None = the default rule; 1 -> pass 1 walks every frame of
# the push (1, 2, 3, 4 tiles), pass 2 two frames' pairs (two pairs and, with an odd frame left over, one); 2 (+ 1: a cap that is no multiple of the
# tiles per frame) -> pass 1 walks two frames' tiles (2 and 1 tiles at three frames: the grid does not divide the tile count), pass 2 single pairs
@pytest.mark.parametrize("cap", [None, 1, 2])
@pytest.mark.parametrize("lg", [13, 14, 15, 16])
def test_walks_of_one_two_and_four_tiles(backend, lg, cap, monkeypatch):
    nframes = (1, 2, 3, 4) if lg <= 14 else (1, 2, 3)
    case = _case(lg, False, nframes)
    ordinary = _ordinary(backend, (lg, False, nframes), case)
    p1, p2, (n1, n2) = _geometry(lg)
    grid = 0
    if cap is not None:
        grid = cap * p1 + (1 if cap == 2 else 0)
        monkeypatch.setenv("SDRPP_GPU_FFT_TICK_GRID", str(grid))
    else:
        monkeypatch.delenv("SDRPP_GPU_FFT_TICK_GRID", raising=False)
    st, _ = _run_pipelined(case, ordinary)
    if cap is not None:  # the walk is the one this case is about: workgroups launched per role over the pushes
        assert st["roles"][n1] == sum(_walk_grid(f * p1, p1, grid) for f in nframes), st["roles"]
        assert st["roles"][n2] == sum(_walk_grid(f * p2, p2, grid) for f in nframes), st["roles"]
    else:  # whatever the default walk is, pass 2 counts pairs: never more workgroups than half the row tiles
        assert st["roles"][n2] <= sum(f * p2 for f in nframes), st["roles"]


@pytest.mark.parametrize("lg", [13, 15])
def test_zero_padded_framing_walks(backend, lg, monkeypatch):
    """nz < N with samples skipped between frames: no frame takes the lean loader, the padded inputs are zero whatever the window register holds; walked
    (pass 1 every frame of a push, pass 2 two pairs and one) and by the default rule"""
    case = _case(lg, True, (1, 2, 3))
    ordinary = _ordinary(backend, (lg, True, (1, 2, 3)), case)
    monkeypatch.delenv("SDRPP_GPU_FFT_TICK_GRID", raising=False)
    _run_pipelined(case, ordinary)
    monkeypatch.setenv("SDRPP_GPU_FFT_TICK_GRID", str(_geometry(lg)[0]))
    _run_pipelined(case, ordinary)


@pytest.mark.parametrize("lg", [13, 16])
def test_two_blocks_in_one_launch_group(backend, lg, monkeypatch):
    """two pushes (1 + 2 frames) go out as ONE launch: every push keeps its own lines"""
    monkeypatch.setenv("SDRPP_GPU_FFT_TICK_GRID", str(_geometry(lg)[0]))
    case = _case(lg, False, (1, 2))
    ordinary = _ordinary(backend, (lg, False, (1, 2)), case)
    _, gs = _run_pipelined(case, ordinary, group=2)
    assert gs["largest"] == 2, gs


def test_long_transform_shares_pass_one(backend, monkeypatch):
    """N = 2^17: pass 1 (32-point columns, the same body with its twiddles in registers) feeds the 4096-point row pass and the transpose, which are
    untouched; the second frame begins in the history"""
    monkeypatch.delenv("SDRPP_GPU_FFT_TICK_GRID", raising=False)
    case = _case(17, False, (1, 1))
    ordinary = _ordinary(backend, (17, False, (1, 1)), case)
    st, _ = _run_pipelined(case, ordinary)
    assert st["roles"]["fft_p1_5"] >= 1 and st["roles"]["fft_p2row"] == 2 * 32 and "fft_p2_7" not in st["roles"], st["roles"]
