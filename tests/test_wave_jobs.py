"""Every kind of wavefront job of the tick's `ifc` role in ONE bank, so that jobs of different kinds share workgroups and levels: noise blanker / squelch, FMIF
segments, the RDS branch's front, reference rotator and line splice, the stereo branch's pilot, loop and matrix.

250 kS/s fed straight in (no decimator), pushes of 120, 1024, 700, 1 and 1155 samples: less than one FMIF segment (256), exactly four FMIF segments which is one
stereo segment (1024), one sample, and ragged multi-segment blocks.  The reference block is 300 samples, so the squelch and the RDS reference rotator see several
blocks in the longer pushes.  The VFOs:
  (a) RAW with blanker + squelch + 32-bin FMIF, over spikes;
  (b) WFM with the stereo branch and the closed-form RDS branch;
  (c) WFM under nco_mode 2 with the RDS branch (reference rotator) and the squelch alone (at a level that closes every block without a spike);
  (d) WFM stereo behind blanker + FMIF;
  (e) WFM whose RDS branch is switched off and on again before the 120-sample push and before the 1-sample push: the first decimator reads the set-aside line,
      and the one-sample block, shorter than that decimator's 44 taps, is spliced onto it by the line job.
Legs: ordinary passes, pipelined, pipelined in launch groups of 4.  Every output of every VFO (audio or the RAW VFO's chain output, the IF chain's output, the RDS
samples) is bit-equal to the same VFO alone in its own context over the same pushes in each leg, and the pipelined legs are bit-equal to the ordinary one (what
test_ifchain, test_fmif, test_rds and test_stereo_rows each claim for their own kind).  Equality only: no tolerance anywhere."""
import numpy as np
import pytest

from conftest import BACKENDS  # noqa: F401  (the `backend` fixture lives in conftest)
from test_ifchain import _ctx
from test_kernel_forms import _bits_equal
from test_stereo_rows import RATE, job, make_cfg, signal, stereo_desc_of, wfm_desc

PUSHES = [120, 1024, 700, 1, 1155]
REF_BLOCK = 300
SPIKES = [(i, 0.9 + 0.3j) for i in (60, 500, 1500, 1501, 2400, 2900)]
GROUP = 4
RESULT_VFO, RESULT_RDS = 1, 32


def _raw(ctx):
    from sdrplusplus_amd import radio

    d, keep = wfm_desc(job(None), RATE, raw=True)
    vid = ctx.vfo_add(d, keep)
    ctx.vfo_set_if(vid, radio.if_desc(RATE, nb=True, nb_level=10.0, squelch=-30.0))
    ctx.vfo_set_fmnr(vid, True, 32)
    return vid


def _wfm(ctx, stereo=False, rds=False, nco_mode=0, ifd=None, fmnr=False):
    from sdrplusplus_amd import radio

    cfg = make_cfg()
    d, keep = wfm_desc(job(cfg), RATE)
    d.nco_mode = nco_mode
    vid = ctx.vfo_add(d, keep)
    if ifd is not None:
        ctx.vfo_set_if(vid, ifd)
    if fmnr:
        ctx.vfo_set_fmnr(vid, True, 32)
    if stereo:
        ctx.vfo_set_stereo(vid, *stereo_desc_of(cfg))
    if rds:
        rd, rkeep = radio.rds_desc(RATE)
        ctx.vfo_set_rds(vid, rd, True, rkeep)
    return vid


def _switch_rds(ctx, vid):
    from sdrplusplus_amd import radio

    rd, rkeep = radio.rds_desc(RATE)
    assert rd.stage_ntaps[0] > 1, "the one-sample push must be shorter than the RDS branch's first decimator"
    ctx.vfo_set_rds(vid, rd, False, rkeep)
    ctx.vfo_set_rds(vid, rd, True, rkeep)


def _if(**kw):
    from sdrplusplus_amd import radio

    return radio.if_desc(RATE, **kw)


# name -> (attach(ctx) -> id, the IF chain's output exists, the RDS branch's output exists, pushes in front of which the RDS branch is switched off and on)
VFOS = {
    "a_raw_nb_sq_fmif": (_raw, True, False, ()),
    "b_stereo_rds": (lambda ctx: _wfm(ctx, stereo=True, rds=True), False, True, ()),
    "c_rotator_rds_sq": (lambda ctx: _wfm(ctx, rds=True, nco_mode=2, ifd=_if(squelch=-12.1)), True, True, ()),
    "d_stereo_nb_fmif": (lambda ctx: _wfm(ctx, stereo=True, ifd=_if(nb=True, nb_level=10.0, squelch=-150.0), fmnr=True), True, False, ()),
    "e_rds_splice": (lambda ctx: _wfm(ctx, rds=True), False, True, (0, 3)),
}


def run(x, names, pipelined=False, group=0):
    """-> ({name: dict(out, ifc, rds)} with every push's samples in a row, pass forms, pipeline stats)"""
    ctx = _ctx(sum(PUSHES), REF_BLOCK)
    vids = {n: VFOS[n][0](ctx) for n in names}
    if pipelined:
        ctx.set_pipelined(True, RESULT_VFO | RESULT_RDS)
        if group:
            ctx.set_pipeline_group(group)
    got = {n: dict(out=[], ifc=[], rds=[]) for n in names}
    before = ctx.pipeline_stats()["roles"].get("ifc", 0)
    pos = 0
    for k, c in enumerate(PUSHES):
        for n in names:
            if k in VFOS[n][3]:
                _switch_rds(ctx, vids[n])
        ctx.push(x[pos:pos + c])
        pos += c
        if not pipelined:
            for n in names:
                got[n]["out"].append(ctx.vfo_read(vids[n]).copy())
                if VFOS[n][1]:
                    got[n]["ifc"].append(np.array(ctx.vfo_ifc_read(vids[n])).view(np.float32).reshape(-1))
                if VFOS[n][2]:
                    got[n]["rds"].append(np.array(ctx.vfo_rds_read(vids[n])).view(np.float32).reshape(-1))
    if pipelined:
        for k in range(1, len(PUSHES) + 1):
            res = ctx.result_wait(k)
            for n in names:
                got[n]["out"].append(res["vfo"][vids[n]].copy())
                if VFOS[n][2]:
                    got[n]["rds"].append(np.array(ctx.result_rds(k, vids[n])).view(np.float32).reshape(-1))
            ctx.result_release(k)
    forms, st = ctx.pass_form_stats(), ctx.pipeline_stats()
    st["ifc_grew"] = st["roles"].get("ifc", 0) - before
    if pipelined:
        ctx.set_pipelined(False)
    ctx.close()
    for n in names:
        for q in ("out", "ifc", "rds"):
            got[n][q] = np.concatenate([np.ascontiguousarray(a, np.float32).reshape(-1) for a in got[n][q]]) if got[n][q] else None
    return got, forms, st


_x = []
_ordinary = {}


def _input():
    if not _x:
        x = signal(sum(PUSHES), seed=11, spikes=SPIKES)
        x.setflags(write=False)
        _x.append(x)
    return _x[0]


def _ordinary_bank(backend):
    """the bank in ordinary passes: run once per backend, shared and left unchanged"""
    if backend not in _ordinary:
        got, forms, st = run(_input(), list(VFOS))
        for v in got.values():
            for a in v.values():
                if a is not None:
                    a.setflags(write=False)
        _ordinary[backend] = (got, forms, st)
    return _ordinary[backend]


def _same(a, b, what):
    for n in a:
        for q in ("out", "ifc", "rds"):
            assert (a[n][q] is None) == (b[n][q] is None), (what, n, q)
            if a[n][q] is not None:
                _bits_equal(a[n][q], b[n][q], "%s: %s %s" % (what, n, q))


@pytest.mark.parametrize("leg", ["ordinary", "pipelined", "grouped"])
def test_every_kind_in_one_bank_equals_each_vfo_alone(backend, leg):
    x = _input()
    piped, group = leg != "ordinary", GROUP if leg == "grouped" else 0
    plain, forms0, _ = _ordinary_bank(backend)
    bank, forms, st = (plain, forms0, None) if not piped else run(x, list(VFOS), True, group)
    n_if = sum(PUSHES)
    for n, (_, has_ifc, has_rds, _sw) in VFOS.items():
        assert len(bank[n]["out"]) == 2 * n_if, (n, len(bank[n]["out"]))
        if has_ifc and not piped:
            assert len(bank[n]["ifc"]) == 2 * n_if, (n, len(bank[n]["ifc"]))
        if has_rds:
            assert len(bank[n]["rds"]) >= 2 * (n_if // 50 - 1), (n, len(bank[n]["rds"]))
    for n in VFOS:
        one, _, _ = run(x, [n], piped, group)
        _same({n: bank[n]}, one, "%s: in the bank vs alone in its context" % leg)
    if piped:
        want = {n: dict(plain[n], ifc=None) for n in plain}  # (a result holds no IF-chain output beside the audio: the RAW VFO's output IS its chain's)
        _same(want, bank, "%s vs ordinary passes" % leg)
        assert st["pass_blocks"] == 0 and st["tick_blocks"] == len(PUSHES) and st["ifc_grew"] > 0 and not forms, (st, forms)
    else:
        assert forms.get("ifc", 0) >= len(PUSHES), forms
        # what the inputs are for: the blanker and FMIF change the stream, the squelch of (c) closes blocks and leaves those with a spike open
        a, c = plain["a_raw_nb_sq_fmif"], plain["c_rotator_rds_sq"]
        assert not np.array_equal(a["ifc"], x.view(np.float32)) and np.array_equal(a["ifc"], a["out"])
        zero = ~np.any(c["ifc"].reshape(-1, 2) != 0, axis=1)
        assert 0 < int(zero.sum()) < n_if and np.array_equal(c["ifc"].reshape(-1, 2)[~zero], x.view(np.float32).reshape(-1, 2)[~zero]), int(zero.sum())
