"""The M17 decoder's front through the C++ host blocks (sdrpp_gpu::M17FrameSource in sdrplusplus_amd/host/sdrpp_gpu_m17.h over RxVFO::attachM17):
tests/host_cpp/test_m17.cpp on the stand-alone dsp::stream double, fed with a case of tests/golden/m17_ref.npz in the fixture's own blocks.  The four streams of
the frame demux must carry the reference's recorded frames — every entry, with the reference's swap counts (368 on linkSetupOut; 96 on lichOut, then 368 on
streamOut / packetOut, whose 96 trailing entries are zero here) — and `diagOut` the reference's symbols per block, through a stop / start in mid-stream, in
ordinary and in pipelined mode.  The soft symbols themselves are the C-ABI's for the same blocks, bit for bit."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_m17 import GOLDEN, RATE, bits_equal, case_input

ROOT = S.ROOT
CASE, B = "aligned_noise", 600


def _capi_soft(x, nblk, lib):
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        d, keep = radio.vfo_desc(RATE, RATE, RATE, 0.0, "RAW")
        vid = ctx.vfo_add(d, keep)
        sd, fd, mk = radio.m17_desc(RATE)
        ctx.vfo_set_symbols(vid, sd, True, mk)
        out = []
        for k in range(nblk):
            ctx.push(x[k * B:(k + 1) * B])
            out.append(ctx.vfo_sym_read(vid)[0])
        ctx.close()
        return out
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, mode, wait_ms, lib):
    z = np.load(GOLDEN)
    x = case_input(z, CASE)
    assert list(z[CASE + "_cut"][:-1]) == [B] * (len(z[CASE + "_cut"]) - 1)
    nblk = len(x) // B  # (whole blocks: the fixture's last, shorter block carries no frame)
    assert all(b < nblk for b in z[CASE + "_fblock"]) and len(z[CASE + "_ftype"]) == 5
    x[:nblk * B].view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(RATE), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % nblk in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    ftype, frames = z[CASE + "_ftype"], z[CASE + "_frames"]
    pad = lambda f: np.concatenate([f[96:], np.zeros(96, np.uint8)])  # noqa: E731
    want = dict(ls=[f for t, f in zip(ftype, frames) if t == 0], lich=[f[:96] for t, f in zip(ftype, frames) if t != 0],
                stream=[pad(f) for t, f in zip(ftype, frames) if t == 1], packet=[pad(f) for t, f in zip(ftype, frames) if t == 2])
    assert [len(want[k]) for k in ("ls", "lich", "stream", "packet")] == [1, 4, 3, 1]
    for name, per in (("ls", 368), ("lich", 96), ("stream", 368), ("packet", 368)):
        assert ld(name + "_counts.i32", np.int32).tolist() == [per] * len(want[name]), (name, rr.stdout)   # the reference's swap counts, a swap per frame
        assert np.array_equal(ld(name + ".u8", np.uint8), np.concatenate(want[name])), name               # ... and every entry
    assert ld("diag_counts.i32", np.int32).tolist() == list(z[CASE + "_counts"][:nblk]), rr.stdout          # the reference's symbols per block on diagOut
    assert bits_equal(ld("diag.f32", np.float32), np.concatenate(_capi_soft(x, nblk, lib)))
    assert len(ld("audio_counts.i32", np.int32)) == nblk, rr.stdout                                        # nothing lost on the radio beside it


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_m17_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_m17.cpp"), tmp, mode, 60000, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_m17_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_m17.cpp"), tmp, mode, 20000, "gpu")
