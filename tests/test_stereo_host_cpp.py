"""The WFM demodulator's stereo decoder through the C++ host blocks (sdrpp_gpu::FusedDemodulator<.., WFM>::setStereo, RxVFO::setStereo):
tests/host_cpp/test_stereo.cpp.  getOutput() must carry the `steady` case's frames of tests/golden/stereo_ref.npz — the reference's own BroadcastFM — within the
bar of tests/test_stereo.py (1e-5 of the reference's RMS per channel and for l - r), one swap per block, nothing lost or doubled."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_stereo import BAR, case_x, distances, gold

ROOT = S.ROOT
B = 1250


def _run_and_check(exe, tmp, mode, wait_ms):
    x, want = case_x("steady"), gold()["steady_audio"]
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    nblk = len(x) // B
    assert "blocks %d" % nblk in rr.stdout
    got = np.fromfile(os.path.join(tmp, "audio.f32"), np.float32).reshape(-1, 2)
    counts = np.fromfile(os.path.join(tmp, "counts.i32"), np.int32)
    assert counts.tolist() == [B] * nblk, rr.stdout
    dl, dr, dd = distances(got, want)
    print("[stereo C++] %s: l %.3g r %.3g l-r %.3g of the reference's RMS" % (mode, dl, dr, dd))
    assert dl < BAR and dr < BAR and dd < BAR, (dl, dr, dd)


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_stereo_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_stereo.cpp"), tmp, mode, 60000)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_stereo_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_stereo.cpp"), tmp, mode, 20000)
