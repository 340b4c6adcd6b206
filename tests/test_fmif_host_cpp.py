"""FMIF through the C++ host blocks (sdrpp_gpu::RxVFO::setFMIFNR -> sdrpp_vfo_set_fmnr) between the blocks of a RUNNING pipelined graph:
tests/host_cpp/test_fmif.cpp, its schedule replayed on the float64 restatement of tests/test_fmif.py over the stream of a twin channel without FMIF."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_fmif import Fmif, Tally, fm_signal
from test_host_cpp import _build

ROOT = S.ROOT


def _run_and_check(exe, tmp, wait_ms):
    sr, B, nblk = 2.4e6, 12000, 12
    x = fm_signal(sr, B * nblk, sr / 8 + 300.0, 24000.0, seed=3)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(sr), str(B), tmp, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % nblk in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)
    nr, ifs = ld("nr.f32", np.float32).view(np.complex64), ld("if.f32", np.float32).view(np.complex64)
    want_counts = ld("if_counts.i32", np.int32).tolist()  # (the resampler delivers 121 and 119 samples in turn)
    assert len(want_counts) == nblk and sum(want_counts) == B * nblk * 24000.0 / sr == len(ifs) and ld("nr_counts.i32", np.int32).tolist() == want_counts  # nothing lost, nothing twice
    # ---- the yardstick under the same schedule (a setter called after block k takes effect from block k + 1 on) ----
    y, t, on = Fmif(32), Tally(), False
    pos = filtered = 0
    for b, n in enumerate(want_counts):
        if b == 2:
            y.set_bins(15)
            on = True
        if b == 4:
            y.set_bins(31)  # setBins clears the delay line
        if b == 6:
            on = False      # unplugged: the delay line stays as block 5 left it
        if b == 8:
            on = True
        if b == 10:
            on = False
        g, i = nr[pos:pos + n], ifs[pos:pos + n]
        pos += n
        if on:
            t.check(g, y.process(i), "block %d" % b)
            filtered += int(np.sum(g != i))
        else:
            assert np.array_equal(g.view(np.uint32), i.view(np.uint32)), b
    t.done("host blocks")
    assert filtered >= 700, filtered
    return rr.stdout


def test_fmif_setter_while_running_on_the_emulator():
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_fmif.cpp"), tmp, 60000)


@pytest.mark.gpu
def test_fmif_setter_while_running_on_the_device():
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_fmif.cpp"), tmp, 20000)
