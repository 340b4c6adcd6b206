"""Signal meters through the C++ host blocks (sdrpp_gpu::IQFrontEnd::setSignalMeters / RxVFO::getSignalInfo -> sdrpp_wf_set_meters, sdrpp_result_meters in
a pipelined graph, sdrpp_wf_meters_read block by block): tests/host_cpp/test_meters.cpp.  After each of its three phases every VFO must report the C-ABI's
own row of the newest line of that phase under the table the line's block was pushed with — also when the table was changed (retune, bandwidth, a VFO
removed and another added: the columns move) while those blocks were in flight.  The expectation is an ordinary-pass context of the same library
over the same samples: bit for bit, no tolerance (tests/test_meters.py holds that path against the oracle)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build

ROOT = S.ROOT
SR, B, N, RATE, NBLK = 2.4e6, 12000, 4096, 100.0, 18
A0, A1, B0, B1, C0, D0 = (600e3, 150e3), (650e3, 150e3), (-500e3, 100e3), (-500e3, 80e3), (100e3, 50e3), (-300e3, 120e3)
# (table, its VFOs) per phase of six blocks
PHASES = [([A0, B0, C0], "abc"), ([A1, B1, C0], "abc"), ([A1, C0, D0], "acd")]


def expected(x):
    """-> per phase {vfo name: (strength, snr) of the phase's newest line}"""
    from sdrplusplus_amd import capi

    nz, skip = capi.design_reshape_params(SR, N, RATE)
    ctx = capi.Context(0, max_push=B)
    ctx.fft_configure(N, nz, skip, capi.design_fft_window(2, nz))
    out = []
    for p, (bands, names) in enumerate(PHASES):
        ctx.wf_set_meters(bands, SR)
        last = None
        for k in range(6 * p, 6 * p + 6):
            ctx.push(x[k * B:(k + 1) * B])
            m = ctx.wf_meters()
            if len(m):
                last = m[-1]
        assert last is not None
        out.append({nm: last[i] for i, nm in enumerate(names)})
    ctx.close()
    return out


def _run_and_check(exe, tmp, mode, wait_ms):
    from sdrplusplus_amd import workloads

    x = workloads.synth(1, B * NBLK, seed=5)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(SR), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    got = np.fromfile(os.path.join(tmp, "signal.f32"), np.float32).reshape(3, 4, 3)
    want = expected(x)
    # phase 1 ends with b removed and d added while the phase's blocks were in flight: they were pushed under the table (a, b, c) — d has no line yet,
    # and c must hold ITS column of that table (2), not the column it has in the new one (1)
    live = ["abc", "ac", "acd"]
    for p in range(3):
        for i, nm in enumerate("abcd"):
            valid, pair = got[p, i, 0] == 1.0, got[p, i, 1:]
            assert valid == (nm in live[p]), (p, nm, got[p])
            if valid:
                assert np.array_equal(pair.view(np.uint32), want[p][nm].view(np.uint32)), (p, nm, pair, want[p])
    assert not np.array_equal(want[1]["b"], want[1]["c"])  # (the columns that would be confused differ)
    return rr.stdout


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_meters_graph(backend, mode):
    with tempfile.TemporaryDirectory() as tmp:
        emu = backend == "emu"
        _run_and_check(_build(tmp, lib="emu" if emu else "product", source="test_meters.cpp"), tmp, mode, 60000 if emu else 20000)
