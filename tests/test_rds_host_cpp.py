"""The WFM demodulator's RDS branch through the C++ host blocks (sdrpp_gpu::RxVFO::attachRDS / setRDSOut / rdsOut, FusedDemodulator<.., WFM>::setRDSOut /
getRDSOutput): tests/host_cpp/test_rds.cpp.  `rdsOut` must carry exactly the samples the C-ABI gives for the same blocks with the same switch — one swap per
block that produced samples, through stop / start and setPipelining off / on, nothing lost or doubled.  Bit for bit on either backend: no tolerance."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_rds import bits_equal, broadcast

ROOT = S.ROOT
SR, B, NBLK, OFF_BLOCK = 1e6, 5000, 12, 8


def _capi_reference(x, lib):
    """the same blocks through the C-ABI, block by block: (samples per block, the WFM radio's audio per block)"""
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        d, keep = radio.vfo_desc(SR, 250e3, 150e3, 200e3, "WFM")
        vid = ctx.vfo_add(d, keep)
        rd, rkeep = radio.rds_desc(250e3)
        ctx.vfo_set_rds(vid, rd, True, rkeep)
        outs, audio = [], []
        for k in range(NBLK):
            if k == OFF_BLOCK:
                ctx.vfo_set_rds(vid, rd, False, rkeep)
            if k == OFF_BLOCK + 1:
                ctx.vfo_set_rds(vid, rd, True, rkeep)
            ctx.push(x[k * B:(k + 1) * B])
            outs.append(ctx.vfo_rds_read(vid))
            audio.append(ctx.vfo_read(vid))
        ctx.close()
        return outs, audio
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, mode, wait_ms, lib):
    x = broadcast(B * NBLK, seed=31, sr=SR)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(SR), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % NBLK in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    got, gcnt = ld("rds.f32", np.float32).view(np.complex64), ld("rds_counts.i32", np.int32)
    assert len(ld("wfm_counts.i32", np.int32)) == NBLK and len(ld("plain_counts.i32", np.int32)) == NBLK, rr.stdout  # nothing lost on either radio
    want, audio = _capi_reference(x, lib)
    assert len(want[OFF_BLOCK]) == 0 and all(len(w) > 0 for k, w in enumerate(want) if k != OFF_BLOCK)
    assert gcnt.tolist() == [len(w) for w in want if len(w)], (gcnt.tolist(), [len(w) for w in want])  # one swap per producing block
    assert bits_equal(got, np.concatenate(want))
    assert bits_equal(ld("wfm_audio.f32", np.float32).reshape(-1, 2), np.concatenate(audio))  # (and the audio is the C-ABI's, switch or no switch)
    return rr.stdout


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_rds_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_rds.cpp"), tmp, mode, 60000, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_rds_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_rds.cpp"), tmp, mode, 20000, "gpu")
