"""The radio's CW mode through the C++ host blocks (sdrpp_gpu::FusedDemodulator<.., CW>, RxVFO::setCWTone): tests/host_cpp/test_cw.cpp runs the radio
module's mode switch WFM -> CW -> USB on one channel of a running front end, with setTone, the bandwidth taken to CW's minimum of 50 Hz (4 560 channel taps)
and pipelining switched off / on in between.  `audio` must carry exactly the samples the C-ABI gives for the same blocks with the same calls — one swap per
producing block, nothing lost or doubled.  Bit for bit on either backend: no tolerance."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_cw import keyed
from test_host_cpp import _build
from test_rds import bits_equal

ROOT = S.ROOT
SR, B, NBLK, OFF = 1e6, 5000, 14, 200e3


def _capi_reference(x, lib):
    """the same blocks through the C-ABI, block by block, with the calls the host blocks make: -> the channel's audio per block"""
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        d, keep = radio.vfo_desc(SR, 250e3, 150e3, OFF, "WFM")
        vid = ctx.vfo_add(d, keep)
        audio = []
        for k in range(NBLK):
            ctx.push(x[k * B:(k + 1) * B])
            audio.append(ctx.vfo_read(vid).copy())
            if k == 2:  # the new demodulator behind the same RxVFO (keep = 1), then RxVFO::setOutSamplerate (keep = 1: the demodulator starts cleared)
                d, keep = radio.vfo_desc(SR, 250e3, 150e3, OFF, "CW")
                vid = ctx.vfo_replace(vid, d, 1, keep)
                d, keep = radio.vfo_desc(SR, 3000.0, 200.0, OFF, "CW")
                vid = ctx.vfo_replace(vid, d, 1, keep)
            if k == 4:
                for tone in (250.0, 1250.0, 600.0):  # setTone(100), setTone(5000), setTone(600) behind the menu's clamp
                    ctx.vfo_set_ssb_phase_delta(vid, *capi.design_phase_delta(tone, 3000.0))
            if k == 6:
                taps = capi.design_low_pass(25.0, 2.5, 3000.0)
                assert len(taps) == 4560
                ctx.vfo_set_channel_taps(vid, taps)
            if k == 10:  # USB behind the RxVFO as it stands (3 kS/s, channel 50 Hz; the demodulator's own bandwidth is USB's 2 800 Hz), then the new rate
                d, keep = radio.vfo_desc(SR, 3000.0, 50.0, OFF, "USB")
                d.ssb_phase_delta_re, d.ssb_phase_delta_im = capi.design_phase_delta(1400.0, 3000.0)
                vid = ctx.vfo_replace(vid, d, 1, keep)
                d, keep = radio.vfo_desc(SR, 24000.0, 2800.0, OFF, "USB")
                vid = ctx.vfo_replace(vid, d, 1, keep)
        ctx.close()
        return audio
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, mode, wait_ms, lib):
    x = keyed(SR, B * NBLK, OFF, 37, dot=0.004).astype(np.complex64)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(SR), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % NBLK in rr.stdout
    got = np.fromfile(os.path.join(tmp, "audio.f32"), np.float32).reshape(-1, 2)
    cnt = np.fromfile(os.path.join(tmp, "counts.i32"), np.int32)
    want = _capi_reference(x, lib)
    lens = [len(w) for w in want]
    assert lens[:3] == [1250] * 3 and set(lens[3:11]) <= {15, 16} and set(lens[11:]) <= {120, 121}, lens  # WFM at 250 kS/s, CW at 3 kS/s, USB at 24 kS/s
    assert cnt.tolist() == [len(w) for w in want], (cnt.tolist(), rr.stdout)  # one swap per producing block
    assert bits_equal(got, np.concatenate(want))
    return rr.stdout


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_cw_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_cw.cpp"), tmp, mode, 60000, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_cw_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_cw.cpp"), tmp, mode, 20000, "gpu")
