"""The recorder sink through the C++ host blocks (sdrpp_gpu::RxVFO::attachRecorder / getRecorderLevel -> sdrpp_vfo_set_rec, result flag 16 in a pipelined
graph, sdrpp_vfo_rec_read block by block): tests/host_cpp/test_recorder.cpp.  `recorded` must carry exactly the bytes the float32 restatement of
tests/test_recorder.py gives for the blocks `audio` carried — one swap per block that is not silent — and the level getter the running maximum of their peaks.
Bit for bit on either backend: no tolerance."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_recorder import I16, f32, restate, signal

ROOT = S.ROOT


def _run_and_check(exe, tmp, mode, wait_ms):
    sr, B, nblk = 2.4e6, 12000, 12
    x = signal(B * nblk, 21)
    x[3 * B:6 * B] = 0  # three blocks of exact zeros: the filters run empty during the first, the next ones are silent
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(sr), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % nblk in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    audio, acnt = ld("rec_audio.f32", np.float32).reshape(-1, 2), ld("rec_audio_counts.i32", np.int32)
    got, gcnt = ld("rec_bytes.u8", np.uint8), ld("rec_bytes_counts.i32", np.int32)
    assert len(acnt) == nblk and len(ld("plain_counts.i32", np.int32)) == nblk, (acnt, rr.stdout)  # nothing lost on either radio
    assert int(np.sum(acnt)) == len(audio)
    want, wcnt, silent, pos = [], [], 0, 0
    level = np.zeros(2, f32)
    for n in acnt:
        samples, info = restate(audio[pos:pos + n], 0.9, True, I16, True)
        pos += n
        level = np.maximum(level, np.asarray([info["peak_l"], info["peak_r"]], f32))
        if info["silent"]:
            silent += 1
            continue
        want.append(samples.reshape(-1).view(np.uint8))
        wcnt.append(samples.size * 2)
    assert 1 <= silent <= 3, silent  # the stretch of zeros really produced silent blocks, and only it
    assert gcnt.tolist() == wcnt, (gcnt.tolist(), wcnt)  # one swap per block that is not silent
    assert np.array_equal(got, np.concatenate(want))
    lvl = ld("level.f32", np.float32)
    assert np.array_equal(lvl.view(np.uint32), level.view(np.uint32)), (lvl, level)
    assert level[0] > 0.1
    return rr.stdout


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_recorder_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_recorder.cpp"), tmp, mode, 60000)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_recorder_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_recorder.cpp"), tmp, mode, 20000)
