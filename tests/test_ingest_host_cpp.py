"""Raw wire formats through the C++ host blocks (sdrpp_gpu::IQFrontEnd::ingestRaw / ingestServerFrame): tests/host_cpp/test_ingest.cpp.  Twelve blocks of 5000
samples at 1 MS/s — int8, then uint8 through the rtl_sdr table from block 6 on — and two server frames; one WFM radio and a consumer bound with bindIQStream.
The consumer's floats are the numpy restatement of the bytes and the radio's audio is what the C-ABI gives for push(restatement) of the same blocks, bit for
bit on either backend, one hand-over per block: nothing lost or doubled."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_ingest import np_u8_table, restate
from test_rds import bits_equal, broadcast

ROOT = S.ROOT
SR, B, NBLK, SWITCH = 1e6, 5000, 12, 6
FRAMES = [(1, 0.37, 5000), (0, 1.0, 3001)]  # (PCMType, scaler, samples)


def _inputs():
    """-> raw bytes of the blocks, the frames, and per hand-over the floats the reference's conversions make of them"""
    from sdrplusplus_amd import capi

    x = broadcast(B * (NBLK + 2), seed=31, sr=SR).view(np.float32)
    q = np.clip(np.round(x / np.max(np.abs(x)) * 100.0), -128, 127).astype(np.int8)
    tab = np_u8_table(capi.U8_RTL_SDR)
    raw, want = [], []
    for k in range(NBLK):
        blk = q[2 * B * k:2 * B * (k + 1)]
        if k < SWITCH:
            raw.append(blk.view(np.uint8))
            want.append(restate(blk, capi.IQ_I8, 128.0))
        else:
            u = (blk.astype(np.int16) + 128).astype(np.uint8)
            raw.append(u)
            want.append(restate(u, capi.IQ_U8, table=tab))
    frames, pos = [], 2 * B * NBLK
    for typ, scaler, n in FRAMES:
        d = q[pos:pos + 2 * n]
        pos += 2 * n
        if typ == 1:
            d = d.astype(np.int16) * 200
            want.append(restate(d, capi.IQ_I16, np.float32(32768) / np.float32(scaler)))
        else:
            want.append(restate(d, capi.IQ_I8, np.float32(128) / np.float32(scaler)))
        frames.append(struct.pack("<HHf", 0, typ, scaler) + d.tobytes())
    frames.append(struct.pack("<HHf", 0, 9, 1.0) + b"\x01\x02\x03\x04")  # an unknown type: 0 samples, nothing handed out
    return np.concatenate(raw), frames, want


def _capi_audio(want, lib):
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        d, keep = radio.vfo_desc(SR, 250e3, 150e3, 200e3, "WFM")
        vid = ctx.vfo_add(d, keep)
        audio = []
        for w in want:
            ctx.push(w.view(np.complex64))
            audio.append(ctx.vfo_read(vid).copy())
        ctx.close()
        return audio
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, lib):
    raw, frames, want = _inputs()
    raw.tofile(os.path.join(tmp, "raw.bin"))
    with open(os.path.join(tmp, "frames.bin"), "wb") as f:
        for fr in frames:
            f.write(struct.pack("<i", len(fr)) + fr)
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "raw.bin"), os.path.join(tmp, "frames.bin"), str(SR), str(B), str(SWITCH), tmp],
                        capture_output=True, text=True, timeout=900)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d frames %d frame samples %d" % (NBLK, len(frames), sum(n for _, _, n in FRAMES)) in rr.stdout, rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    assert ld("iq_counts.i32", np.int32).tolist() == [len(w) // 2 for w in want]  # one hand-over per block and frame that held samples
    assert bits_equal(ld("iq.f32", np.float32), np.concatenate(want))
    audio = _capi_audio(want, lib)
    assert ld("audio_counts.i32", np.int32).tolist() == [len(a) for a in audio]
    assert bits_equal(ld("audio.f32", np.float32).reshape(-1, 2), np.concatenate(audio))


def test_ingest_graph_on_the_emulator():
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_ingest.cpp"), tmp, "emu")


@pytest.mark.gpu
def test_ingest_graph_on_the_device():
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_ingest.cpp"), tmp, "gpu")
