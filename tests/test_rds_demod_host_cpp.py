"""The radio's RDS demodulator through the C++ host blocks (sdrpp_gpu::RDSDemod in sdrplusplus_amd/host/sdrpp_gpu_rds.h over RxVFO::attachRDSDemod /
setRDSDemodSoft / resetRDSDemod / rdsBits / rdsSoft): tests/host_cpp/test_rds_demod.cpp.  `out` and `soft` must carry exactly the bits and soft values the C-ABI
gives for the same blocks with the same calls — one swap per block that started a symbol, `soft` only while it is enabled, through stop / start, setPipelining
off / on, reset() and a bind in mid-stream; a bound adaptor stops the channel's rdsOut (radio A's has no reader at all: the graph would block) while radio B's
rdsOut carries exactly its samples up to the bind.  Bit for bit on either backend: no tolerance."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_rds import broadcast
from test_rds_demod import bits_equal

ROOT = S.ROOT
SR, B, NBLK = 1e6, 20000, 13
SOFT_OFF, RESET_AT, BIND_B, REBIND_B = 7, 9, 10, 11  # the block in FRONT of which the call takes effect (the program issues it behind the block before)


def _capi_reference(x, lib):
    """the same blocks through the C-ABI, block by block -> per radio the (soft, bits) per block, B's RDS samples per block, A's audio per block"""
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        vids = []
        for off in (200e3, -250e3):
            d, keep = radio.vfo_desc(SR, 250e3, 150e3, off, "WFM")
            vids.append(ctx.vfo_add(d, keep))
            rd, rkeep = radio.rds_desc(250e3)
            ctx.vfo_set_rds(vids[-1], rd, True, rkeep)
        dd, dk = radio.rds_demod_desc(5000.0, 0)
        ctx.vfo_set_rds_demod(vids[0], dd, True, dk)
        outs, rds_b, audio = ([], []), [], []
        for k in range(NBLK):
            if k == RESET_AT:
                ctx.vfo_rds_demod_reset(vids[0])
            if k in (BIND_B, REBIND_B):
                ctx.vfo_set_rds_demod(vids[1], None)
                ctx.vfo_set_rds_demod(vids[1], dd, True, dk)
            ctx.push(x[k * B:(k + 1) * B])
            outs[0].append(ctx.vfo_rds_demod_read(vids[0]))
            outs[1].append(ctx.vfo_rds_demod_read(vids[1]) if k >= BIND_B else (np.zeros(0, np.float32), np.zeros(0, np.uint8)))
            rds_b.append(ctx.vfo_rds_read(vids[1]))
            audio.append(ctx.vfo_read(vids[0]))
        ctx.close()
        return outs, rds_b, audio
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, mode, wait_ms, lib, env=None):
    x = (broadcast(B * NBLK, seed=31, sr=SR) * np.exp(2j * np.pi * 200e3 * np.arange(B * NBLK) / SR)).astype(np.complex64)
    x = (x + broadcast(B * NBLK, seed=32, sr=SR) * np.exp(-2j * np.pi * 250e3 * np.arange(B * NBLK) / SR)).astype(np.complex64)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(SR), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900, env=env)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % NBLK in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    want, rds_b, audio = _capi_reference(x, lib)
    assert all(len(w[0]) > 10 for w in want[0]) and all(len(w[0]) > 10 for w in want[1][BIND_B:])
    # A: bits for every block; soft for every block but the one its output was disabled for
    assert ld("a_bits_counts.i32", np.int32).tolist() == [len(p[0]) for p in want[0]], rr.stdout
    assert bits_equal(ld("a_bits.u8", np.uint8), np.concatenate([p[1] for p in want[0]]))
    soft_a = [p[0] for k, p in enumerate(want[0]) if k != SOFT_OFF]
    assert ld("a_soft_counts.i32", np.int32).tolist() == [len(p) for p in soft_a], rr.stdout
    assert bits_equal(ld("a_soft.f32", np.float32), np.concatenate(soft_a))
    # B: rdsOut up to the bind and not a sample after it; bits from the bind on; soft from the second init() on
    # (pipelined blocks are delivered up to `lag` = 4 blocks late: those still in flight at the bind are not written to rdsOut either — nobody reads it any more)
    got_rds = ld("b_rds_counts.i32", np.int32).tolist()
    assert BIND_B - 4 <= len(got_rds) <= BIND_B and got_rds == [len(r) for r in rds_b[:len(got_rds)]], rr.stdout
    assert mode == "pipelined" or len(got_rds) == BIND_B
    assert bits_equal(ld("b_rds.f32", np.float32).view(np.complex64), np.concatenate(rds_b[:len(got_rds)]))
    assert ld("b_bits_counts.i32", np.int32).tolist() == [len(p[0]) for p in want[1][BIND_B:]], rr.stdout
    assert bits_equal(ld("b_bits.u8", np.uint8), np.concatenate([p[1] for p in want[1][BIND_B:]]))
    assert ld("b_soft_counts.i32", np.int32).tolist() == [len(p[0]) for p in want[1][REBIND_B:]], rr.stdout
    assert bits_equal(ld("b_soft.f32", np.float32), np.concatenate([p[0] for p in want[1][REBIND_B:]]))
    # nothing lost on the radios beside them, and A's audio is the C-ABI's
    for tag in ("a", "b", "p"):
        assert len(ld(tag + "_audio_counts.i32", np.int32)) == NBLK, (tag, rr.stdout)
    assert bits_equal(ld("a_audio.f32", np.float32).reshape(-1, 2), np.concatenate(audio))
    return rr.stderr


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_rds_demod_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_rds_demod.cpp"), tmp, mode, 60000, "emu")


def test_rds_demod_graph_host_side_under_sanitizers():
    """The same stand-alone program with the HOST side (the adaptor, the C++ blocks, the test double of dsp::stream / dsp::block, the test) compiled with
    -fsanitize=address,undefined and linked with the emulator library, pipelined: no report, and the outputs are still the C-ABI's.  No preloaded runtime and no
    GPU are involved."""
    EMU = os.path.join(ROOT, "tests", "emu")
    S.locked_make("-C", EMU, "-s")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_rds_demod_asan")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "host_cpp", "test_rds_demod.cpp"),
                            "-I" + os.path.join(ROOT, "tests", "host_cpp", "standalone"), "-L" + EMU, "-l:libsdrpp_gpu_emu.so", "-Wl,-rpath," + EMU, "-lpthread"], capture_output=True, text=True)
        if r.returncode != 0 and ("cannot find" in r.stderr or "sanitizer" in r.stderr.lower()):
            pytest.skip("no address / undefined sanitizer runtime in this toolchain")
        assert r.returncode == 0, r.stderr[-2000:]
        err = _run_and_check(exe, tmp, "pipelined", 120000, "emu", env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_rds_demod_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_rds_demod.cpp"), tmp, mode, 20000, "gpu")
