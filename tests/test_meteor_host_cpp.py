"""The Meteor QPSK demodulator through the C++ host blocks (sdrpp_gpu::Meteor in sdrplusplus_amd/host/sdrpp_gpu_meteor.h over RxVFO::attachQPSK / setQPSKMode /
resetQPSK / qpskOut / qpskPacked): tests/host_cpp/test_meteor.cpp.  `out` and the packed stream must carry exactly the soft symbols and int8 pairs the C-ABI
gives for the same blocks with the same calls — one swap per block that started a symbol, through stop / start, setPipelining off / on, setOQPSK, reset() and a
bind in mid-stream; a bound adaptor stops the channel's own `out` (channel A's has no reader at all: the graph would block) while channel B's `out` carries
exactly its samples up to the bind.  Bit for bit on either backend: no tolerance."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_meteor import bits_equal

ROOT = S.ROOT
SR, B, NBLK = 600e3, 8000, 13
OQPSK_AT, RESET_AT, BIND_B, REBIND_B = 8, 9, 10, 11  # the block in FRONT of which the call takes effect (the program issues it behind the block before)


def _capi_reference(x, lib):
    """the same blocks through the C-ABI, block by block -> per channel the (soft, packed) per block, B's IF samples per block"""
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        vids = []
        for off in (150e3, -150e3):
            d, keep = radio.vfo_desc(SR, 150e3, 150e3, off, "RAW")
            vids.append(ctx.vfo_add(d, keep))
        md, mk = radio.meteor_desc()
        mo, mok = radio.meteor_desc(oqpsk=True)
        ctx.vfo_set_qpsk(vids[0], md, True, mk)
        none = (np.zeros(0, np.complex64), np.zeros((0, 2), np.int8))
        outs, if_b = ([], []), []
        for k in range(NBLK):
            if k == OQPSK_AT:
                ctx.vfo_qpsk_set_mode(vids[0], False, True)
            if k == RESET_AT:
                ctx.vfo_qpsk_reset(vids[0])
            if k == BIND_B:
                ctx.vfo_set_qpsk(vids[1], md, True, mk)
            if k == REBIND_B:
                ctx.vfo_set_qpsk(vids[1], None)
                ctx.vfo_set_qpsk(vids[1], mo, True, mok)
            ctx.push(x[k * B:(k + 1) * B])
            outs[0].append(ctx.vfo_qpsk_read(vids[0]))
            outs[1].append(ctx.vfo_qpsk_read(vids[1]) if k >= BIND_B else none)
            if_b.append(ctx.vfo_read(vids[1]))
        ctx.close()
        return outs, if_b
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, mode, wait_ms, lib, env=None):
    r = np.random.default_rng(61)
    x = (0.1 * (r.standard_normal(B * NBLK) + 1j * r.standard_normal(B * NBLK))).astype(np.complex64)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(SR), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900, env=env)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % NBLK in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    want, if_b = _capi_reference(x, lib)
    assert all(len(w[0]) > 900 for w in want[0]) and all(len(w[0]) > 900 for w in want[1][BIND_B:])
    # A: soft symbols and int8 pairs for every block, a swap each (the packed stream's swaps carry 2 x the symbols)
    assert ld("a_soft_counts.i32", np.int32).tolist() == [len(p[0]) for p in want[0]], rr.stdout
    assert ld("a_packed_counts.i32", np.int32).tolist() == [2 * len(p[0]) for p in want[0]], rr.stdout
    assert bits_equal(ld("a_soft.f32", np.float32).view(np.complex64), np.concatenate([p[0] for p in want[0]]))
    assert bits_equal(ld("a_packed.i8", np.int8).reshape(-1, 2), np.concatenate([p[1] for p in want[0]]))
    # B: `out` up to the bind and not a sample after it; symbols from the bind on
    # (pipelined blocks are delivered up to `lag` = 4 blocks late: those still in flight at the bind are not written to `out` either — nobody reads it any more)
    got_out = ld("b_out_counts.i32", np.int32).tolist()
    assert BIND_B - 4 <= len(got_out) <= BIND_B and got_out == [len(q) for q in if_b[:len(got_out)]], rr.stdout
    assert mode == "pipelined" or len(got_out) == BIND_B
    assert bits_equal(ld("b_out.f32", np.float32).reshape(-1, 2), np.concatenate(if_b[:len(got_out)]).view(np.float32).reshape(-1, 2))
    assert ld("b_soft_counts.i32", np.int32).tolist() == [len(p[0]) for p in want[1][BIND_B:]], rr.stdout
    assert ld("b_packed_counts.i32", np.int32).tolist() == [2 * len(p[0]) for p in want[1][BIND_B:]], rr.stdout
    assert bits_equal(ld("b_soft.f32", np.float32).view(np.complex64), np.concatenate([p[0] for p in want[1][BIND_B:]]))
    assert bits_equal(ld("b_packed.i8", np.int8).reshape(-1, 2), np.concatenate([p[1] for p in want[1][BIND_B:]]))
    # nothing lost on the radio beside them
    assert len(ld("p_audio_counts.i32", np.int32)) == NBLK, rr.stdout
    return rr.stderr


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_meteor_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_meteor.cpp"), tmp, mode, 60000, "emu")


def test_meteor_graph_host_side_under_sanitizers():
    """The same stand-alone program with the HOST side (the adaptor, the C++ blocks, the test double of dsp::stream / dsp::block, the test) compiled with
    -fsanitize=address,undefined and linked with the emulator library, pipelined: no report, and the outputs are still the C-ABI's.  No preloaded runtime and no
    GPU are involved."""
    EMU = os.path.join(ROOT, "tests", "emu")
    S.locked_make("-C", EMU, "-s")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_meteor_asan")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "host_cpp", "test_meteor.cpp"),
                            "-I" + os.path.join(ROOT, "tests", "host_cpp", "standalone"), "-L" + EMU, "-l:libsdrpp_gpu_emu.so", "-Wl,-rpath," + EMU, "-lpthread"], capture_output=True, text=True)
        if r.returncode != 0 and ("cannot find" in r.stderr or "sanitizer" in r.stderr.lower()):
            pytest.skip("no address / undefined sanitizer runtime in this toolchain")
        assert r.returncode == 0, r.stderr[-2000:]
        err = _run_and_check(exe, tmp, "pipelined", 120000, "emu", env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_meteor_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_meteor.cpp"), tmp, mode, 20000, "gpu")
