"""The pager decoder's DSP through the C++ host blocks (sdrpp_gpu::POCSAGDSP in sdrplusplus_amd/host/sdrpp_gpu_pager.h over RxVFO::attachSymbols / setSymbolsOn /
symOut / symSoft): tests/host_cpp/test_pager.cpp.  `out` and `soft` must carry exactly the bits and soft values the C-ABI gives for the same blocks with the same
switch — one swap each per block that started a symbol, through stop / start and setPipelining off / on, nothing lost or doubled.  Bit for bit on either
backend: no tolerance."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import support as S
from test_host_cpp import _build
from test_pager import bits_equal, fsk

ROOT = S.ROOT
SR, B, NBLK, OFF_BLOCK = 240e3, 5000, 12, 8


def _capi_reference(x, lib):
    """the same blocks through the C-ABI, block by block: per channel the (soft, bits) per block, and the NFM radio's audio per block"""
    from sdrplusplus_amd import capi, radio

    old = capi.DEFAULT_LIB
    if lib == "emu":
        capi.DEFAULT_LIB = os.path.join(ROOT, "tests", "emu", "libsdrpp_gpu_emu.so")
    try:
        ctx = capi.Context(0, max_push=B)
        ctx.set_reference_block(0)
        vids, descs = [], []
        for baud in (2400.0, 1200.0):
            d, keep = radio.vfo_desc(SR, 24e3, 12.5e3, 30e3, "RAW")
            vids.append(ctx.vfo_add(d, keep))
            descs.append(radio.pager_desc(24e3, baud))
            ctx.vfo_set_symbols(vids[-1], descs[-1][0], True, descs[-1][1])
        d, keep = radio.vfo_desc(SR, 50e3, 12.5e3, -60e3, "NFM")
        nfm = ctx.vfo_add(d, keep)
        outs, audio = ([], []), []
        for k in range(NBLK):
            if k in (OFF_BLOCK, OFF_BLOCK + 1):
                ctx.vfo_set_symbols(vids[0], descs[0][0], k != OFF_BLOCK, descs[0][1])
            ctx.push(x[k * B:(k + 1) * B])
            for i in range(2):
                outs[i].append(ctx.vfo_sym_read(vids[i]))
            audio.append(ctx.vfo_read(nfm))
        ctx.close()
        return outs, audio
    finally:
        capi.DEFAULT_LIB = old


def _run_and_check(exe, tmp, mode, wait_ms, lib, env=None):
    x = (fsk(B * NBLK, seed=41, f0=30e3) + fsk(B * NBLK, seed=42, f0=-60e3, amp=0.2)).astype(np.complex64)
    x.view(np.float32).tofile(os.path.join(tmp, "iq.f32"))
    rr = subprocess.run([exe, os.path.join(ROOT, "sdrplusplus_amd", "data", "decim_plans.bin"), os.path.join(tmp, "iq.f32"), str(SR), str(B), tmp, mode, str(wait_ms)],
                        capture_output=True, text=True, timeout=900, env=env)
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert "blocks %d" % NBLK in rr.stdout
    ld = lambda name, dt: np.fromfile(os.path.join(tmp, name), dt)  # noqa: E731
    want, audio = _capi_reference(x, lib)
    assert len(want[0][OFF_BLOCK][0]) == 0 and all(len(w[0]) > 0 for k, w in enumerate(want[0]) if k != OFF_BLOCK) and all(len(w[0]) > 0 for w in want[1])
    for tag, w in (("a", want[0]), ("b", want[1])):
        counts = [len(p[0]) for p in w if len(p[0])]
        assert ld(tag + "_bits_counts.i32", np.int32).tolist() == counts, (tag, rr.stdout)  # one swap per producing block, on `out` ...
        assert ld(tag + "_soft_counts.i32", np.int32).tolist() == counts, (tag, rr.stdout)  # ... and on `soft` (swapped only when count > 0)
        assert bits_equal(ld(tag + "_soft.f32", np.float32), np.concatenate([p[0] for p in w])), tag
        assert bits_equal(ld(tag + "_bits.u8", np.uint8), np.concatenate([p[1] for p in w])), tag
    assert len(ld("audio_counts.i32", np.int32)) == NBLK, rr.stdout  # nothing lost on the radio beside them
    assert bits_equal(ld("audio.f32", np.float32).reshape(-1, 2), np.concatenate(audio).view(np.float32).reshape(-1, 2))
    return rr.stderr


@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_pager_graph_on_the_emulator(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, lib="emu", source="test_pager.cpp"), tmp, mode, 60000, "emu")


@pytest.mark.parametrize("san", ["address", "thread"])
def test_pager_graph_host_side_under_sanitizers(san):
    """The same stand-alone program with the HOST side (the adaptor, the C++ blocks, the test double of dsp::stream / dsp::block, the test) compiled with
    -fsanitize=address / thread and linked with the emulator library, pipelined: no memory error, no data race (the one filtered report is GCC's own, see
    tests/test_host_cpp.py), and the outputs are still the C-ABI's."""
    EMU = os.path.join(ROOT, "tests", "emu")
    S.locked_make("-C", EMU, "-s")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "test_pager_" + san)
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "host_cpp", "test_pager.cpp"),
                            "-I" + os.path.join(ROOT, "tests", "host_cpp", "standalone"), "-L" + EMU, "-l:libsdrpp_gpu_emu.so", "-Wl,-rpath," + EMU, "-lpthread"], capture_output=True, text=True)
        if r.returncode != 0 and ("cannot find" in r.stderr or "sanitizer" in r.stderr.lower()):
            pytest.skip("no %s sanitizer runtime in this toolchain" % san)
        assert r.returncode == 0, r.stderr[-2000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0 exitcode=0")
        err = _run_and_check(exe, tmp, "pipelined", 120000, "emu", env=env)
        assert "AddressSanitizer" not in err, err[-3000:]
        reports = [ln for ln in err.splitlines() if ln.startswith("WARNING: ThreadSanitizer")]
        assert all("double lock of a mutex" in ln for ln in reports), "\n".join(reports) + err[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["pipelined", "bypass"])
def test_pager_graph_on_the_device(mode):
    with tempfile.TemporaryDirectory() as tmp:
        _run_and_check(_build(tmp, source="test_pager.cpp"), tmp, mode, 20000, "gpu")
