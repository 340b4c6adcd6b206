"""Records tests/golden/stereo_ref.npz, stereo_ref_cuts.npz and stereo_ref_toggle.npz (no file larger than the largest fixture there is): the reference's dsp::demod::BroadcastFM (dsp/demod/broadcast_fm.h, compiled unmodified against oracle/shim) with its
stereo decoder on, run over a handful of IF-rate inputs.  Only the recorded DATA is committed; the harness below is this project's own and is compiled into a
temporary directory.

    python tests/golden/make_stereo_golden.py /path/to/SDRPlusPlus

(broadcast_fm.h does not itself include channel/frequency_xlator.h: the harness includes that first.)

Inputs are IF-rate I/Q (250 kS/s) stored as int16, value / 16384 (exactly representable): an FM carrier (amplitude 0.06) of 75 kHz deviation carrying
L = 1 kHz and R = 2.3 kHz at different levels as L+R, L-R on 38 kHz and the 19 kHz pilot at 9 % of the deviation, and noise between 0.0005 and 0.02.  Per case:
    <name>_x       int16 [n, 2]
    <name>_cut     the block schedule: samples per process() call
    <name>_ops     per block the operation in front of it: 0 none, 1 setStereo(false), 2 setStereo(true), 3 reset()
    <name>_stereo  per block: the stereo decoder on (1) or off (0) when it ran
    <name>_audio   the (l, r) frames of all blocks, float32 [n, 2] (not for `nopilot`, which is compared with the device's own mono audio)
    <name>_lp      the audio low-pass on (1) or off (0)
and once, in stereo_ref.npz: pilot_taps (float32 [317, 2]), alpha, beta (float32), delay.
The generator asserts on the reference's own output: rms(l - r) > 0.1 rms in the pilot cases, and for `nopilot` that (l + r) / 2 is the mono audio delayed
by 159 samples within 1e-5 of its RMS, every value finite."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dsp/channel/frequency_xlator.h"
#include "dsp/demod/broadcast_fm.h"
struct Probe : dsp::demod::BroadcastFM {
    void dump(const char* path) {
        FILE* f = fopen(path, "wb");
        const int n = pilotFirTaps.size;
        fwrite(&n, sizeof(int), 1, f);
        fwrite(pilotFirTaps.taps, sizeof(dsp::complex_t), (size_t)n, f);
        float ab[2];
        dsp::loop::PhaseControlLoop<float>::criticallyDamped(25000.0 / _samplerate, ab[0], ab[1]);
        fwrite(ab, sizeof(float), 2, f);
        fclose(f);
    }
};
// argv: in.bin audio.bin consts.bin stereo lowpass op...      op: c<count> | n (setStereo(true)) | f (setStereo(false)) | r (reset())
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n), rds((size_t)n + 64);
    std::vector<dsp::stereo_t> au((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    dsp::stream<dsp::complex_t> dummy;
    Probe fm;
    fm.init(&dummy, 75000.0, 250000.0, atoi(argv[4]) != 0, atoi(argv[5]) != 0, false);
    fm.dump(argv[3]);
    long pos = 0;
    for (int a = 6; a < argc; a++) {
        if (argv[a][0] == 'n') { fm.setStereo(true); }
        else if (argv[a][0] == 'f') { fm.setStereo(false); }
        else if (argv[a][0] == 'r') { fm.reset(); }
        else {
            const int v = atoi(argv[a] + 1);
            int got = 0;
            fm.process(v, x.data() + pos, au.data() + pos, got, rds.data());
            pos += v;
        }
    }
    if (pos != n) { return 3; }
    f = fopen(argv[2], "wb");
    fwrite(au.data(), sizeof(dsp::stereo_t), (size_t)n, f);
    fclose(f);
    return 0;
}
"""


def signal(n, seed, noise, pilot=True, rate=250000.0):
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    left, right = 0.5 * np.sin(2 * np.pi * 1000.0 * t), 0.3 * np.sin(2 * np.pi * 2300.0 * t + 0.4)
    msg = 0.45 * (left + right) + 0.45 * (left - right) * np.sin(2 * np.pi * 38000.0 * t)
    if pilot:
        msg = msg + 0.09 * np.sin(2 * np.pi * 19000.0 * t)
    x = 0.06 * np.exp(1j * 2 * np.pi * np.cumsum(75e3 * msg) / rate) + noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    q = np.empty((n, 2), np.int16)
    q[:, 0] = np.rint(x.real * 16384.0)
    q[:, 1] = np.rint(x.imag * 16384.0)
    return q


def schedule(n, sizes):
    out, pos, k = [], 0, 0
    while pos < n:
        s = min(sizes[k % len(sizes)], n - pos)
        out.append(s)
        pos += s
        k += 1
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


OPS = {"f": 1, "n": 2, "r": 3}
CASES = [
    # name, n, seed, noise, pilot, low-pass, block sizes (cycled), {block: op in front of it}
    ("steady", 12500, 1, 0.0005, True, True, [1250], {}),
    ("cuts", 12000, 2, 0.002, True, True, [997, 7, 1, 1250], {}),
    ("toggle", 12500, 3, 0.02, True, True, [1250], {3: "f", 5: "n", 8: "r"}),
    ("nolp", 4000, 4, 0.002, True, False, [1250], {}),
    ("nopilot", 12500, 1, 0.0005, False, True, [1250], {}),
]


# no fixture file larger than the largest there is: the cases are spread over three
FILES = {"steady": "stereo_ref.npz", "nolp": "stereo_ref.npz", "cuts": "stereo_ref_cuts.npz", "nopilot": "stereo_ref_cuts.npz", "toggle": "stereo_ref_toggle.npz"}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "h.cpp"), os.path.join(tmp, "h")
        with open(src, "w") as f:
            f.write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "core", "src"), "-o", exe, src, "-lpthread"], check=True)
        fin, fau, fco = (os.path.join(tmp, k) for k in ("in.bin", "audio.bin", "consts.bin"))

        def run(x, stereo, lowpass, toks):
            x.tofile(fin)
            subprocess.run([exe, fin, fau, fco, str(int(stereo)), str(int(lowpass))] + toks, check=True)
            return np.fromfile(fau, np.float32).reshape(-1, 2)

        for name, n, seed, noise, pilot, lowpass, sizes, ops in CASES:
            q = signal(n, seed, noise, pilot)
            cut = schedule(n, sizes)
            x = (q.astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
            toks, opl, on, state = [], [], [], 1
            for b, s in enumerate(cut):
                op = ops.get(b)
                if op:
                    toks.append(op)
                    state = {"f": 0, "n": 1, "r": state}[op]
                opl.append(OPS[op] if op else 0)
                toks.append("c%d" % s)
                on.append(state)
            audio = run(x, True, lowpass, toks)
            assert np.all(np.isfinite(audio)), name
            l, r = audio[:, 0], audio[:, 1]
            if pilot:
                st = np.repeat(np.asarray(on), cut).astype(bool)
                assert rms((l - r)[st]) > 0.1 * rms(audio[st]), (name, rms((l - r)[st]), rms(audio[st]))
            else:
                mono = run(x, False, lowpass, ["c%d" % s for s in cut])[:, 0]
                want = np.concatenate([np.zeros(159, np.float32), mono[:-159]])
                rel = rms((l + r) / 2 - want) / rms(want)
                print("nopilot: (l + r) / 2 against the mono audio delayed by 159: %.3g of its RMS" % rel)
                assert rel < 1e-5, rel
            o = out.setdefault(FILES[name], {})
            o[name + "_x"] = q
            o[name + "_cut"] = np.asarray(cut, np.int32)
            o[name + "_ops"] = np.asarray(opl, np.int8)
            o[name + "_stereo"] = np.asarray(on, np.int8)
            o[name + "_lp"] = np.int8(lowpass)
            if pilot:  # (nopilot is compared with the device's own mono audio: its frames are not needed)
                o[name + "_audio"] = audio
        co = open(fco, "rb").read()
        nt = int(np.frombuffer(co, np.int32, 1)[0])
        o = out["stereo_ref.npz"]
        o["pilot_taps"] = np.frombuffer(co, np.float32, 2 * nt, 4).reshape(-1, 2).copy()
        ab = np.frombuffer(co, np.float32, 2, 4 + 8 * nt)
        o["alpha"], o["beta"] = np.float32(ab[0]), np.float32(ab[1])
        o["delay"] = np.int32((nt - 1) // 2 + 1)
    for fn, o in out.items():
        path = os.path.join(ROOT, "tests", "golden", fn)
        np.savez_compressed(path, **o)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 233 * 1024, "fixture larger than the largest one there is (fmif_ref.npz)"


if __name__ == "__main__":
    main()
