"""Records tests/golden/rds_ref.npz: the reference's dsp::demod::BroadcastFM (dsp/demod/broadcast_fm.h, compiled unmodified against oracle/shim) in its
mono branch with the audio low-pass on and `rdsOut` on, run over a handful of IF-rate inputs.  Only the recorded DATA is committed; the harness below is
this project's own and is compiled into a temporary directory.

    python tests/golden/make_rds_golden.py /path/to/SDRPlusPlus

(broadcast_fm.h does not itself include channel/frequency_xlator.h: the harness includes that first.)

Inputs are IF-rate I/Q (250 kS/s) stored as int16, value / 16384 (exactly representable): an FM carrier of 75 kHz deviation carrying 1 kHz audio, a 19 kHz
pilot, a BPSK-modulated 57 kHz subcarrier of about 3 kHz deviation, and noise.  Per case:
    <name>_x       int16 [n, 2]
    <name>_cut     the block schedule: samples per process() call
    <name>_on      per block: rdsOut on (1) or off (0) when it ran — setRDSOut is called in front of the first block of every change
    <name>_reset   the blocks in front of which the discriminator and the audio filter were cleared: reset(), and every setRDSOut (it calls reset())
    <name>_rds     the `rdsout` samples of all blocks, float32 [m, 2], and <name>_counts, the samples per block (0 while rdsOut is off)
    <name>_audio   toggle_reset only: the left channel (mono branch: left == right) of the three blocks around each setRDSOut — blocks 2 .. 5, where the
                   reference clears the discriminator and the audio filter (the click this project's layer does not make)
"""
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
// argv: in.bin rds.bin counts.bin audio.bin op...      op: c<count> | n (setRDSOut(true)) | f (setRDSOut(false)) | r (reset())
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
    dsp::demod::BroadcastFM fm;
    fm.init(&dummy, 75000.0, 250000.0, false, true, true);
    std::vector<int> counts;
    long pos = 0, nr = 0;
    bool on = true;
    for (int a = 5; a < argc; a++) {
        if (argv[a][0] == 'n') { fm.setRDSOut(true); on = true; }
        else if (argv[a][0] == 'f') { fm.setRDSOut(false); on = false; }
        else if (argv[a][0] == 'r') { fm.reset(); }
        else {
            const int v = atoi(argv[a] + 1);
            int got = 0;
            fm.process(v, x.data() + pos, au.data() + pos, got, rds.data() + nr);
            if (!on) { got = 0; }
            counts.push_back(got);
            nr += got;
            pos += v;
        }
    }
    if (pos != n) { return 3; }
    f = fopen(argv[2], "wb");
    fwrite(rds.data(), sizeof(dsp::complex_t), (size_t)nr, f);
    fclose(f);
    f = fopen(argv[3], "wb");
    fwrite(counts.data(), sizeof(int), counts.size(), f);
    fclose(f);
    f = fopen(argv[4], "wb");
    for (long i = 0; i < n; i++) {
        if (au[(size_t)i].l != au[(size_t)i].r) { return 4; }
        fwrite(&au[(size_t)i].l, sizeof(float), 1, f);
    }
    fclose(f);
    return 0;
}
"""


def signal(n, seed, rate=250000.0):
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    bits = np.cumsum(r.integers(0, 2, int(n / rate * 1187.5) + 2)) & 1
    ts = t * 1187.5
    bb = np.where(bits[ts.astype(np.int64)] == 1, 1.0, -1.0) * np.where((ts - np.floor(ts)) < 0.5, 1.0, -1.0)
    msg = 0.45 * np.sin(2 * np.pi * 1000.0 * t) + 0.09 * np.sin(2 * np.pi * 19000.0 * t) + 0.04 * bb * np.cos(2 * np.pi * 57000.0 * t)
    x = 0.06 * np.exp(1j * 2 * np.pi * np.cumsum(75e3 * msg) / rate) + 0.0005 * (r.standard_normal(n) + 1j * r.standard_normal(n))
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


CASES = [
    # name, n, seed, block sizes (cycled), {block: op in front of it}
    ("steady", 20000, 1, [1250], {}),
    ("cuts", 10000, 2, [997, 7, 1, 1250], {}),
    ("toggle_reset", 15000, 3, [1250], {3: "f", 5: "n", 8: "r"}),
]


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
        names = []
        for name, n, seed, sizes, ops in CASES:
            q = signal(n, seed)
            cut = schedule(n, sizes)
            x = (q.astype(np.float32) / np.float32(16384.0)).view(np.complex64).reshape(-1)
            fin, frds, fcnt, fau = (os.path.join(tmp, k) for k in ("in.bin", "rds.bin", "counts.bin", "audio.bin"))
            x.tofile(fin)
            toks, on, resets, state = [], [], [], 1
            for b, s in enumerate(cut):
                if b in ops:
                    toks.append(ops[b])
                    resets.append(b)
                    state = {"f": 0, "n": 1, "r": state}[ops[b]]
                toks.append("c%d" % s)
                on.append(state)
            subprocess.run([exe, fin, frds, fcnt, fau] + toks, check=True)
            audio = np.fromfile(fau, np.float32)
            out[name + "_x"] = q
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_on"] = np.asarray(on, np.int8)
            out[name + "_reset"] = np.asarray(resets, np.int32)
            out[name + "_rds"] = np.fromfile(frds, np.float32).reshape(-1, 2)
            out[name + "_counts"] = np.fromfile(fcnt, np.int32)
            if name == "toggle_reset":
                out[name + "_audio"] = audio[2 * 1250:6 * 1250]
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "rds_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
