"""Records tests/golden/cw_ref.npz: the reference's dsp::demod::CW<stereo_t> (dsp/demod/cw.h, compiled unmodified against oracle/shim) as the radio module
sets it up (demodulators/cw.h:37, 105-107: tone 800 Hz, attack 100 / 3000, decay 5 / 3000, 3 kS/s), run over a handful of IF-rate inputs.  Only the recorded
DATA is committed; the harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_cw_golden.py /path/to/SDRPlusPlus

Inputs are IF-rate I/Q (3 kS/s) stored as int16, value / 16384 (exactly representable): a keyed carrier 20 Hz above the channel's centre (dots of 60 ms,
a few dashes), plus noise.  Per case:
    <name>_x       int16 [n, 2]
    <name>_cut     the block schedule: samples per process() call
    <name>_ops     [k, 3] float64: (block in front of which the setter ran, setter, value) — setter 0 setTone(value Hz), 1 setAGCAttack(value / 3000),
                   2 setAGCDecay(value / 3000); the value is the menu's, as demodulators/cw.h:49, 57, 66 pass it on
    <name>_audio   the left channel of every block (MonoToStereo: left == right, checked by the harness), float32 [n]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
IF_RATE, TONE, ATTACK, DECAY = 3000.0, 800.0, 100.0, 5.0

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dsp/demod/cw.h"
// argv: in.bin audio.bin op...      op: c<count> | t<tone Hz> | a<attack, menu value> | d<decay, menu value>
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n);
    std::vector<dsp::stereo_t> au((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    dsp::stream<dsp::complex_t> dummy;
    dsp::demod::CW<dsp::stereo_t> cw;
    cw.init(&dummy, 800.0, 100.0 / 3000.0, 5.0 / 3000.0, 3000.0);
    long pos = 0;
    for (int a = 3; a < argc; a++) {
        const double v = atof(argv[a] + 1);
        if (argv[a][0] == 't') { cw.setTone(v); }
        else if (argv[a][0] == 'a') { cw.setAGCAttack(v / 3000.0); }
        else if (argv[a][0] == 'd') { cw.setAGCDecay(v / 3000.0); }
        else {
            const int c = atoi(argv[a] + 1);
            if (cw.process(c, x.data() + pos, au.data() + pos) != c) { return 5; }
            pos += c;
        }
    }
    if (pos != n) { return 3; }
    f = fopen(argv[2], "wb");
    for (long i = 0; i < n; i++) {
        if (memcmp(&au[(size_t)i].l, &au[(size_t)i].r, sizeof(float)) != 0) { return 4; }
        fwrite(&au[(size_t)i].l, sizeof(float), 1, f);
    }
    fclose(f);
    return 0;
}
"""


def signal(n, seed, rate=IF_RATE):
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    unit = int(0.06 * rate)  # one dot
    key = np.zeros(n)
    pos = unit // 2
    while pos < n:
        mark = unit * (3 if r.integers(0, 4) == 0 else 1)
        key[pos:pos + mark] = 1.0
        pos += mark + unit * int(r.integers(1, 4))
    x = 0.3 * key * np.exp(2j * np.pi * 20.0 * t) + 0.002 * (r.standard_normal(n) + 1j * r.standard_normal(n))
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
    # name, n, seed, block sizes (cycled), [(block, setter, value)]
    ("steady", 3000, 1, [15], []),
    ("cuts", 4000, 2, [15, 1, 997, 7, 1, 1, 300], []),
    ("tone", 3000, 3, [15], [(100, "t", 600.0)]),
    ("agc", 3600, 4, [15], [(60, "a", 20.0), (130, "d", 15.0), (180, "a", 200.0)]),
]
SETTERS = {"t": 0, "a": 1, "d": 2}


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
            fin, fau = os.path.join(tmp, "in.bin"), os.path.join(tmp, "audio.bin")
            x.tofile(fin)
            toks = []
            for b, s in enumerate(cut):
                for ob, k, v in ops:
                    if ob == b:
                        toks.append("%s%r" % (k, v))
                toks.append("c%d" % s)
            subprocess.run([exe, fin, fau] + toks, check=True)
            out[name + "_x"] = q
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_ops"] = np.asarray([(b, SETTERS[k], v) for b, k, v in ops], np.float64).reshape(-1, 3)
            out[name + "_audio"] = np.fromfile(fau, np.float32)
            assert len(out[name + "_audio"]) == n
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "cw_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
