"""Records tests/golden/ifchain_ref.npz: the radio IF chain blocks of the reference (dsp/noise_reduction/noise_blanker.h and
power_squelch.h, compiled unmodified against oracle/shim) run over a handful of inputs.  Only the recorded DATA is committed; the
harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_ifchain_golden.py /path/to/SDRPlusPlus

Per case: input IF `x`, the block cut `cut` (sizes), blanker rate / level, squelch level, and the outputs of the blanker alone (`nb`),
the squelch alone (`sq`) and both in order (`both`)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dsp/noise_reduction/noise_blanker.h"
#include "dsp/noise_reduction/power_squelch.h"
// argv: in.bin out.bin mode(0 nb, 1 sq, 2 both) rate nb_level sq_level cut...
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n), t((size_t)n), y((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    const int mode = atoi(argv[3]);
    dsp::stream<dsp::complex_t> dummy;
    dsp::noise_reduction::NoiseBlanker nb;
    dsp::noise_reduction::PowerSquelch sq;
    nb.init(&dummy, atof(argv[4]), atof(argv[5]));
    sq.init(&dummy, atof(argv[6]));
    long pos = 0;
    for (int a = 7; a < argc; a++) {
        const int c = atoi(argv[a]);
        dsp::complex_t* in = x.data() + pos;
        if (mode == 0) { nb.process(c, in, y.data() + pos); }
        else if (mode == 1) { sq.process(c, in, y.data() + pos); }
        else {
            nb.process(c, in, t.data() + pos);
            sq.process(c, t.data() + pos, y.data() + pos);
        }
        pos += c;
    }
    if (pos != n) { return 3; }
    f = fopen(argv[2], "wb");
    fwrite(y.data(), sizeof(dsp::complex_t), (size_t)n, f);
    fclose(f);
    return 0;
}
"""


def signal(n, seed, impulses, fade):
    """tone 0.05 + noise sigma 0.004 (+ impulses of amplitude 2) (+ a silent stretch and a 60 dB fade)"""
    r = np.random.default_rng(seed)
    k = np.arange(n)
    x = 0.05 * np.exp(2j * np.pi * 0.013 * k) + 0.004 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    if fade:
        g = np.ones(n)
        g[n // 4:n // 4 + n // 8] = 0.0                        # silence (exact zeros: the blanker's inAmp == 0 branch, a -inf squelch block)
        g[n // 2:] = 10.0 ** (-3.0 * np.arange(n - n // 2) / (n - n // 2))  # 60 dB down over the second half
        x = x * g
    if impulses:
        at = r.choice(np.arange(200, n - 200), impulses, replace=False)
        x[at] += 2.0 * np.exp(2j * np.pi * r.random(impulses))
    return x.astype(np.complex64)


def cut_of(n, size):
    c = [size] * (n // size)
    if n % size:
        c.append(n % size)
    return c


CASES = [
    # name, n, seed, impulses, fade, if_rate, nb_level, sq_level, block
    ("impulses_l10", 720, 1, 6, False, 24000.0, 10.0, -20.0, 120),
    ("impulses_l3", 720, 2, 6, False, 24000.0, 3.0, -30.0, 120),
    ("fade_l10", 960, 3, 6, True, 24000.0, 10.0, -20.0, 120),
    ("fade_odd_cut", 750, 4, 5, True, 50000.0, 10.0, -30.0, 250),
    ("noise_l1p5", 300, 5, 0, False, 15000.0, 1.5, -20.0, 75),
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
        for name, n, seed, imp, fade, if_rate, nbl, sql, blk in CASES:
            x = signal(n, seed, imp, fade)
            cut = cut_of(n, blk)
            rate = 500.0 / if_rate
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            x.tofile(fin)
            out[name + "_x"] = x
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_par"] = np.asarray([rate, nbl, sql], np.float64)
            for mode, key in enumerate(("nb", "sq", "both")):
                subprocess.run([exe, fin, fout, str(mode), repr(rate), repr(nbl), repr(sql)] + [str(c) for c in cut], check=True)
                out[name + "_" + key] = np.fromfile(fout, np.complex64)
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "ifchain_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
