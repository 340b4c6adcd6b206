"""Records tests/golden/pager_ref.npz: the reference's POCSAGDSP (decoder_modules/pager_decoder/src/pocsag/dsp.h, compiled unmodified against oracle/shim)
run over a handful of IF-rate inputs.  Only the recorded DATA is committed; the harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_pager_golden.py /path/to/SDRPlusPlus [--time]

Inputs are IF-rate I/Q (24 kS/s) stored as int16, value / 16384 (exactly representable): 2FSK at +-4500 Hz, amplitude 0.06, random bits, and noise.  Per case:
    <name>_x        int16 [n, 2]
    <name>_baud     the baud rate POCSAGDSP::init was given (sample rate 24000)
    <name>_cut      the block schedule: samples per process() call
    <name>_reset    the blocks in front of which the chain was replaced by a fresh POCSAGDSP (what attaching the branch anew, or sdrpp_vfo_reset, stands for)
    <name>_soft     the soft symbols of all blocks, float32 [m];  <name>_bits  uint8 [m];  <name>_counts  symbols per block
    <name>_pcl      after init: pcl.freq (omega), _minFreq, _maxFreq, _alpha (mu gain), _beta (omega gain), and the discriminator's _invDeviation — six float32
                    (private members: the harness reaches them by redefining the access keywords in front of the reference's headers)
    <name>_dev_max  the reference's own SPREAD: K = 8 further runs, every input sample (both parts) multiplied by 1 +- 2^-24 with a random sign; per symbol the
                    largest |soft - soft_0| over the eight runs, float32 [m];  <name>_dev_rms  the RMS of all those deviations (one float64)
and once: `bank`, the 128 x 8 interpolator bank as MM::generateInterpTaps builds it, phase-major.
All nine runs of a case must agree in the per-block symbol counts and in every bit: the recorder asserts it (a case that does not gets another seed — the
fixture never depends on a coin toss).

--time: also prints what POCSAGDSP::process costs on one CPU thread, per case (samples / s), for profiles/pager_rate.md.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RATE = 24000.0
K_SPREAD = 8

HARNESS = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include <volk/volk.h>
#define private public
#define protected public
#include "pocsag/dsp.h"
#undef private
#undef protected
// argv: in.bin soft.bin bits.bin counts.bin meta.bin bank.bin baud reps op...      op: c<count> | r (a fresh POCSAGDSP)
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    const double baud = atof(argv[7]);
    const int reps = atoi(argv[8]);
    std::vector<float> soft((size_t)n + 64);
    std::vector<uint8_t> bits((size_t)n + 64);
    std::vector<int> counts;
    float meta[6] = {};
    double best = 1e30;
    for (int rep = 0; rep < reps; rep++) {
        dsp::stream<dsp::complex_t> dummy;
        POCSAGDSP* d = new POCSAGDSP;
        d->init(&dummy, 24000.0, baud);
        meta[0] = d->recov.pcl.freq; meta[1] = d->recov.pcl._minFreq; meta[2] = d->recov.pcl._maxFreq;
        meta[3] = d->recov.pcl._alpha; meta[4] = d->recov.pcl._beta; meta[5] = d->demod._invDeviation;
        if (rep == 0) {
            f = fopen(argv[6], "wb");
            for (int p = 0; p < d->recov.interpBank.phaseCount; p++) { fwrite(d->recov.interpBank.phases[p], sizeof(float), (size_t)d->recov.interpBank.tapsPerPhase, f); }
            fclose(f);
        }
        counts.clear();
        long pos = 0, ns = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int a = 9; a < argc; a++) {
            if (argv[a][0] == 'r') {
                d = new POCSAGDSP;  // (the old one is left alone: its destructor would stop a block that never ran)
                d->init(&dummy, 24000.0, baud);
            }
            else {
                const int v = atoi(argv[a] + 1);
                const int got = d->process(v, x.data() + pos, soft.data() + ns, bits.data() + ns);
                counts.push_back(got);
                ns += got;
                pos += v;
            }
        }
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (pos != n) { return 3; }
        if (rep + 1 == reps) {
            f = fopen(argv[2], "wb"); fwrite(soft.data(), sizeof(float), (size_t)ns, f); fclose(f);
            f = fopen(argv[3], "wb"); fwrite(bits.data(), 1, (size_t)ns, f); fclose(f);
            f = fopen(argv[4], "wb"); fwrite(counts.data(), sizeof(int), counts.size(), f); fclose(f);
            f = fopen(argv[5], "wb"); fwrite(meta, sizeof(float), 6, f); fclose(f);
        }
    }
    printf("%.9f\n", best);
    return 0;
}
"""


def signal(n, seed, baud, sigma):
    r = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    bits = r.integers(0, 2, int(n / RATE * baud) + 2)
    f = np.where(bits[(t * baud).astype(np.int64)] == 1, 4500.0, -4500.0)
    x = 0.06 * np.exp(1j * 2 * np.pi * np.cumsum(f) / RATE) + sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))
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
    # name, n, seed, baud, noise sigma per component, block sizes (cycled), blocks with a fresh chain in front of them
    ("steady_2400", 6000, 1, 2400.0, 0.0005, [500], []),
    ("steady_1200", 6000, 2, 1200.0, 0.006, [500], []),
    ("steady_512", 8000, 3, 512.0, 0.006, [500], []),
    ("noisy_2400", 6000, 4, 2400.0, 0.02, [500], []),
    ("cuts", 5000, 5, 1200.0, 0.006, [997, 7, 1, 1250], []),
    ("reset", 6000, 6, 2400.0, 0.006, [500], [5]),
]


def main():
    args = [a for a in sys.argv[1:] if a != "--time"]
    timing = "--time" in sys.argv[1:]
    if len(args) != 1:
        sys.exit(__doc__)
    ref = args[0]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "h.cpp"), os.path.join(tmp, "h")
        with open(src, "w") as f:
            f.write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "core", "src"),
                        "-I" + os.path.join(ref, "decoder_modules", "pager_decoder", "src"), "-o", exe, src, "-lpthread"], check=True)
        fin, fsoft, fbits, fcnt, fmeta, fbank = (os.path.join(tmp, k) for k in ("in.bin", "soft.bin", "bits.bin", "counts.bin", "meta.bin", "bank.bin"))

        def run(x, baud, toks, reps=1):
            x.tofile(fin)
            r = subprocess.run([exe, fin, fsoft, fbits, fcnt, fmeta, fbank, repr(baud), str(reps)] + toks, check=True, capture_output=True, text=True)
            return np.fromfile(fsoft, np.float32), np.fromfile(fbits, np.uint8), np.fromfile(fcnt, np.int32), float(r.stdout.strip())

        names = []
        for name, n, seed, baud, sigma, sizes, resets in CASES:
            q = signal(n, seed, baud, sigma)
            cut = schedule(n, sizes)
            x = (q.astype(np.float32) / np.float32(16384.0)).reshape(-1)  # interleaved re, im
            toks = []
            for b, s in enumerate(cut):
                if b in resets:
                    toks.append("r")
                toks.append("c%d" % s)
            soft, bits, counts, secs = run(x, baud, toks, 20 if timing else 1)
            if timing:
                print("%-12s %d samples, %d symbols: %.1f us per run, %.2f MS/s on one thread" % (name, n, len(soft), secs * 1e6, n / secs / 1e6))
            assert np.array_equal(bits, (soft > 0.0).astype(np.uint8))
            meta = np.fromfile(fmeta, np.float32)
            bank = np.fromfile(fbank, np.float32).reshape(128, 8)
            if "bank" in out:
                assert np.array_equal(out["bank"], bank)
            out["bank"] = bank
            r = np.random.default_rng(1000 + seed)
            dev = np.zeros((K_SPREAD, len(soft)), np.float64)
            for k in range(K_SPREAD):
                sgn = np.where(r.integers(0, 2, x.shape) == 1, 1.0, -1.0)
                xk = (x.astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32)
                sk, bk, ck, _ = run(xk, baud, toks)
                assert np.array_equal(ck, counts), "%s: run %d differs in its symbol counts: change the seed" % (name, k)
                assert np.array_equal(bk, bits), "%s: run %d differs in a bit: change the seed" % (name, k)
                dev[k] = sk.astype(np.float64) - soft.astype(np.float64)
            out[name + "_x"] = q
            out[name + "_baud"] = np.float64(baud)
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_reset"] = np.asarray(resets, np.int32)
            out[name + "_soft"] = soft
            out[name + "_bits"] = bits
            out[name + "_counts"] = counts
            out[name + "_pcl"] = meta
            out[name + "_dev_max"] = np.abs(dev).max(axis=0).astype(np.float32)
            out[name + "_dev_rms"] = np.float64(np.sqrt(np.mean(dev * dev)))
            print("%-12s symbols %d, weak (|soft| < 0.05) %d, spread max %.3g rms %.3g, soft rms %.3f" % (
                name, len(soft), int((np.abs(soft) < 0.05).sum()), np.abs(dev).max(), out[name + "_dev_rms"], np.sqrt(np.mean(soft.astype(np.float64) ** 2))))
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "pager_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
