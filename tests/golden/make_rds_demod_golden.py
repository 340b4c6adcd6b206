"""Records tests/golden/rds_demod_ref.npz: the reference's RDSDemod (decoder_modules/radio/src/rds_demod.h, compiled unmodified against oracle/shim) run over
a handful of 5 kS/s inputs.  Only the recorded DATA is committed; the harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_rds_demod_golden.py /path/to/SDRPlusPlus [--time]

Inputs are complex baseband at 5 kS/s stored as int16, value / 16384 (exactly representable): differentially encoded random bits, one sine period per bit with
the bit's sign (+-sin(2 pi frac(1187.5 t))), times amp * exp(j (2 pi df t + phi)), plus noise.  Per case:
    <name>_x        int16 [n, 2]
    <name>_tx       the data bits (before differential encoding), uint8
    <name>_cut      the block schedule: samples per process() call
    <name>_fresh    the blocks in front of which the chain was replaced by a fresh RDSDemod;  <name>_reset  the blocks in front of which reset() was called
    <name>_soft     the soft symbols of all blocks, float32 [m];  <name>_bits  uint8 [m];  <name>_counts  symbols per block
    <name>_dev_max  the reference's own SPREAD: K = 8 further runs, every input component multiplied by 1 +- 2^-24 with a random sign; per symbol the largest
                    |soft - soft_0| over the eight runs, float32 [m];  <name>_dev_rms  the RMS of all those deviations (one float64)
and once, the members after init (private: the harness reaches them by redefining the access keywords in front of the reference's headers):
    agc    _setPoint, _maxGain, _rate, _initGain, _gain                                      loop1 / loop2   _alpha, _beta, phase, freq, _minFreq, _maxFreq, _minPhase,
    taps   the band-pass's complex taps, complex64 [K]                                                      _maxPhase, phaseDelta, _initPhase, _initFreq
    mm     pcl.freq (omega), _minFreq, _maxFreq, _alpha (mu gain), _beta (omega gain)         bank    the 128 x 8 interpolator bank, phase-major
All nine runs of a case must agree in the per-block symbol counts and in every bit: the recorder asserts it (a case that does not gets another seed).

--time: also prints what RDSDemod::process costs on one CPU thread, per case (samples / s), for profiles/rds_demod_rate.md.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RATE = 5000.0
BAUD = 1187.5
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
#include "rds_demod.h"
#undef private
#undef protected
static void loop_members(dsp::loop::Costas<2>& l, float* m) {
    m[0] = l.pcl._alpha; m[1] = l.pcl._beta; m[2] = l.pcl.phase; m[3] = l.pcl.freq; m[4] = l.pcl._minFreq; m[5] = l.pcl._maxFreq;
    m[6] = l.pcl._minPhase; m[7] = l.pcl._maxPhase; m[8] = l.pcl.phaseDelta; m[9] = l._initPhase; m[10] = l._initFreq;
}
// argv: in.bin soft.bin bits.bin counts.bin meta.bin reps op...      op: c<count> | f (a fresh RDSDemod) | r (reset())
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    const int reps = atoi(argv[6]);
    std::vector<float> soft((size_t)n + 64);
    std::vector<uint8_t> bits((size_t)n + 64);
    std::vector<int> counts;
    double best = 1e30;
    for (int rep = 0; rep < reps; rep++) {
        dsp::stream<dsp::complex_t> dummy;
        RDSDemod* d = new RDSDemod;
        d->init(&dummy, true);
        if (rep == 0) {
            f = fopen(argv[5], "wb");
            float agc[5] = { d->agc._setPoint, d->agc._maxGain, d->agc._rate, d->agc._initGain, d->agc._gain };
            fwrite(agc, sizeof(float), 5, f);
            float lm[11];
            loop_members(d->costas, lm); fwrite(lm, sizeof(float), 11, f);
            loop_members(d->costas2, lm); fwrite(lm, sizeof(float), 11, f);
            float mm[5] = { d->recov.pcl.freq, d->recov.pcl._minFreq, d->recov.pcl._maxFreq, d->recov.pcl._alpha, d->recov.pcl._beta };
            fwrite(mm, sizeof(float), 5, f);
            const float k = (float)d->taps.size;
            fwrite(&k, sizeof(float), 1, f);
            fwrite(d->taps.taps, sizeof(dsp::complex_t), (size_t)d->taps.size, f);
            for (int p = 0; p < d->recov.interpBank.phaseCount; p++) { fwrite(d->recov.interpBank.phases[p], sizeof(float), (size_t)d->recov.interpBank.tapsPerPhase, f); }
            fclose(f);
        }
        counts.clear();
        long pos = 0, ns = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int a = 7; a < argc; a++) {
            if (argv[a][0] == 'f') {
                d = new RDSDemod;  // (the old one is left alone: its destructor would stop a block that never ran)
                d->init(&dummy, true);
            }
            else if (argv[a][0] == 'r') {
                // RDSDemod::reset() without the block's stop / start (no worker runs here)
                d->agc._gain = d->agc._initGain;
                d->costas.pcl.phase = d->costas._initPhase; d->costas.pcl.freq = d->costas._initFreq;
                dsp::buffer::clear<dsp::complex_t>(d->fir.buffer, d->fir._taps.size - 1);
                d->costas2.pcl.phase = d->costas2._initPhase; d->costas2.pcl.freq = d->costas2._initFreq;
                d->recov.offset = 0; d->recov.pcl.phase = 0.0f; d->recov.pcl.freq = d->recov._omega; d->recov.lastOut = 0.0f;
                d->diff.last = d->diff._initSym;
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
        }
    }
    printf("%.9f\n", best);
    return 0;
}
"""


def signal(n, seed, amp, df, sigma):
    """-> (int16 [n, 2], data bits uint8)"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    nb = int(n / RATE * BAUD) + 2
    data = r.integers(0, 2, nb).astype(np.uint8)
    enc = np.bitwise_xor.accumulate(data)
    sym = t * BAUD
    k = np.floor(sym).astype(np.int64)
    base = np.where(enc[k] == 1, 1.0, -1.0) * np.sin(2 * np.pi * (sym - k))
    phi = r.uniform(0, 2 * np.pi)
    x = amp * base * np.exp(1j * (2 * np.pi * df * t + phi)) + sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))
    q = np.empty((n, 2), np.int16)
    q[:, 0] = np.rint(x.real * 16384.0)
    q[:, 1] = np.rint(x.imag * 16384.0)
    return q, data


def schedule(n, sizes):
    out, pos, k = [], 0, 0
    while pos < n:
        s = min(sizes[k % len(sizes)], n - pos)
        out.append(s)
        pos += s
        k += 1
    return out


CASES = [
    # name, n, seed, amp, df (Hz), noise sigma per component, block sizes (cycled), blocks with a fresh chain in front, blocks with reset() in front
    ("steady", 20000, 1, 0.05, 0.0, 5e-4, [1250], [], []),
    ("offset", 20000, 2, 0.05, 3.0, 2e-3, [1250], [], []),
    ("noisy", 20000, 3, 0.05, -2.0, 1e-2, [1250], [], []),
    ("weak", 20000, 4, 0.002, 1.0, 1e-4, [1250], [], []),
    ("cuts", 12000, 5, 0.05, 0.0, 5e-4, [997, 7, 1, 1250], [], []),
    ("fresh", 8000, 6, 0.05, 1.0, 5e-4, [1000], [5], []),
    ("reset", 8000, 7, 0.05, 1.0, 5e-4, [1000], [], [5]),
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
                        "-I" + os.path.join(ref, "decoder_modules", "radio", "src"), "-o", exe, src, "-lpthread"], check=True)
        fin, fsoft, fbits, fcnt, fmeta = (os.path.join(tmp, k) for k in ("in.bin", "soft.bin", "bits.bin", "counts.bin", "meta.bin"))

        def run(x, toks, reps=1):
            x.tofile(fin)
            r = subprocess.run([exe, fin, fsoft, fbits, fcnt, fmeta, str(reps)] + toks, check=True, capture_output=True, text=True)
            return np.fromfile(fsoft, np.float32), np.fromfile(fbits, np.uint8), np.fromfile(fcnt, np.int32), float(r.stdout.strip())

        names = []
        for name, n, seed, amp, df, sigma, sizes, fresh, resets in CASES:
            q, data = signal(n, seed, amp, df, sigma)
            cut = schedule(n, sizes)
            x = (q.astype(np.float32) / np.float32(16384.0)).reshape(-1)  # interleaved re, im
            toks = []
            for b, s in enumerate(cut):
                if b in fresh:
                    toks.append("f")
                if b in resets:
                    toks.append("r")
                toks.append("c%d" % s)
            soft, bits, counts, secs = run(x, toks, 20 if timing else 1)
            if timing:
                print("%-8s %d samples, %d symbols: %.1f us per run, %.2f MS/s on one thread" % (name, n, len(soft), secs * 1e6, n / secs / 1e6))
            if "agc" not in out:
                m = np.fromfile(fmeta, np.float32)
                out["agc"], out["loop1"], out["loop2"], out["mm"] = m[0:5], m[5:16], m[16:27], m[27:32]
                k = int(m[32])
                out["taps"] = m[33:33 + 2 * k].view(np.complex64).copy()
                out["bank"] = m[33 + 2 * k:].reshape(128, 8).copy()
            r = np.random.default_rng(1000 + seed)
            dev = np.zeros((K_SPREAD, len(soft)), np.float64)
            for k in range(K_SPREAD):
                sgn = np.where(r.integers(0, 2, x.shape) == 1, 1.0, -1.0)
                xk = (x.astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32)
                sk, bk, ck, _ = run(xk, toks)
                assert np.array_equal(ck, counts), "%s: run %d differs in its symbol counts: change the seed" % (name, k)
                assert np.array_equal(bk, bits), "%s: run %d differs in a bit: change the seed" % (name, k)
                dev[k] = sk.astype(np.float64) - soft.astype(np.float64)
            out[name + "_x"] = q
            out[name + "_tx"] = data
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_fresh"] = np.asarray(fresh, np.int32)
            out[name + "_reset"] = np.asarray(resets, np.int32)
            out[name + "_soft"] = soft
            out[name + "_bits"] = bits
            out[name + "_counts"] = counts
            out[name + "_dev_max"] = np.abs(dev).max(axis=0).astype(np.float32)
            out[name + "_dev_rms"] = np.float64(np.sqrt(np.mean(dev * dev)))
            dm = np.abs(dev).max(axis=0)
            half = soft[len(soft) // 2:].astype(np.float64)
            print("%-8s symbols %d (%.1f / s), min |soft| / rms in the second half %.3f, spread median %.3g max %.3g, share above 1e-3: %.4f, rms %.3g" % (
                name, len(soft), len(soft) / (n / RATE), np.abs(half).min() / np.sqrt(np.mean(half ** 2)), np.median(dm), dm.max(), float((dm > 1e-3).mean()), out[name + "_dev_rms"]))
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "rds_demod_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
