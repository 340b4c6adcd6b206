"""Records tests/golden/meteor_ref.npz: the reference's dsp::demod::Meteor (decoder_modules/meteor_demodulator/src/meteor_demod.h, compiled unmodified against
oracle/shim) run over a handful of 150 kS/s inputs, with the module's sink arithmetic (main.cpp:193-201) applied to its symbols.  Only the recorded DATA is
committed; the harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_meteor_golden.py /path/to/SDRPlusPlus [--time]

Inputs are complex baseband at 150 kS/s stored as int16, value / 16384 (exactly representable): random QPSK symbols at 72 000 symbols/s through a root-raised-
cosine pulse (beta 0.6, +-8 symbols; a symbol period is 25 and a sample period 12 ticks of a 1.8 MHz grid, so the pulse is evaluated exactly where it is
needed), times amp * exp(j (2 pi df t + phi)), plus noise.  The `oqpsk` and `mode` cases delay Q by half a symbol at the transmitter.  Per case:
    <name>_x        int16 [n, 2]  (`fresh` and `reset` read `steady`'s input and `reset_oqpsk` the beginning of `oqpsk`'s, as long as its cuts: <name>_xof names it)
    <name>_cut      the block schedule: samples per process() call
    <name>_ops      what was called in front of a block: int32 [k, 2] rows (block, op), op 1 = a fresh Meteor, 2 = reset(), 3 = setOQPSK(true)
    <name>_mode     broken, oqpsk the chain was initialised with
    <name>_soft     the complex soft symbols of all blocks, complex64 [m];  <name>_i8  int8 [m, 2];  <name>_counts  symbols per block
    <name>_dev_max  the reference's own SPREAD: K = 8 further runs, every input component multiplied by 1 +- 2^-24 with a random sign; per symbol and component
                    the largest |soft - soft_0| over the eight runs, float32 [m, 2]
and once, the members after the module's init (main.cpp:66; private: the harness reaches them by redefining the access keywords in front of the reference's
headers):
    agc    _setPoint, _maxGain, _rate, _initGain, _gain          loop   _alpha, _beta, phase, freq, _minFreq, _maxFreq, _minPhase, _maxPhase, phaseDelta, _initPhase, _initFreq
    taps   the root-raised-cosine taps, float32 [K]              mm     pcl.freq (omega), _minFreq, _maxFreq, _alpha (mu gain), _beta (omega gain)
    bank   the 128 x 8 interpolator bank, phase-major
The recorder asserts, per case (a case that fails gets another seed): all nine runs agree in every count and, over the second half, in the sign of every
component; over the second half the smallest |component| is at least 0.3 x the component RMS (`fresh`, `reset`, `reset_oqpsk` and `mode` start over in front of block 5, 2 or 4,
at or inside the second half: they are judged over the last quarter, where the chain has locked again); 4 x spread exceeds 1e-5 x RMS for at most 10 % of the symbols;
between runs at most 1 % of the int8 values differ, none by more than 1.

--time: also prints what Meteor::process costs on one CPU thread, per case (samples / s), for profiles/meteor_rate.md.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RATE = 150000.0
SYMRATE = 72000.0
BETA = 0.6
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
#include "meteor_demod.h"
#undef private
#undef protected
typedef dsp::demod::Meteor Meteor;
static Meteor* make(bool broken, bool oqpsk) {
    Meteor* d = new Meteor;
    d->init(NULL, 72000.0f, 150000, 33, 0.6f, 0.1f, 0.005f, broken, oqpsk, 1e-6, 0.01);  // (the module's call)
    return d;
}
// argv: in.bin soft.bin i8.bin counts.bin meta.bin reps broken oqpsk op...      op: c<count> | f (a fresh Meteor) | r (reset()) | o (setOQPSK(true))
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    const int reps = atoi(argv[6]);
    const bool broken = atoi(argv[7]) != 0, oqpsk = atoi(argv[8]) != 0;
    std::vector<dsp::complex_t> soft((size_t)n + 64);
    std::vector<int8_t> i8(2 * ((size_t)n + 64));
    std::vector<int> counts;
    double best = 1e30;
    for (int rep = 0; rep < reps; rep++) {
        Meteor* d = make(broken, oqpsk);
        if (rep == 0) {
            f = fopen(argv[5], "wb");
            float agc[5] = { d->agc._setPoint, d->agc._maxGain, d->agc._rate, d->agc._initGain, d->agc._gain };
            fwrite(agc, sizeof(float), 5, f);
            auto& l = d->costas;
            float lm[11] = { l.pcl._alpha, l.pcl._beta, l.pcl.phase, l.pcl.freq, l.pcl._minFreq, l.pcl._maxFreq, l.pcl._minPhase, l.pcl._maxPhase, l.pcl.phaseDelta, l._initPhase, l._initFreq };
            fwrite(lm, sizeof(float), 11, f);
            float mm[5] = { d->recov.pcl.freq, d->recov.pcl._minFreq, d->recov.pcl._maxFreq, d->recov.pcl._alpha, d->recov.pcl._beta };
            fwrite(mm, sizeof(float), 5, f);
            const float k = (float)d->rrcTaps.size;
            fwrite(&k, sizeof(float), 1, f);
            fwrite(d->rrcTaps.taps, sizeof(float), (size_t)d->rrcTaps.size, f);
            for (int p = 0; p < d->recov.interpBank.phaseCount; p++) { fwrite(d->recov.interpBank.phases[p], sizeof(float), (size_t)d->recov.interpBank.tapsPerPhase, f); }
            fclose(f);
        }
        counts.clear();
        long pos = 0, ns = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int a = 9; a < argc; a++) {
            if (argv[a][0] == 'f') { d = make(broken, oqpsk); }  // (the old one is left alone: its destructor would stop a block that never ran)
            else if (argv[a][0] == 'r') { d->reset(); }          // (no worker runs: tempStop / tempStart do nothing)
            else if (argv[a][0] == 'o') { d->setOQPSK(true); }
            else {
                const int v = atoi(argv[a] + 1);
                const int got = d->process(v, x.data() + pos, soft.data() + ns);
                counts.push_back(got);
                ns += got;
                pos += v;
            }
        }
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (pos != n) { return 3; }
        if (rep + 1 == reps) {
            // the module's sinkHandler (main.cpp:197-200)
            for (long i = 0; i < ns; i++) {
                i8[(size_t)(2 * i)] = std::clamp<int>(soft[(size_t)i].re * 84.0f, -127, 127);
                i8[(size_t)(2 * i) + 1] = std::clamp<int>(soft[(size_t)i].im * 84.0f, -127, 127);
            }
            f = fopen(argv[2], "wb"); fwrite(soft.data(), sizeof(dsp::complex_t), (size_t)ns, f); fclose(f);
            f = fopen(argv[3], "wb"); fwrite(i8.data(), 1, (size_t)(2 * ns), f); fclose(f);
            f = fopen(argv[4], "wb"); fwrite(counts.data(), sizeof(int), counts.size(), f); fclose(f);
        }
    }
    printf("%.9f\n", best);
    return 0;
}
"""


def rrc_pulse(t, beta):
    """the root-raised-cosine pulse at t symbol periods (unit energy up to a constant); t == 0 and |t| == 1 / (4 beta) by their limits"""
    t = np.asarray(t, np.float64)
    out = np.empty_like(t)
    z = np.abs(t) < 1e-12
    s = np.abs(np.abs(t) - 1.0 / (4.0 * beta)) < 1e-12
    g = ~(z | s)
    tg = t[g]
    out[g] = (np.sin(np.pi * tg * (1 - beta)) + 4 * beta * tg * np.cos(np.pi * tg * (1 + beta))) / (np.pi * tg * (1 - (4 * beta * tg) ** 2))
    out[z] = 1.0 - beta + 4 * beta / np.pi
    out[s] = beta / np.sqrt(2.0) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
    return out


def signal(n, seed, amp, df, sigma, q_delay=0.0):
    """-> int16 [n, 2]; q_delay: symbol periods the Q pulses are sent late"""
    r = np.random.default_rng(seed)
    span = 8
    tn = np.arange(n) * 12.0 / 25.0  # sample times in symbol periods, exact on the 1.8 MHz grid
    nsym = int(tn[-1]) + 2 * span + 2
    si = r.integers(0, 2, nsym) * 2.0 - 1.0
    sq = r.integers(0, 2, nsym) * 2.0 - 1.0
    k0 = np.floor(tn).astype(np.int64)
    bi = np.zeros(n)
    bq = np.zeros(n)
    for j in range(-span, span + 1):
        k = k0 + j
        bi += si[k + span] * rrc_pulse(tn - k, BETA)
        bq += sq[k + span] * rrc_pulse(tn - k - q_delay, BETA)
    base = (bi + 1j * bq) / np.sqrt(2.0)  # (|base| about 1 at a symbol's instant: amp is the order of the sample magnitude)
    t = np.arange(n) / RATE
    phi = r.uniform(0, 2 * np.pi)
    x = amp * base * np.exp(1j * (2 * np.pi * df * t + phi)) + sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))
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


OPS = {"f": 1, "r": 2, "o": 3}
CASES = [
    # name, n, seed, amp, df (Hz), noise sigma per component, block sizes (cycled), broken, oqpsk, Q delay at the transmitter, {block: op in front of it}
    ("steady", 6000, 1, 0.05, 0.0, 5e-4, [750], 0, 0, 0.0, {}),
    ("offset", 6000, 2, 0.05, 300.0, 2e-3, [750], 0, 0, 0.0, {}),
    ("noisy", 6000, 3, 0.05, -200.0, 5e-3, [750], 0, 0, 0.0, {}),
    ("weak", 6000, 4, 0.002, 100.0, 1e-4, [750], 0, 0, 0.0, {}),
    ("oqpsk", 6000, 5, 0.05, 100.0, 5e-4, [750], 0, 1, 0.5, {}),
    ("broken", 6000, 6, 0.05, 100.0, 5e-4, [750], 1, 0, 0.0, {}),
    ("cuts", 4000, 7, 0.05, 0.0, 5e-4, [997, 7, 1, 750], 0, 0, 0.0, {}),
    ("fresh", 6000, 1, 0.05, 0.0, 5e-4, [750], 0, 0, 0.0, {5: "f"}),
    ("reset", 6000, 1, 0.05, 0.0, 5e-4, [750], 0, 0, 0.0, {5: "r"}),
    ("reset_oqpsk", 3000, 5, 0.05, 100.0, 5e-4, [750], 0, 1, 0.5, {2: "r"}),  # (the first half of `oqpsk`'s input: lastI is visible in this mode only)
    ("mode", 6000, 10, 0.05, 100.0, 5e-4, [750], 0, 0, 0.5, {4: "o"}),  # (an OQPSK signal read as QPSK until the switch)
]


def sink(soft):
    """the module's sinkHandler in numpy: clamp<int>(v * 84.0f, -127, 127), the conversion truncating"""
    v = soft.view(np.float32).reshape(-1, 2) * np.float32(84.0)
    return np.clip(np.trunc(v), -127, 127).astype(np.int8)


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
                        "-I" + os.path.join(ref, "decoder_modules", "meteor_demodulator", "src"), "-o", exe, src, "-lpthread"], check=True)
        fin, fsoft, fi8, fcnt, fmeta = (os.path.join(tmp, k) for k in ("in.bin", "soft.bin", "i8.bin", "counts.bin", "meta.bin"))

        def run(x, toks, broken, oqpsk, reps=1):
            x.tofile(fin)
            r = subprocess.run([exe, fin, fsoft, fi8, fcnt, fmeta, str(reps), str(broken), str(oqpsk)] + toks, check=True, capture_output=True, text=True)
            return np.fromfile(fsoft, np.complex64), np.fromfile(fi8, np.int8).reshape(-1, 2), np.fromfile(fcnt, np.int32), float(r.stdout.strip())

        names = []
        for name, n, seed, amp, df, sigma, sizes, broken, oqpsk, qd, ops in CASES:
            q = signal(6000, seed, amp, df, sigma, qd)[:n]
            cut = schedule(n, sizes)
            x = (q.astype(np.float32) / np.float32(16384.0)).reshape(-1)  # interleaved re, im
            toks = []
            for b, s in enumerate(cut):
                if b in ops:
                    toks.append(ops[b])
                toks.append("c%d" % s)
            soft, i8, counts, secs = run(x, toks, broken, oqpsk, 20 if timing else 1)
            assert np.array_equal(i8, sink(soft)), "%s: the sink's arithmetic in numpy differs from the harness" % name
            if timing:
                print("%-8s %d samples, %d symbols: %.1f us per run, %.2f MS/s on one thread" % (name, n, len(soft), secs * 1e6, n / secs / 1e6))
            if "agc" not in out and not broken and not oqpsk:
                m = np.fromfile(fmeta, np.float32)
                out["agc"], out["loop"], out["mm"] = m[0:5], m[5:16], m[16:21]
                k = int(m[21])
                out["taps"] = m[22:22 + k].copy()
                out["bank"] = m[22 + k:].reshape(128, 8).copy()
            r = np.random.default_rng(1000 + seed)
            s0 = soft.view(np.float32).reshape(-1, 2).astype(np.float64)
            h = len(soft) // 2 if not ops else (3 * len(soft)) // 4  # (a case that starts over in mid-stream is judged where it has locked again)
            dev = np.zeros((K_SPREAD,) + s0.shape, np.float64)
            worst_i8 = 0.0
            for k in range(K_SPREAD):
                sgn = np.where(r.integers(0, 2, x.shape) == 1, 1.0, -1.0)
                xk = (x.astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32)
                sk, ik, ck, _ = run(xk, toks, broken, oqpsk)
                assert np.array_equal(ck, counts), "%s: run %d differs in its symbol counts: change the seed" % (name, k)
                sk = sk.view(np.float32).reshape(-1, 2).astype(np.float64)
                assert np.array_equal(sk[h:] > 0, s0[h:] > 0), "%s: run %d differs in a sign over the second half: change the seed" % (name, k)
                dd = np.abs(ik.astype(np.int32) - i8.astype(np.int32))
                assert dd.max() <= 1, "%s: run %d has an int8 value that differs by %d" % (name, k, dd.max())
                worst_i8 = max(worst_i8, float((dd != 0).mean()))
                dev[k] = sk - s0
            assert worst_i8 <= 0.01, "%s: %.4f of the int8 values differ between runs" % (name, worst_i8)
            dm = np.abs(dev).max(axis=0)
            rms = np.sqrt(np.mean(s0 ** 2))
            eye = np.abs(s0[h:]).min() / np.sqrt(np.mean(s0[h:] ** 2))
            assert eye >= 0.3, "%s: smallest |component| over the second half is %.3f of the RMS: change the seed" % (name, eye)
            above = float((4.0 * dm > 1e-5 * rms).any(axis=1).mean())
            assert above <= 0.10, "%s: 4 x spread exceeds the floor for %.3f of the symbols: change the seed" % (name, above)
            if name in ("fresh", "reset", "reset_oqpsk"):
                of = "oqpsk" if name == "reset_oqpsk" else "steady"
                assert np.array_equal(q, out[of + "_x"][:n])
                out[name + "_xof"] = np.asarray(of)  # (the same input, or its beginning: stored once)
            else:
                out[name + "_x"] = q
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_ops"] = np.asarray([[b, OPS[o]] for b, o in sorted(ops.items())], np.int32).reshape(-1, 2)
            out[name + "_mode"] = np.asarray([broken, oqpsk], np.int32)
            out[name + "_soft"] = soft
            out[name + "_i8"] = i8
            out[name + "_counts"] = counts
            out[name + "_dev_max"] = dm.astype(np.float32)
            print("%-8s symbols %d (%.1f / s), eye %.3f, spread median %.3g max %.3g, share above the floor %.4f, int8 differing between runs %.4f" % (
                name, len(soft), len(soft) / (n / RATE), eye, np.median(dm), dm.max(), above, worst_i8))
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "meteor_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
